"""The seams of the index kernels' launch geometry (kvcached_amd/csrc/index_kernels.hip): the cases that sit on each of them,
a second reference for alloc_extend / alloc_decode, and the sweeps that hold an operation against the expected values.

The seeded cases of tests/kvc_glue_cases.py draw their lengths at random; what they reach is a matter of luck (no request longer
than one token group, no sweep that starts above bitmap word 0, no full bitmap word but word 0, no empty wave in front of a block-opening
one: tests/test_index_edges.py computes that). Here every length is chosen: each list below names one seam and the values on
both sides of it. Every sweep takes the operation as a callable: tests/test_gpu_index_edges.py hands in the kernels (through
the C ABI and through the wrappers of integration/sglang/allocators.py), tests/test_index_edges.py numpy stand-ins - the oracle
(the sweeps must pass) and seven wrong ones (the sweeps must fail, naming the first bad element).

Everything is int64 and compared bit for bit, every element, against oracle/sglang_glue.py: expand and unique directly; extend
and decode through `ref_extend`, a vectorised per-position statement that tests/test_index_edges.py pins to the oracle's loops
on every case here (the loops are too slow to be run once per GPU test). Parity with SGLang's own alloc_extend / alloc_decode
kernels stays UNPINNED, as oracle/sglang_glue.py says: SGLang is not available to these tests.

An output buffer is GUARD sentinel words, the payload, GUARD sentinel words. An operation is `op(case, buf) -> buf after the
call`; it must write the payload at buf[GUARD:], and both guards and every payload element it has no business writing must
still hold the sentinel afterwards."""
import functools
import os
import sys
import zlib

import numpy as np

import kvc_glue_cases as G

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
import sglang_glue as O  # noqa: E402

# ------------------------------------------------------------------ the launch constants, once
THREADS = 256                 # __launch_bounds__(256) of expand / alloc_extend / alloc_decode / mark_blocks, `blockIdx.x * 256`
LANES = 64                    # `wave = threadIdx.x >> 6, lane = threadIdx.x & 63`
WAVES = THREADS // LANES      # wave_cnt[4] in alloc_decode_kernel
IDS_PER_LAUNCH = 1024         # kMaxIdsPerLaunch (kernels.hpp): ids in the kernarg segment; above it expand launches again and
#                               extend / decode stage the ids in a device buffer (gpu_context.cpp: StagedIds)
EXTEND_GROUP = 4096           # kExtendTokensPerGroup: tokens of one request per blockIdx.y
SWEEP_CHUNK_WORDS = 1024      # sweep_blocks_kernel: `w0 += 1024`, one word per thread of its 1024
BLOCKS_PER_WORD = 32          # mark_blocks_kernel: `w = b >> 5`, `bit = 1u << (b & 31u)`
SWEEP_CHUNK_BLOCKS = SWEEP_CHUNK_WORDS * BLOCKS_PER_WORD     # 32768
MIN_BITMAP_WORDS = 4096       # GpuContext::unique_block_ids: `std::max<size_t>(words, 4096)`

GUARD = 256
SENTINEL = np.int64(-0x5E5E5E5E5E5E5E5E)     # every value an index operation produces is >= 0: no case can produce this
MISSING = np.int64(-(1 << 40))               # stands for a block id the caller left out (the stand-ins' id lists are padded with it)


class Refused(Exception):
    """What a numpy stand-in of unique_block_ids raises for an index outside [0, n_blocks * tpb)."""


def _seed(name):
    return zlib.crc32(name.encode())


def guarded(n):
    return np.full(GUARD + n + GUARD, SENTINEL, dtype=np.int64)


# ------------------------------------------------------------------ the second reference
def ref_extend(prefix_lens, seq_lens, owned, free_pages, tpb):
    """Position p of request i lies in block blocks_i[p // tpb] at offset p % tpb, where blocks_i are the blocks the request
    owns followed by its share of the new ones (consumed in request order): check_extend_invariants, all positions at once.
    Unlike the oracle it never looks at last_loc. -> (slot per output position, index into free_pages of the block it lies in
    or -1 for a block of the prefix, request per position, token of the request per position)."""
    pre, seq = np.asarray(prefix_lens, dtype=np.int64), np.asarray(seq_lens, dtype=np.int64)
    free_pages = np.asarray(free_pages, dtype=np.int64)
    ext, bs = seq - pre, len(pre)
    n_pre = -(-pre // tpb)
    n_new = -(-seq // tpb) - n_pre
    new_start = np.cumsum(n_new) - n_new
    rows = n_pre + n_new
    row_start = np.cumsum(rows) - rows
    table = np.empty(int(rows.sum()), dtype=np.int64)
    for i in range(bs):
        a, b = int(row_start[i]), int(row_start[i] + n_pre[i])
        assert len(owned[i]) == n_pre[i]
        table[a:b] = owned[i]
        table[b:int(row_start[i] + rows[i])] = free_pages[int(new_start[i]):int(new_start[i] + n_new[i])]
    assert int(n_new.sum()) == len(free_pages)
    req = np.repeat(np.arange(bs), ext)
    t = np.arange(int(ext.sum()), dtype=np.int64) - (np.cumsum(ext) - ext)[req]
    pos = pre[req] + t
    blk = pos // tpb
    val = table[row_start[req] + blk] * tpb + pos % tpb
    k = np.where(blk >= n_pre[req], new_start[req] + blk - n_pre[req], -1)
    return val, k, req, t


# ------------------------------------------------------------------ comparing a buffer
def check_buffer(label, case, got, mode="raw"):
    """`got` is the whole buffer after the call. mode "raw": guards and payload, every element. "payload": the payload only -
    all that a caller sees who allocates `out` exactly, as the wrappers do and tests/test_gpu_sglang_glue.py with them.
    "written": only the elements the operation must write (an output that was never filled with the sentinel)."""
    want, name = case["want"], case["name"]
    full = guarded(len(want))
    full[GUARD:GUARD + len(want)] = want
    assert got.dtype == np.int64 and got.shape == full.shape, (label, name, got.dtype, got.shape, full.shape)
    differs = got != full
    if mode != "raw":
        differs[:GUARD] = differs[GUARD + len(want):] = False
    if mode == "written":
        differs &= full != SENTINEL
    bad = np.flatnonzero(differs)
    if bad.size:
        i = int(bad[0]) - GUARD
        place = f"guard word {i}" if i < 0 else f"guard word {i - len(want)} behind the payload" if i >= len(want) \
            else f"element {i} ({case['where'](i)})"
        w = "the sentinel" if full[bad[0]] == SENTINEL else int(full[bad[0]])
        g = "the sentinel" if got[bad[0]] == SENTINEL else int(got[bad[0]])
        raise AssertionError(f"{label} {name}: {place}: got {g}, want {w} ({bad.size} elements differ)")


def _sweep(op, cases, label, mode):
    for case in cases:
        assert not (case["reference"] == SENTINEL).any(), case["name"]      # the sentinel is a value no case produces
        check_buffer(label, case, op(case, guarded(len(case["want"]))), mode)


# ------------------------------------------------------------------ expand
EXPAND_TPBS = [1, 3, 5, 16, 48, 255, 256, 257, 1000]
EXPAND_REMAINDERS = [0, 1, 255]                           # total % 256: the last workgroup full, one thread, all but one
EXPAND_CHUNK_NS = [1023, 1024, 1025, 2047, 2048, 2049]    # around one and two launches of IDS_PER_LAUNCH ids


def expand_shapes():
    shapes = [(0, 16)]
    for tpb in EXPAND_TPBS:
        shapes.append((1, tpb))
        for rem in EXPAND_REMAINDERS:                     # (no n exists where gcd(tpb, 256) does not divide the remainder)
            n = next((n for n in range(2, 2 * THREADS + 2) if n * tpb % THREADS == rem), None)
            if n is not None:
                shapes.append((n, tpb))
    return shapes + [(n, tpb) for tpb in (1, 3) for n in EXPAND_CHUNK_NS]


def make_expand(name, ids, tpb):
    ids = np.asarray(ids, dtype=np.int64)
    want = O.expand_block_ids(ids, tpb)
    want.flags.writeable = False
    return dict(name=name, ids=ids, tpb=tpb, want=want, reference=want, where=lambda i: f"id {i // tpb} token {i % tpb}")


@functools.lru_cache(maxsize=None)
def expand_cases():
    return [make_expand(f"expand_n{n}_t{tpb}", np.random.default_rng(_seed(f"e{n}_{tpb}")).permutation(1 << 16)[:n], tpb)
            for n, tpb in expand_shapes()]


def sweep_expand(op, label, mode="raw", cases=None):
    _sweep(op, expand_cases() if cases is None else cases, label, mode)


# ------------------------------------------------------------------ extend
EXTEND_LENS = [0, 1, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193]
PHASE_TPBS = [1, 2, 3, 16, 48, 64, 4096, 5000]
EXTEND_BS = [1, 2, 255, 256, 257, 258, 512, 513]
NEW_BLOCK_TOTALS = [0, 1, 1023, 1024, 1025]


def extend_dict(name, c, cut=0, out_len=None):
    """A case of kvc_glue_cases.extend_case in the form the sweeps take. `cut` new block ids are left off the end of the list
    that is handed over, `out_len` is handed over as extend_num_tokens (default: the sum of the extensions). The payload is
    as long as the sum, so that a write at or past a smaller extend_num_tokens lands where it is seen."""
    tpb = c["tpb"]
    val, k, req, t = ref_extend(c["prefix_lens"], c["seq_lens"], c["owned"], c["free_pages"], tpb)
    ids = c["free_pages"][:len(c["free_pages"]) - cut]
    out_len = len(val) if out_len is None else out_len
    assert 0 <= out_len <= len(val) and 0 <= cut <= len(c["free_pages"])
    want = val.copy()
    want[k >= len(ids)] = SENTINEL
    want[out_len:] = SENTINEL
    want.flags.writeable = val.flags.writeable = False
    return dict(name=name, tpb=tpb, prefix_lens=c["prefix_lens"], seq_lens=c["seq_lens"], last_loc=c["last_loc"], ids=ids,
                free_pages=c["free_pages"], owned=c["owned"], out_len=out_len, want=want, reference=val,
                where=lambda i: f"request {int(req[i])} token {int(t[i])}")


def make_extend(name, tpb, pre, ext, cut=0, out_len=None):
    pre, ext = np.asarray(pre, dtype=np.int64), np.asarray(ext, dtype=np.int64)
    n_ids = int((-(-(pre + ext) // tpb)).sum())
    c = G.extend_case(seed=_seed(name), bs=len(pre), tpb=tpb, n_blocks=2 * n_ids + 64, prefix_lens=pre, extend_lens=ext)
    return extend_dict(name, c, cut, out_len)


@functools.lru_cache(maxsize=None)
def extend_cases():
    cs = [make_extend(f"alone_ext{n}", 16, [5], [n]) for n in EXTEND_LENS]
    # a long request between short and empty ones, in both orders: what comes behind it starts where it ends
    pre, ext = [0, 7, 16, 33, 15, 1], [3, 0, None, 0, 17, 1]
    for n in EXTEND_LENS[5:]:
        e = [n if x is None else x for x in ext]
        cs.append(make_extend(f"mixed_ext{n}", 16, pre, e))
        cs.append(make_extend(f"mixed_reversed_ext{n}", 16, pre[::-1], e[::-1]))
    # extend_num_tokens on the group count: 4096 k and 4096 k + 1
    cs.append(make_extend("total4096", 16, [3, 0, 20, 16], [1000, 0, 3000, 96]))
    cs.append(make_extend("total4097", 16, [3, 0, 20, 16], [1000, 0, 3000, 97]))
    cs.append(make_extend("total8192", 16, [0, 5, 16], [4000, 0, 4192]))
    cs.append(make_extend("total8193", 16, [0, 5, 16], [4000, 1, 4192]))
    # the prefix's phase against the block, and an extension that stays inside the last partial block, fills it, goes one past
    for tpb in PHASE_TPBS:
        pre, ext = [], []
        for phase in sorted({0, 1 % tpb, tpb - 1}):
            p = 2 * tpb + phase
            room = -p % tpb
            for e in sorted({room - 1, room, room + 1} if room else {1, tpb, tpb + 1}):
                if e >= 0:
                    pre.append(p)
                    ext.append(e)
        cs.append(make_extend(f"phase_t{tpb}", tpb, pre, ext))
    for tpb in (4096, 5000):                              # a block that lies on both sides of a group seam
        cs.append(make_extend(f"straddle_t{tpb}", tpb, [2 * tpb + phase for phase in (0, 1, tpb - 1)], [8193] * 3))
    for bs in EXTEND_BS:                                  # the prefix sums over j < r, strided by 256
        r = np.arange(bs)
        cs.append(make_extend(f"bs{bs}", 16, r * 3 % 40, r * 7 % 5))
    cs.append(make_extend("newblocks0", 16, [3, 5], [2, 4]))                  # no id at all: a NULL id pointer
    cs.append(make_extend("newblocks1", 16, [3], [14]))
    for n in NEW_BLOCK_TOTALS[2:]:                        # the last count in the kernarg segment, the first staged one
        cs.append(make_extend(f"newblocks{n}", 1, [2, 0, 1], [500, n - 1000, 500]))
    # inconsistent input, which the kernel's guards make safe: what cannot be computed keeps the sentinel
    pre, ext = [5, 0, 16, 31, 3], [20, 40, 0, 33, 4097]
    share = -(-(pre[-1] + ext[-1]) // 16) - -(-pre[-1] // 16)
    total = sum(ext)
    cs.append(make_extend("ids_short_by_1", 16, pre, ext, cut=1))
    cs.append(make_extend("ids_short_by_a_request", 16, pre, ext, cut=share))
    for out_len in (total - 1, total - 100, EXTEND_GROUP, 1):
        cs.append(make_extend(f"out_len_{total}_minus_{total - out_len}", 16, pre, ext, out_len=out_len))
    return cs


def sweep_extend(op, label, mode="raw", cases=None):
    _sweep(op, extend_cases() if cases is None else cases, label, mode)


# ------------------------------------------------------------------ decode
DECODE_BS = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 769]
DECODE_MASKS = {                                          # which requests r of a batch of bs open a block
    "none": lambda r, bs: r < 0,
    "all": lambda r, bs: r >= 0,
    "lane0": lambda r, bs: r % LANES == 0,
    "lane63": lambda r, bs: r % LANES == LANES - 1,
    "wave0": lambda r, bs: r % THREADS // LANES == 0,     # one wave of each workgroup: empty waves before, between, after
    "wave1": lambda r, bs: r % THREADS // LANES == 1,
    "wave2": lambda r, bs: r % THREADS // LANES == 2,
    "wave3": lambda r, bs: r % THREADS // LANES == 3,
    "waves0and2": lambda r, bs: r % THREADS // LANES % 2 == 0,      # an empty wave between two that are not
    "waves0and3": lambda r, bs: r % THREADS // LANES % 3 == 0,
    "first_and_last": lambda r, bs: (r == 0) | (r == bs - 1),
    "last": lambda r, bs: r == bs - 1,
    "first": lambda r, bs: r == 0,
    "alternating": lambda r, bs: r % 2 == 0,
    "last_workgroup": lambda r, bs: r // THREADS == (bs - 1) // THREADS,
}
DECODE_STAGED_BS = [1023, 1024, 1025]                     # tokens_per_block 1: as many new blocks as requests


def opens_block(seq_lens, tpb):
    return (np.asarray(seq_lens) - 1) % tpb == 0


def decode_dict(name, c, cut=0):
    tpb, seq = c["tpb"], c["seq_lens"]
    val, k, req, _ = ref_extend(seq - 1, seq, c["owned"], c["free_pages"], tpb)
    ids = c["free_pages"][:len(c["free_pages"]) - cut]
    want = val.copy()
    want[k >= len(ids)] = SENTINEL
    want.flags.writeable = val.flags.writeable = False
    return dict(name=name, tpb=tpb, seq_lens=seq, last_loc=c["last_loc"], ids=ids, free_pages=c["free_pages"], want=want,
                reference=val, where=lambda i: f"request {i}")


def make_decode(name, tpb, seq, cut=0):
    seq = np.asarray(seq, dtype=np.int64)
    c = G.decode_case(seed=_seed(name), bs=len(seq), tpb=tpb, n_blocks=2 * int((-(-seq // tpb)).sum()) + 64, seq_lens=seq)
    return decode_dict(name, c, cut)


def masked_seq_lens(name, mask, tpb):
    """Lengths of 1 .. 4 blocks: k * tpb + 1 where the request opens a block (1, with last_loc -1, among them), else anything
    but."""
    rng = np.random.default_rng(_seed(name))
    whole = rng.integers(0, 4, size=len(mask)) * tpb
    return np.where(mask, whole + 1, whole + rng.integers(2, tpb + 1, size=len(mask)))


@functools.lru_cache(maxsize=None)
def decode_cases():
    cs = []
    for bs in DECODE_BS:
        for m, f in DECODE_MASKS.items():
            name = f"decode_bs{bs}_{m}"
            cs.append(make_decode(name, 16, masked_seq_lens(name, f(np.arange(bs), bs), 16)))
    for bs in DECODE_STAGED_BS:
        cs.append(make_decode(f"decode_bs{bs}_t1", 1, np.random.default_rng(bs).integers(1, 50, size=bs)))
    cs.append(make_decode("decode_first_tokens", 16, [1] * 5))                # seq_len 1, last_loc -1
    cs.append(make_decode("decode_first_tokens_t1", 1, [1] * 3))
    name = "decode_ids_short_by_1"
    cs.append(make_decode(name, 16, masked_seq_lens(name, np.arange(300) % 2 == 0, 16), cut=1))
    return cs


def sweep_decode(op, label, mode="raw", cases=None):
    _sweep(op, decode_cases() if cases is None else cases, label, mode)


# ------------------------------------------------------------------ unique
UNIQUE_TPBS = [1, 16]
RANGE_LOS = [0, 1, 1023, 1024, 1025, 3000]                # first touched bitmap word
RANGE_LENS = [1, 2, 1023, 1024, 1025, 2048, 2049]         # touched words: around one and two chunks of the sweep
FILLINGS = ["ends", "seams", "dense", "dense_with_gaps"]
GAP_EVERY = 3


def range_blocks(lo, n_words, filling):
    """The blocks of one query that touches exactly the words [lo, lo + n_words - 1]."""
    words = lo + np.arange(n_words, dtype=np.int64)
    if filling == "ends":                                 # one block in the first word, one in the last
        return np.array([words[0] * 32 + 5, words[-1] * 32 + 17])
    if filling == "seams":                                # bits 0 and 31 on both sides of every wave seam (relative word
        rel = {0, n_words - 1}                            # 63|64; the chunk seams 1023|1024 are among them) and at both ends
        for s in range(LANES, n_words, LANES):
            rel |= {s - 1, s}
        w = lo + np.array(sorted(rel), dtype=np.int64)
        return np.sort(np.concatenate([w * 32, w * 32 + 31]))
    if filling == "dense_with_gaps":                      # every GAP_EVERY-th word empty, the two ends never
        rel = np.arange(n_words)
        words = words[(rel % GAP_EVERY != 1) | (rel == n_words - 1)]
    return (words[:, None] * 32 + np.arange(32)).reshape(-1)


def indices_of(blocks, tpb, rng):
    """Token indices that fall into exactly these blocks: every block through a token of its own choice, every 7th through its
    first and its last token too, every 5th twice more; shuffled."""
    b = np.asarray(blocks, dtype=np.int64)
    idx = np.concatenate([b * tpb + b % tpb, b[::7] * tpb, b[::7] * tpb + tpb - 1, b[::5] * tpb + tpb // 2, b[::5] * tpb + tpb // 2])
    return rng.permutation(idx)


def unique_step(name, blocks, tpb, n_blocks, extra=(), refused=False):
    """One query. `extra` are indices outside the pool; with them the call must be refused."""
    rng = np.random.default_rng(_seed(name))
    idx = indices_of(blocks, tpb, rng)
    if len(extra):
        idx = rng.permutation(np.concatenate([idx, np.asarray(extra, dtype=np.int64)]))
    want = None
    if not refused:
        want = O.unique_block_ids(idx, tpb)
        assert np.array_equal(want, np.unique(blocks)) and want[-1] < n_blocks
    return dict(name=name, idx=idx, tpb=tpb, n_blocks=n_blocks, want=want)


def unique_range_steps(tpb):
    """A generator (the dense queries are large): every (lo, len) with every filling."""
    for lo in RANGE_LOS:
        for n_words in RANGE_LENS:
            for filling in FILLINGS:
                if filling == "dense_with_gaps" and n_words < 3:
                    continue                              # (no room for a gap between the ends)
                yield unique_step(f"unique_t{tpb}_lo{lo}_len{n_words}_{filling}", range_blocks(lo, n_words, filling), tpb,
                                  (lo + n_words) * 32)


HYGIENE_BLOCKS = 60000


def unique_misc_steps(tpb):
    steps = []
    rng = np.random.default_rng(tpb)
    for n in (1, 255, 256, 257):                          # mark_blocks_kernel's last workgroup
        idx = rng.integers(0, 5000 * tpb, size=n)
        steps.append(dict(name=f"unique_t{tpb}_n{n}", idx=idx, tpb=tpb, n_blocks=5000, want=O.unique_block_ids(idx, tpb)))
    idx = rng.choice(np.array([7, 40, 4999]), size=100000) * tpb + rng.integers(0, tpb, size=100000)
    steps.append(dict(name=f"unique_t{tpb}_100000_in_3_blocks", idx=idx, tpb=tpb, n_blocks=5000, want=np.array([7, 40, 4999])))
    for nb in (64, 65, 95):                               # n_blocks % 32 in {0, 1, 31}: the last block, and the first index past it
        name = f"unique_t{tpb}_nblocks{nb}"
        steps.append(unique_step(name + "_last_block", [0, nb // 2, nb - 1], tpb, nb))
        steps.append(unique_step(name + "_one_past_alone", [], tpb, nb, extra=[nb * tpb], refused=True))
        steps.append(unique_step(name + "_one_past_among_valid", [0, nb - 1], tpb, nb, extra=[nb * tpb], refused=True))
        steps.append(unique_step(name + "_after_the_refusal", [1, nb - 2], tpb, nb))
    # hygiene: what a refused call marked must be gone, whether or not the next query's word range covers it
    nb, name = HYGIENE_BLOCKS, f"unique_t{tpb}_hygiene"
    steps.append(unique_step(name + "_refused_3_40000", [3, 40000], tpb, nb, extra=[nb * tpb, -1], refused=True))
    steps.append(unique_step(name + "_covering_1_50000", [1, 50000], tpb, nb))
    steps.append(unique_step(name + "_refused_40000", [40000], tpb, nb, extra=[nb * tpb + 5], refused=True))
    steps.append(unique_step(name + "_not_covering_1_3", [1, 3], tpb, nb))
    steps.append(unique_step(name + "_covering_2_50000", [2, 50000], tpb, nb))
    return steps


def unique_growth_steps(tpb=16):
    """One context from its first query on: a bitmap of exactly MIN_BITMAP_WORDS words, one word more, 2^17 words, and a small
    pool again. Blocks on both sides of word 4095|4096 where the pool has them; block 131071 (bit 31 of word 4095), set and swept
    before the growth, is not in the first answer after it."""
    edge = MIN_BITMAP_WORDS * 32                          # first block of word 4096
    name = f"unique_t{tpb}_growth"
    return [unique_step(name + "_131072", [0, edge - 32, edge - 1], tpb, edge),
            unique_step(name + "_131073_without_131071", [5, edge], tpb, edge + 1),
            unique_step(name + "_131073", [edge - 1, edge], tpb, edge + 1),
            unique_step(name + "_4194304", [0, edge - 1, edge, edge + 31, (1 << 22) - 1], tpb, 1 << 22),
            unique_step(name + "_100", [0, 50, 99], tpb, 100)]


def run_unique(uniq, steps, refused, label):
    """uniq(idx, tpb, n_blocks) -> the sorted block ids, or raises one of `refused`. The steps run in order in one context:
    a step's answer shows what the steps before it left behind."""
    for s in steps:
        name = s["name"]
        if s["want"] is None:
            try:
                got = uniq(s["idx"], s["tpb"], s["n_blocks"])
            except refused:
                continue
            raise AssertionError(f"{label} {name}: not refused, answered {len(got)} blocks")
        got, want = np.asarray(uniq(s["idx"], s["tpb"], s["n_blocks"]), dtype=np.int64), np.asarray(s["want"], dtype=np.int64)
        n = min(len(got), len(want))
        bad = np.flatnonzero(got[:n] != want[:n])
        if bad.size or len(got) != len(want):
            i = int(bad[0]) if bad.size else n
            g = int(got[i]) if i < len(got) else "nothing"
            w = int(want[i]) if i < len(want) else "nothing"
            raise AssertionError(f"{label} {name}: element {i}: got {g}, want {w} (got {len(got)} blocks, want {len(want)})")


def touched_words(step):
    """(first word, number of words, blocks per touched word) of a query, from its indices."""
    blocks = np.unique(step["idx"] // step["tpb"])
    words, counts = np.unique(blocks >> 5, return_counts=True)
    return int(words[0]), int(words[-1] - words[0] + 1), dict(zip(words.tolist(), counts.tolist()))


def check_unique_cap(raw, label):
    """raw(idx, tpb, n_blocks, host, cap) -> the C function's return value; `host` is an int64 array that the call may fill.
    cap = count - 1: the count comes back and the array is untouched; the next query is exact; cap = count fills exactly."""
    blocks, tpb, nb = np.array([2, 9, 700, 4000, 4001]), 16, 5000
    idx = indices_of(blocks, tpb, np.random.default_rng(5))
    host = np.full(len(blocks) + GUARD, SENTINEL, dtype=np.int64)
    got = raw(idx, tpb, nb, host, len(blocks) - 1)
    assert got == len(blocks), f"{label} cap = count - 1: returned {got}, want {len(blocks)}"
    bad = np.flatnonzero(host != SENTINEL)
    assert bad.size == 0, f"{label} cap = count - 1: host element {int(bad[0])} was written: {int(host[bad[0]])}"
    other = np.array([3, 9, 4999])
    got = raw(indices_of(other, tpb, np.random.default_rng(6)), tpb, nb, host, len(other))
    assert got == len(other), f"{label} next query: returned {got}, want {len(other)}"
    want = np.concatenate([other, np.full(len(host) - len(other), SENTINEL)])
    bad = np.flatnonzero(host != want)
    assert bad.size == 0, f"{label} next query: host element {int(bad[0])}: got {int(host[bad[0]])}, want {int(want[bad[0]])}"
    host[:] = SENTINEL
    got = raw(idx, tpb, nb, host, len(blocks))
    want = np.concatenate([blocks, np.full(GUARD, SENTINEL)])
    bad = np.flatnonzero(host != want)
    assert got == len(blocks) and bad.size == 0, \
        f"{label} cap = count: returned {got}, host element {int(bad[0]) if bad.size else None} differs"
