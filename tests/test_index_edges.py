"""What tests/test_gpu_index_edges.py rests on, without a GPU: the cases of tests/kvc_index_edges.py reach the seams they are
named after (computed from the generated inputs, not from their parameters), the seeded cases of tests/test_gpu_sglang_glue.py
do not (the facts the sweeps were written for), the vectorised reference agrees with the oracle's loops on every case, the sweeps
pass when handed the oracle as the operation, and they fail - naming the first bad element - each of seven wrong operations
that pass every seeded case.

Parity of alloc_extend / alloc_decode with SGLang's own kernels stays unpinned here as in oracle/sglang_glue.py: SGLang is not
available to these tests. Both references restate the same published algorithm, one by parts and last_loc, one by position."""
import numpy as np
import pytest

import kvc_glue_cases as G
import kvc_index_edges as E
import test_gpu_sglang_glue as S
from kvc_index_edges import GUARD, MISSING, SENTINEL, O


def _params(test):
    """The argvalues of a test's (single) parametrize mark."""
    return list(test.pytestmark[0].args[1])


# ------------------------------------------------------------------ the seeded cases, in the sweeps' form
def seeded_expand_cases():
    """tests/test_gpu_sglang_glue.py::test_expand_block_ids as it is today: its ids, and the same moved up by the wide bases."""
    cs = []
    for n, tpb in _params(S.test_expand_block_ids):
        ids = np.random.default_rng(n * 31 + tpb).permutation(1 << 22)[:n].astype(np.int64)
        cs.append(E.make_expand(f"seeded_n{n}_t{tpb}", ids, tpb))
        cs += [E.make_expand(f"seeded_n{n}_t{tpb}_base{base}", ids % (1 << 12) + base, tpb) for base in G.wide_id_bases(tpb)]
    return cs


def seeded_extend_configs():
    """test_alloc_extend_indices and the forty batches of test_alloc_extend_accepts_int32_lengths."""
    return S.EXTEND_GPU_CASES + [dict(seed=seed, bs=1 + seed % 13, tpb=16, max_prefix=50, max_extend=50 + 20 * (seed % 5))
                                 for seed in range(21, 61)]


@pytest.fixture(scope="module")
def seeded_extend():
    return [E.extend_dict("seeded_" + G.case_id(cfg), G.extend_case(**cfg)) for cfg in seeded_extend_configs()]


@pytest.fixture(scope="module")
def seeded_decode():
    return [E.decode_dict("seeded_" + G.case_id(cfg), G.decode_case(**cfg)) for cfg in S.DECODE_GPU_CASES]


def seeded_unique_steps():
    """test_unique_block_ids (both queries of every case) and test_unique_block_ids_rejects_out_of_range_and_recovers, as they
    are today. (test_unique_block_ids_beyond_2_to_32_blocks is refused before a kernel runs.)"""
    for n, tpb, n_blocks in _params(S.test_unique_block_ids):
        rng = np.random.default_rng(n + tpb)
        idx = rng.integers(0, n_blocks * tpb, size=n)
        idx[0], idx[-1] = 0, n_blocks * tpb - 1
        lines = [v for v in ((1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32) if v < n_blocks * tpb]
        idx[1:1 + len(lines)] = lines
        yield dict(name=f"seeded_unique_{n}_{tpb}_{n_blocks}", idx=idx, tpb=tpb, n_blocks=n_blocks, want=O.unique_block_ids(idx, tpb))
        idx2 = rng.integers(0, min(n_blocks, 50) * tpb, size=200)
        yield dict(name=f"seeded_unique_{n}_{tpb}_{n_blocks}_second", idx=idx2, tpb=tpb, n_blocks=n_blocks,
                   want=O.unique_block_ids(idx2, tpb))
    yield dict(name="seeded_refused_5_1600_7", idx=np.array([5, 1600, 7]), tpb=16, n_blocks=100, want=None)
    yield dict(name="seeded_refused_minus_1", idx=np.array([-1]), tpb=16, n_blocks=100, want=None)
    yield dict(name="seeded_recovers", idx=np.array([33, 1, 17, 34]), tpb=16, n_blocks=100, want=np.array([0, 1, 2]))


# ------------------------------------------------------------------ numpy stand-ins: the oracle as the operation
def oracle_expand(case, buf):
    out = O.expand_block_ids(case["ids"], case["tpb"])
    buf[GUARD:GUARD + len(out)] = out
    return buf


def _padded(case):
    return np.concatenate([case["ids"], np.full(len(case["free_pages"]) - len(case["ids"]), MISSING)])


def _store(buf, out, limit):
    """What the kernels' guards amount to: nothing at or past `limit`, nothing computed from an id that was not given."""
    n = min(limit, len(out))
    keep = np.flatnonzero(out[:n] >= 0)
    buf[GUARD + keep] = out[keep]
    return buf


def oracle_extend(case, buf):
    out = O.alloc_extend(case["prefix_lens"], case["seq_lens"], case["last_loc"], _padded(case), case["tpb"])
    return _store(buf, out, case["out_len"])


def oracle_decode(case, buf):
    out = O.alloc_decode(case["seq_lens"], case["last_loc"], _padded(case), case["tpb"])
    return _store(buf, out, len(out))


class OracleUnique:
    """The oracle behind the kernels' interface: refuses an index outside the pool. The three switches are the mutants."""

    def __init__(self, drops_first_word=False, cuts_full_words=None, leaks=False):
        self.drops_first_word, self.cuts_full_words, self.leaks = drops_first_word, cuts_full_words, leaks
        self.left = np.empty(0, dtype=np.int64)              # bits still set in the bitmap when a call begins

    def __call__(self, idx, tpb, n_blocks):
        idx = np.asarray(idx, dtype=np.int64)
        valid = (idx >= 0) & (idx // tpb < n_blocks)
        marked = O.unique_block_ids(idx[valid], tpb)
        out = marked
        if marked.size:                                   # the sweep covers the words this call touched, and clears them
            lo, hi = marked[0] >> 5, marked[-1] >> 5
            inside = (self.left >> 5 >= lo) & (self.left >> 5 <= hi)
            out = np.union1d(marked, self.left[inside])
            self.left = self.left[~inside]
            if self.drops_first_word and lo > 0:
                out = out[out >> 5 != lo]
            if self.cuts_full_words is not None:       # (in words from this one on)
                words, counts = np.unique(out >> 5, return_counts=True)
                full = words[(counts == 32) & (words >= self.cuts_full_words)]
                out = out[~(np.isin(out >> 5, full) & (out & 31 == 31))]
        if not valid.all():
            if self.leaks:
                self.left = np.union1d(self.left, out)
            raise E.Refused(f"{int((~valid).sum())} token indices are outside")
        return out.tolist()


# ------------------------------------------------------------------ the cases are what they say
def test_the_launch_constants_are_the_kernels():
    """The constants of kvc_index_edges.py, read back from the sources they point to, by the text of the lines. A tripwire: a
    failure here says that the kernels' source has changed and that the constants (and with them the seams the cases sit on) want
    rechecking - not that a kernel is wrong."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(__file__), "..", "kvcached_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in ("index_kernels.hip", "kernels.hpp", "gpu_context.cpp")}
    k = text["index_kernels.hip"]
    assert int(re.search(r"kMaxIdsPerLaunch = (\d+);", text["kernels.hpp"]).group(1)) == E.IDS_PER_LAUNCH
    assert int(re.search(r"kExtendTokensPerGroup = (\d+);", k).group(1)) == E.EXTEND_GROUP
    assert f"w0 += {E.SWEEP_CHUNK_WORDS})" in k and f"__launch_bounds__({E.SWEEP_CHUNK_WORDS}) void sweep_blocks_kernel" in k
    assert k.count(f"__launch_bounds__({E.THREADS}) void") == 4 and f"blockIdx.x * {E.THREADS}" in k
    assert "threadIdx.x >> 6" in k and "w = b >> 5" in k and E.LANES == 1 << 6 and E.BLOCKS_PER_WORD == 1 << 5
    assert f"std::max<size_t>(words, {E.MIN_BITMAP_WORDS})" in text["gpu_context.cpp"]
    assert E.SWEEP_CHUNK_BLOCKS == 32768 and E.WAVES == 4 and E.GUARD == 256


def test_expand_cases_are_what_they_say():
    cases = E.expand_cases()
    shapes = {(len(c["ids"]), c["tpb"]) for c in cases}
    assert len(shapes) == len(cases)
    for tpb in E.EXPAND_TPBS:
        assert (1, tpb) in shapes
        reachable = {r for r in E.EXPAND_REMAINDERS if r % np.gcd(tpb, 256) == 0}
        assert {n * t % 256 for n, t in shapes if t == tpb and n > 1} >= reachable, tpb
    assert {1, 3, 5, 255, 257} <= {t for t in E.EXPAND_TPBS if np.gcd(t, 256) == 1}     # these reach 0, 1 and 255
    for tpb in (1, 3):
        assert {n for n, t in shapes if t == tpb} >= set(E.EXPAND_CHUNK_NS)
    assert any(n == 0 for n, _ in shapes)
    assert max(len(c["want"]) for c in cases) <= 300000


def test_extend_cases_are_what_they_say():
    cases = E.extend_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    ext = [c["seq_lens"] - c["prefix_lens"] for c in cases]
    alone = sorted(int(e[0]) for e in ext if len(e) == 1 and int(e[0]) in E.EXTEND_LENS)
    assert sorted(set(alone)) == E.EXTEND_LENS
    # a long request with short and zero-length ones on both sides, and with either of them first
    for n in E.EXTEND_LENS[5:]:
        orders = set()
        for e in ext:
            at = np.flatnonzero(e == n)
            if len(e) > 1 and at.size == 1 and 0 < at[0] < len(e) - 1 and (e == 0).any():
                before, after = e[:at[0]], e[at[0] + 1:]
                if 0 in before and 0 in after and before.max() < 256 and after.max() < 256:
                    orders.add(int(before[0]) < int(after[-1]))
        assert orders == {False, True}, n
    totals = {int(e.sum()) for e in ext if len(e) > 1}
    assert {4096, 4097, 8192, 8193} <= totals
    assert max(int(e.sum()) for e in ext) < 26000
    assert {len(e) for e in ext} >= set(E.EXTEND_BS)
    assert {len(c["free_pages"]) for c in cases} >= set(E.NEW_BLOCK_TOTALS)
    assert any(len(c["ids"]) == 0 and c["out_len"] > 0 for c in cases)
    # the prefix phase against the block, and the three ways an extension can end
    for tpb in E.PHASE_TPBS:
        seen = {}
        for c in (c for c in cases if c["tpb"] == tpb):
            pre, seq = c["prefix_lens"], c["seq_lens"]
            new = -(-seq // tpb) - -(-pre // tpb)
            for p, s, n in zip(pre.tolist(), seq.tolist(), new.tolist()):
                kinds = seen.setdefault(p % tpb, set())
                if s > p and n == 0 and s % tpb:
                    kinds.add("inside")
                if s > p and s % tpb == 0:
                    kinds.add("fills")
                if s > p and n >= 1 and (s - 1) % tpb == 0:
                    kinds.add("one past")
        for phase in {0, 1 % tpb, tpb - 1}:
            room = -phase % tpb
            want = {"fills", "one past"} | ({"inside"} if room >= 2 else set())
            assert seen.get(phase, set()) >= want, (tpb, phase, seen.get(phase))
    # a block on both sides of a group seam: token t = 4096 of a request is not the first of its block
    for tpb in (4096, 5000):
        straddles = [(int(p) + E.EXTEND_GROUP) % tpb for c in cases if c["tpb"] == tpb
                     for p, s in zip(c["prefix_lens"], c["seq_lens"]) if s - p == 8193]
        assert len(straddles) == 3 and sum(x != 0 for x in straddles) >= 2, (tpb, straddles)
    # inconsistent input: the id list short by one and by the last request's share, extend_num_tokens below the sum
    cuts = {len(c["free_pages"]) - len(c["ids"]) for c in cases}
    assert cuts == {0, 1, 256}
    for c in cases:
        missing = c["want"] == SENTINEL
        cut = len(c["free_pages"]) - len(c["ids"])
        if cut:
            pre, seq = int(c["prefix_lens"][-1]), int(c["seq_lens"][-1])
            start = len(missing) - (seq - pre)
            share = -(-seq // 16) - -(-pre // 16)
            assert c["tpb"] == 16 and not missing[:start].any() and missing[-1] and (cut == 1 or cut == share)
            assert int(missing.sum()) == (seq - 1) % 16 + 1 + 16 * (cut - 1)      # the last `cut` blocks of the last request
            assert not missing[start:start + (-pre % 16)].any()                   # what follows last_loc is still written
        elif c["out_len"] < len(c["want"]):
            assert missing[c["out_len"]:].all() and not missing[:c["out_len"]].any()
        else:
            assert not missing.any()
    shorts = sorted(len(c["want"]) - c["out_len"] for c in cases if c["out_len"] < len(c["want"]))
    assert shorts == [1, 4190 - E.EXTEND_GROUP, 100, 4189]
    assert any(c["out_len"] == E.EXTEND_GROUP and (c["seq_lens"] - c["prefix_lens"]).max() > E.EXTEND_GROUP for c in cases)


def _wave_states(seq_lens, tpb):
    """Per workgroup and wave of alloc_decode_kernel: (requests in the wave, requests that open a block)."""
    need = E.opens_block(seq_lens, tpb)
    out = []
    for base in range(0, len(need), E.THREADS):
        out.append([(len(w), int(w.sum())) for w in (need[base + k * E.LANES:base + (k + 1) * E.LANES] for k in range(E.WAVES))])
    return out


def _state(size, count):
    return "empty" if count == 0 else "full" if count == size else "partial"


def _predecessors(cases):
    """{(wave position, state of the FULL-SIZE wave right before it)} over all waves with a block-opening request; position 0
    stands for wave 0 of a later workgroup, whose predecessor is wave 3 of the one before."""
    seen = set()
    for c in cases:
        flat = [w for wg in _wave_states(c["seq_lens"], c["tpb"]) for w in wg]
        for i in range(1, len(flat)):
            if flat[i][1] and flat[i - 1][0] == E.LANES:
                seen.add((i % E.WAVES, _state(*flat[i - 1])))
    return seen


def test_decode_cases_are_what_they_say():
    cases = E.decode_cases()
    by_name = {c["name"]: c for c in cases}
    assert len(by_name) == len(cases)
    for bs in E.DECODE_BS:
        for m, f in E.DECODE_MASKS.items():
            c = by_name[f"decode_bs{bs}_{m}"]
            assert c["tpb"] == 16 and len(c["seq_lens"]) == bs
            assert np.array_equal(E.opens_block(c["seq_lens"], 16), f(np.arange(bs), bs)), c["name"]
            assert len(c["free_pages"]) == int(f(np.arange(bs), bs).sum())
    # every wave position behind an empty, a partly and a wholly block-opening wave
    assert _predecessors(cases) == {(k, s) for k in range(E.WAVES) for s in ("empty", "partial", "full")}
    # whole workgroups without a block-opening request in front of one that has some
    assert any(len(c["seq_lens"]) > 512 and not E.opens_block(c["seq_lens"][:512], 16).any() and len(c["free_pages"]) for c in cases)
    assert {len(c["free_pages"]) for c in cases if c["tpb"] == 1 and len(c["seq_lens"]) > 1000} == set(E.DECODE_STAGED_BS)
    assert any((c["seq_lens"] == 1).all() and (c["last_loc"] == -1).all() and c["tpb"] == 16 for c in cases)
    assert any((c["seq_lens"] == 1).any() and c["tpb"] == 16 and len(c["seq_lens"]) > 256 for c in cases)
    short = [c for c in cases if len(c["ids"]) < len(c["free_pages"])]
    assert len(short) == 1 and int((short[0]["want"] == SENTINEL).sum()) == 1
    last = int(np.flatnonzero(E.opens_block(short[0]["seq_lens"], 16))[-1])
    assert short[0]["want"][last] == SENTINEL


@pytest.mark.parametrize("tpb", E.UNIQUE_TPBS)
def test_unique_cases_are_what_they_say(tpb):
    seen = {f: set() for f in E.FILLINGS}
    for s in E.unique_range_steps(tpb):
        filling = next(f for f in sorted(E.FILLINGS, key=len, reverse=True) if s["name"].endswith("_" + f))
        lo, n_words, per_word = E.touched_words(s)
        seen[filling].add((lo, n_words))
        blocks = set(np.unique(s["idx"] // tpb).tolist())
        assert s["n_blocks"] == (lo + n_words) * 32 and int(s["idx"].max()) < s["n_blocks"] * tpb
        if filling == "ends":
            assert len(blocks) == 2 and len(per_word) == min(n_words, 2)
        if filling == "seams":
            for seam in range(E.LANES, n_words, E.LANES):     # the chunk seams are wave seams too
                assert {(lo + w) * 32 + b for w in (seam - 1, seam) for b in (0, 31)} <= blocks
            assert all(v == 2 for v in per_word.values())
        if filling == "dense":
            assert len(per_word) == n_words and all(v == 32 for v in per_word.values()) and s["n_blocks"] - 1 in blocks
            tokens = s["idx"] % tpb
            assert tpb == 1 or ((tokens == 0).any() and (tokens == tpb - 1).any())
            assert len(s["idx"]) > len(blocks)                # duplicates
        if filling == "dense_with_gaps":
            assert all(v == 32 for v in per_word.values()) and len(per_word) < n_words
            assert lo in per_word and lo + n_words - 1 in per_word and lo + 1 not in per_word
    pairs = {(lo, n) for lo in E.RANGE_LOS for n in E.RANGE_LENS}
    assert seen["ends"] == seen["seams"] == seen["dense"] == pairs
    assert seen["dense_with_gaps"] == {p for p in pairs if p[1] >= 3}
    assert max(n for _, n in pairs) * 32 == 65568
    # the other queries
    misc = {s["name"]: s for s in E.unique_misc_steps(tpb)}
    assert {len(s["idx"]) for s in misc.values()} >= {1, 255, 256, 257, 100000}
    assert [len(s["want"]) for s in misc.values() if len(s["idx"]) == 100000] == [3]
    for nb in (64, 65, 95):
        name = f"unique_t{tpb}_nblocks{nb}"
        assert nb - 1 in misc[name + "_last_block"]["want"] and misc[name + "_one_past_alone"]["idx"].tolist() == [nb * tpb]
        refused = misc[name + "_one_past_among_valid"]
        assert refused["want"] is None and nb * tpb in refused["idx"] and int(refused["idx"].max()) == nb * tpb
    assert {nb % 32 for nb in (64, 65, 95)} == {0, 1, 31}
    # hygiene: the refused calls' valid blocks are in no later answer; the later queries' word ranges do / do not cover them
    h = [s for s in E.unique_misc_steps(tpb) if "hygiene" in s["name"]]
    assert [s["want"] is None for s in h] == [True, False, True, False, False]

    def valid_blocks(s):
        return set(np.unique(s["idx"][(s["idx"] >= 0) & (s["idx"] < s["n_blocks"] * tpb)] // tpb).tolist())

    def covers(s, blocks):
        lo, n_words, _ = E.touched_words(s)
        return all(lo <= b >> 5 < lo + n_words for b in blocks)

    assert valid_blocks(h[0]) == {3, 40000} and h[1]["want"].tolist() == [1, 50000] and covers(h[1], {3, 40000})
    assert valid_blocks(h[2]) == {40000} and h[3]["want"].tolist() == [1, 3] and not covers(h[3], {40000})
    assert h[4]["want"].tolist() == [2, 50000] and covers(h[4], {40000})
    g = E.unique_growth_steps()
    assert [s["n_blocks"] for s in g] == [131072, 131073, 131073, 1 << 22, 100]
    assert [-(-s["n_blocks"] // 32) for s in g[:2]] == [E.MIN_BITMAP_WORDS, E.MIN_BITMAP_WORDS + 1]
    assert 131071 in g[0]["want"] and 131071 not in g[1]["want"] and 131072 in g[1]["want"]
    for s in g[2:4]:
        assert {4095, 4096} <= set(np.unique(s["want"] >> 5).tolist())


# ------------------------------------------------------------------ the facts the sweeps were written for
def test_the_seeded_cases_miss_these_seams(seeded_extend, seeded_decode):
    """Computed from the seeded cases of tests/test_gpu_sglang_glue.py as they are today. (Its end-to-end loop draws prompts
    below 400 tokens and decodes from request 0 on.)"""
    longest = max(int((c["seq_lens"] - c["prefix_lens"]).max()) for c in seeded_extend)
    assert longest == 2572 < E.EXTEND_GROUP                # no token past a request's first group was ever written
    seed11 = next(c for c in seeded_extend if c["name"] == "seeded_s11_bs1_t16")
    assert (seed11["seq_lens"] - seed11["prefix_lens"]).tolist() == [2572]
    # new-block counts: nothing next to the 1024 ids of the kernarg segment, and no batch without a new block
    for cases, below, above in ((seeded_extend, 691, 1447), (seeded_decode, 325, 1877)):
        counts = sorted(len(c["free_pages"]) for c in cases)
        assert not [n for n in counts if below < n < above] and below in counts and above in counts
    assert 0 not in [len(c["free_pages"]) for c in seeded_extend]
    assert [c["name"] for c in seeded_decode if not len(c["free_pages"])] == ["seeded_s1_bs1_t16"]     # one request
    full_words = set()
    for s in seeded_unique_steps():
        if s["want"] is not None:
            lo, n_words, per_word = E.touched_words(s)
            assert lo == 0, s["name"]                      # the sweep has only ever started at word 0
            full_words |= {(w, n_words, s["name"].endswith("_second")) for w, v in per_word.items() if v == 32}
    # the only word that has ever been full is word 0, in the follow-up queries (200 indices into blocks 0 .. 49)
    assert full_words == {(0, 2, True)}
    # decode: no full-size wave without a block-opening request, so none in front of a wave that has some
    for c in seeded_decode:
        assert not [w for wg in _wave_states(c["seq_lens"], c["tpb"]) for w in wg if w == (E.LANES, 0)], c["name"]
    assert "empty" not in {s for _, s in _predecessors(seeded_decode)}


# ------------------------------------------------------------------ the second reference, pinned
def test_the_vectorised_reference_is_the_oracle(seeded_extend, seeded_decode):
    """ref_extend (by position, from the blocks a request owns) against O.alloc_extend / O.alloc_decode (by parts, from
    last_loc) on every consistent sweep case and every seeded case; and against check_extend_invariants, which it restates."""
    for c in E.extend_cases() + seeded_extend:
        if len(c["ids"]) == len(c["free_pages"]) and c["out_len"] == len(c["want"]):
            out = O.alloc_extend(c["prefix_lens"], c["seq_lens"], c["last_loc"], c["free_pages"], c["tpb"])
            assert np.array_equal(out, c["want"]) and out.dtype == c["want"].dtype == np.int64, c["name"]
            assert O.get_num_new_pages(c["seq_lens"], c["tpb"], c["prefix_lens"]) == len(c["free_pages"])
    for c in E.extend_cases():                             # (`reference` is the answer to the consistent input of every case)
        G.check_extend_invariants(c, c["reference"])
    for c in E.decode_cases() + seeded_decode:
        if len(c["ids"]) == len(c["free_pages"]):
            assert np.array_equal(O.alloc_decode(c["seq_lens"], c["last_loc"], c["free_pages"], c["tpb"]), c["want"]), c["name"]


# ------------------------------------------------------------------ rehearsal
def test_the_sweeps_pass_the_oracle():
    E.sweep_expand(oracle_expand, "oracle")
    E.sweep_extend(oracle_extend, "oracle")
    E.sweep_decode(oracle_decode, "oracle")
    for mode in ("payload", "written"):
        E.sweep_extend(oracle_extend, "oracle", mode)


@pytest.mark.parametrize("tpb", E.UNIQUE_TPBS)
def test_the_unique_sweeps_pass_the_oracle(tpb):
    uniq = OracleUnique()
    E.run_unique(uniq, E.unique_growth_steps(tpb), E.Refused, "oracle")
    E.run_unique(uniq, E.unique_range_steps(tpb), E.Refused, "oracle")
    E.run_unique(uniq, E.unique_misc_steps(tpb), E.Refused, "oracle")
    assert uniq.left.size == 0

    def raw(idx, tpb, n_blocks, host, cap):
        got = uniq(idx, tpb, n_blocks)
        if len(got) <= cap:
            host[:len(got)] = got
        return len(got)

    E.check_unique_cap(raw, "oracle")


# ------------------------------------------------------------------ mutation
def expand_one_too_many(case, buf):
    oracle_expand(case, buf)
    if len(case["ids"]):
        buf[GUARD + len(case["want"])] = 0
    return buf


def extend_first_group_only(case, buf):
    """Every workgroup with blockIdx.y >= 1 returns."""
    oracle_extend(case, buf)
    ext = case["seq_lens"] - case["prefix_lens"]
    t = np.arange(int(ext.sum())) - np.repeat(np.cumsum(ext) - ext, ext)
    buf[GUARD + np.flatnonzero(t >= E.EXTEND_GROUP)] = SENTINEL
    return buf


def extend_writes_at_out_len(case, buf):
    """`<=` for `<` in the guard of the store."""
    full = dict(case, out_len=len(case["want"]))
    out = oracle_extend(full, E.guarded(len(case["want"])))
    oracle_extend(case, buf)
    if case["out_len"] < len(case["want"]):
        buf[GUARD + case["out_len"]] = out[GUARD + case["out_len"]]
    return buf


def decode_empty_wave_repeats(case, buf):
    """A wave with no block-opening request leaves the previous wave's count in wave_cnt[]."""
    tpb, ids = case["tpb"], case["ids"]
    need = E.opens_block(case["seq_lens"], tpb)
    before = 0
    for base in range(0, len(need), E.THREADS):
        counts = [int(need[base + k * E.LANES:base + (k + 1) * E.LANES].sum()) for k in range(E.WAVES)]
        seen = [c if c or k == 0 else counts[k - 1] for k, c in enumerate(counts)]
        for r in range(base, min(base + E.THREADS, len(need))):
            wave, lane0 = (r - base) // E.LANES, base + (r - base) // E.LANES * E.LANES
            if need[r]:
                k = before + sum(seen[:wave]) + int(need[lane0:r].sum())
                if k < len(ids):
                    buf[GUARD + r] = ids[k] * tpb
            else:
                buf[GUARD + r] = case["last_loc"][r] + 1
        before += sum(counts)
    return buf


def _fails(run, *first_bad):
    with pytest.raises(AssertionError) as e:
        run()
    assert all(part in str(e.value) for part in first_bad), str(e.value)


def test_the_sweeps_catch_a_wrong_expand():
    E.sweep_expand(expand_one_too_many, "seeded", "payload", seeded_expand_cases())
    _fails(lambda: E.sweep_expand(expand_one_too_many, "mutant"), "mutant expand_n1_t1:", "guard word 0 behind the payload",
           "got 0, want the sentinel")


def test_the_sweeps_catch_a_wrong_extend(seeded_extend):
    E.sweep_extend(extend_first_group_only, "seeded", "payload", seeded_extend)
    _fails(lambda: E.sweep_extend(extend_first_group_only, "mutant"), "mutant alone_ext4097:", "element 4096 (request 0 token 4096)",
           "got the sentinel, want ")
    _fails(lambda: E.sweep_extend(extend_first_group_only, "mutant", "written"), "mutant alone_ext4097:", "element 4096 ")
    E.sweep_extend(extend_writes_at_out_len, "seeded", "payload", seeded_extend)
    _fails(lambda: E.sweep_extend(extend_writes_at_out_len, "mutant"), "mutant out_len_4190_minus_1:",
           "element 4189 (request 4 token 4096)", "want the sentinel")


def test_the_sweeps_catch_a_wrong_decode(seeded_decode):
    E.sweep_decode(decode_empty_wave_repeats, "seeded", "payload", seeded_decode)
    # empty waves behind the last block-opening one, and dense masks, pass it too: only an empty wave between two block-opening ones shows it
    by = {c["name"]: c for c in E.decode_cases()}
    E.sweep_decode(decode_empty_wave_repeats, "mutant", cases=[by["decode_bs255_wave0"], by["decode_bs513_alternating"]])
    # wave 1 is empty and repeats wave 0's count of 64: request 128, the first of wave 2, takes id 128 where it must take id 64
    _fails(lambda: E.sweep_decode(decode_empty_wave_repeats, "mutant"), "mutant decode_bs129_waves0and2:", "element 128 (request 128)")


@pytest.mark.parametrize("mutant,first_bad", [
    (dict(drops_first_word=True), ("_lo1_len1_ends:", "element 0: got nothing, want 37 (got 0 blocks, want 2)")),
    (dict(cuts_full_words=1), ("_lo0_len2_dense:", "element 63: got nothing, want 63 (got 63 blocks, want 64)")),
])
def test_the_sweeps_catch_a_wrong_unique_sweep(mutant, first_bad):
    E.run_unique(OracleUnique(**mutant), seeded_unique_steps(), E.Refused, "seeded")
    _fails(lambda: E.run_unique(OracleUnique(**mutant), E.unique_range_steps(16), E.Refused, "mutant"), "mutant unique_t16", *first_bad)


def test_a_cut_full_word_0_is_caught_by_the_seeded_cases_too():
    """A sweep that emits only the first 31 blocks of EVERY full word fails the seeded follow-up queries, which fill word 0 (and
    nothing else); the mutant above cuts the full words behind word 0, which only the dense sweeps have."""
    _fails(lambda: E.run_unique(OracleUnique(cuts_full_words=0), seeded_unique_steps(), E.Refused, "seeded"),
           "seeded_unique_3000_16_5000_second:", "element 31: got 32, want 31")
    _fails(lambda: E.run_unique(OracleUnique(cuts_full_words=0), E.unique_range_steps(16), E.Refused, "mutant"),
           "_lo0_len1_dense:", "element 31: got nothing, want 31 (got 31 blocks, want 32)")


def test_the_sweeps_catch_a_leaked_bit():
    E.run_unique(OracleUnique(leaks=True), seeded_unique_steps(), E.Refused, "seeded")     # [0, 1, 2] has block 0 anyway
    _fails(lambda: E.run_unique(OracleUnique(leaks=True), E.unique_misc_steps(16), E.Refused, "mutant"),
           "mutant unique_t16_nblocks64_after_the_refusal:", "element 0: got 0, want 1")
    hygiene = [s for s in E.unique_misc_steps(16) if "hygiene" in s["name"]]
    _fails(lambda: E.run_unique(OracleUnique(leaks=True), hygiene[:2], E.Refused, "mutant"),
           "hygiene_covering_1_50000:", "element 1: got 3, want 50000 (got 4 blocks, want 2)")
    _fails(lambda: E.run_unique(OracleUnique(leaks=True), hygiene[2:], E.Refused, "mutant"),
           "hygiene_covering_2_50000:", "element 1: got 40000, want 50000 (got 3 blocks, want 2)")
