"""Seeded inputs for the SGLang token-index glue (shared by the CPU oracle tests and the GPU parity tests)."""
from __future__ import annotations

import numpy as np


def extend_case(seed: int, bs: int, tpb: int, max_prefix: int = None, max_extend: int = None, n_blocks: int = 1 << 20,
                aligned_prefix: bool = False, zero_extend_every: int = 0, id_base: int = 0, prefix_lens=None, extend_lens=None):
    """A consistent alloc_extend input: each request owns distinct blocks for its prefix; last_loc is the slot of
    its last prefix token (-1 when the prefix is empty, as SGLang passes it). `id_base` is added to every drawn block id
    (token indices of 2^31, 2^32 and beyond; the default leaves the cases as they always were). `prefix_lens` and
    `extend_lens` (both or neither, bs entries each) take the place of the drawn lengths: only the block ids are drawn then."""
    rng = np.random.default_rng(seed)
    drawn = max_prefix is not None and max_extend is not None and prefix_lens is None and extend_lens is None
    given = max_prefix is None and max_extend is None and prefix_lens is not None and extend_lens is not None
    assert drawn or given, "give either max_prefix and max_extend or prefix_lens and extend_lens"
    if drawn:
        pre = rng.integers(0, max_prefix + 1, size=bs)
        if aligned_prefix:
            pre = pre // tpb * tpb
        ext = rng.integers(1, max_extend + 1, size=bs)
        if zero_extend_every:
            ext[::zero_extend_every] = 0
    else:
        pre, ext = np.array(prefix_lens, dtype=np.int64), np.array(extend_lens, dtype=np.int64)
        assert pre.shape == ext.shape == (bs,) and (pre >= 0).all() and (ext >= 0).all()
    seq = pre + ext
    pre_blocks = (pre + tpb - 1) // tpb
    new_blocks = (seq + tpb - 1) // tpb - pre_blocks
    ids = rng.permutation(n_blocks)[: int(pre_blocks.sum() + new_blocks.sum())].astype(np.int64) + np.int64(id_base)
    owned, k = [], 0
    for n in pre_blocks:
        owned.append(ids[k:k + n])
        k += n
    free_pages = ids[k:]
    last_loc = np.array([(owned[i][-1] * tpb + (pre[i] - 1) % tpb) if pre[i] else -1 for i in range(bs)], dtype=np.int64)
    return dict(prefix_lens=pre.astype(np.int64), seq_lens=seq.astype(np.int64), last_loc=last_loc,
                free_pages=free_pages, tpb=tpb, owned=owned, extend_num_tokens=int(ext.sum()))


def decode_case(seed: int, bs: int, tpb: int, max_len: int = None, n_blocks: int = 1 << 20, force_boundary_every: int = 0,
                id_base: int = 0, seq_lens=None):
    """`seq_lens` (bs entries, each >= 1) takes the place of the drawn lengths: only the block ids are drawn then."""
    rng = np.random.default_rng(seed)
    assert (max_len is None) != (seq_lens is None), "give either max_len or seq_lens"
    if seq_lens is None:
        seq = rng.integers(1, max_len + 1, size=bs)
        if force_boundary_every:
            seq[::force_boundary_every] = (seq[::force_boundary_every] // tpb) * tpb + 1
    else:
        seq = np.array(seq_lens, dtype=np.int64)
        assert seq.shape == (bs,) and (seq >= 1).all()
    pre = seq - 1
    pre_blocks = (pre + tpb - 1) // tpb
    need = (seq + tpb - 1) // tpb - pre_blocks
    ids = rng.permutation(n_blocks)[: int(pre_blocks.sum() + need.sum())].astype(np.int64) + np.int64(id_base)
    owned, k = [], 0
    for n in pre_blocks:
        owned.append(ids[k:k + n])
        k += n
    free_pages = ids[k:]
    last_loc = np.array([(owned[i][-1] * tpb + (pre[i] - 1) % tpb) if pre[i] else -1 for i in range(bs)], dtype=np.int64)
    return dict(seq_lens=seq.astype(np.int64), last_loc=last_loc, free_pages=free_pages, tpb=tpb, owned=owned)


def check_extend_invariants(case, out):
    """Layout-independent properties of a correct alloc_extend result."""
    tpb = case["tpb"]
    pos0 = 0
    used_new = []
    k = 0
    for i, (pre, seq) in enumerate(zip(case["prefix_lens"], case["seq_lens"])):
        pre, seq = int(pre), int(seq)
        n_new = (seq + tpb - 1) // tpb - (pre + tpb - 1) // tpb
        blocks = list(case["owned"][i]) + list(case["free_pages"][k:k + n_new])
        k += n_new
        used_new += blocks[len(case["owned"][i]):]
        for t in range(seq - pre):
            p = pre + t
            assert out[pos0 + t] == blocks[p // tpb] * tpb + p % tpb, (i, t)
        pos0 += seq - pre
    assert pos0 == len(out) and k == len(case["free_pages"])
    assert len(set(used_new)) == len(used_new)


def case_id(c) -> str:
    """pytest id of a case: the cases without an id_base keep the ids they always had."""
    return f"s{c['seed']}_bs{c['bs']}_t{c['tpb']}" + (f"_base{c['id_base']}" if c.get("id_base") else "")


def wide_id_bases(tpb: int):
    """Block id bases whose token indices (id * tpb + j) straddle 2^31, straddle 2^32, and lie at 2^40 * tpb."""
    return [(1 << 31) // tpb - 3, (1 << 32) // tpb - 3, 1 << 40]


# Small batches and 48 candidate blocks (the drawn ids are base + part of a permutation of 0..47, the line lies at base + 3);
# the seeds are the first ones for which the new blocks' token indices lie on both sides of the line (and, for extend, the
# prefix blocks' too): test_sglang_glue.py asserts that they do. The point of these cases is the width of the values.
_WIDE_EXTEND_SEEDS = {1: (101, 101, 100), 16: (111, 111, 100), 48: (105, 105, 100)}
_WIDE_DECODE_SEEDS = {1: (202, 202, 200), 16: (200, 200, 200), 48: (200, 200, 200)}
WIDE_EXTEND_CASES = [dict(seed=_WIDE_EXTEND_SEEDS[tpb][i], bs=6, tpb=tpb, max_prefix=2 * tpb, max_extend=2 * tpb + 3, n_blocks=48,
                          id_base=base) for tpb in (1, 16, 48) for i, base in enumerate(wide_id_bases(tpb))]
WIDE_DECODE_CASES = [dict(seed=_WIDE_DECODE_SEEDS[tpb][i], bs=12, tpb=tpb, max_len=2 * tpb + 2, n_blocks=48, force_boundary_every=2,
                          id_base=base) for tpb in (1, 16, 48) for i, base in enumerate(wide_id_bases(tpb))]

EXTEND_CASES = [
    dict(seed=1, bs=1, tpb=16, max_prefix=0, max_extend=40),
    dict(seed=2, bs=7, tpb=16, max_prefix=100, max_extend=100),
    dict(seed=3, bs=64, tpb=16, max_prefix=300, max_extend=50, aligned_prefix=True),
    dict(seed=4, bs=33, tpb=1, max_prefix=20, max_extend=20),
    dict(seed=5, bs=50, tpb=3, max_prefix=40, max_extend=40, zero_extend_every=7),
    dict(seed=6, bs=300, tpb=64, max_prefix=500, max_extend=300),
] + WIDE_EXTEND_CASES
DECODE_CASES = [
    dict(seed=1, bs=1, tpb=16, max_len=100),
    dict(seed=2, bs=257, tpb=16, max_len=1000, force_boundary_every=5),
    dict(seed=3, bs=64, tpb=1, max_len=50),
    dict(seed=4, bs=1000, tpb=3, max_len=200),
] + WIDE_DECODE_CASES
