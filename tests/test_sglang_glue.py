"""CPU tests of the SGLang token-index glue: the numpy oracle against the reference's own torch expressions
(kvcached/integration/sglang/patches.py:192-196, :283) and against the layout-independent invariants of
alloc_extend / alloc_decode (SGLang's kernels themselves are not in this image: parity unpinned for those two,
see oracle/sglang_glue.py), plus the host helper num_new_pages."""
import os
import sys

import numpy as np
import pytest
import torch

import kvc_glue_cases as G

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
import sglang_glue as O  # noqa: E402


@pytest.mark.parametrize("n,tpb", [(0, 16), (1, 1), (5, 16), (1025, 64), (17, 3)])
def test_expand_matches_the_reference_expression(n, tpb):
    ids = np.random.default_rng(n + tpb).permutation(1 << 20)[:n].astype(np.int64)
    page_ids = torch.tensor(ids, dtype=torch.int64)
    want = (page_ids[:, None] * tpb + torch.arange(tpb)).reshape(-1)       # the reference's expression
    assert np.array_equal(O.expand_block_ids(ids, tpb), want.numpy())
    # the same ids moved up: token indices that straddle 2^31 and 2^32, and block ids of 2^40; compared as int64
    for base in G.wide_id_bases(tpb):
        wide = ids % (1 << 12) + base
        page_ids = torch.tensor(wide, dtype=torch.int64)
        want = (page_ids[:, None] * tpb + torch.arange(tpb)).reshape(-1)
        got = O.expand_block_ids(wide, tpb)
        assert got.dtype == np.int64 and want.dtype == torch.int64 and np.array_equal(got, want.numpy())
        if n:
            assert int(got.max()) == (int(wide.max()) + 1) * tpb - 1      # in Python ints: nothing wrapped on either side


@pytest.mark.parametrize("tpb", [1, 16, 48])
def test_unique_matches_the_reference_expression(tpb):
    idx = np.random.default_rng(tpb).integers(0, 5000 * tpb, size=3000)
    want = torch.unique(torch.tensor(idx) // tpb)
    assert np.array_equal(O.unique_block_ids(idx, tpb), want.numpy())


@pytest.mark.parametrize("cfg", G.EXTEND_CASES, ids=G.case_id)
def test_oracle_alloc_extend_invariants(cfg):
    case = G.extend_case(**cfg)
    out = O.alloc_extend(case["prefix_lens"], case["seq_lens"], case["last_loc"], case["free_pages"], case["tpb"])
    assert (out >= 0).all()
    G.check_extend_invariants(case, out)
    assert O.get_num_new_pages(case["seq_lens"], case["tpb"], case["prefix_lens"]) == len(case["free_pages"])


@pytest.mark.parametrize("cfg", G.DECODE_CASES, ids=G.case_id)
def test_oracle_alloc_decode_is_a_one_token_extend(cfg):
    case = G.decode_case(**cfg)
    out = O.alloc_decode(case["seq_lens"], case["last_loc"], case["free_pages"], case["tpb"])
    ext = O.alloc_extend(case["seq_lens"] - 1, case["seq_lens"], case["last_loc"], case["free_pages"], case["tpb"])
    assert np.array_equal(out, ext)
    assert O.get_num_new_pages(case["seq_lens"], case["tpb"], decode=True) == len(case["free_pages"])


def test_id_base_zero_leaves_the_cases_as_they_were():
    for cfg in (c for c in G.EXTEND_CASES if "id_base" not in c):
        a, b = G.extend_case(**cfg), G.extend_case(**cfg, id_base=0)
        assert a.keys() == b.keys() and "id_base" not in cfg
        for k in a:
            if k == "owned":
                assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a[k], b[k]))
            elif isinstance(a[k], np.ndarray):
                assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype
            else:
                assert a[k] == b[k]
    # the same draw with a base is the same case, every block id moved by the base
    cfg = G.EXTEND_CASES[1]
    a, b = G.extend_case(**cfg), G.extend_case(**cfg, id_base=1 << 40)
    assert np.array_equal(a["free_pages"] + (1 << 40), b["free_pages"]) and np.array_equal(a["seq_lens"], b["seq_lens"])
    assert np.array_equal(np.where(a["last_loc"] < 0, -1, a["last_loc"] + (cfg["tpb"] << 40)), b["last_loc"])
    for cfg in (c for c in G.DECODE_CASES if "id_base" not in c):
        a, b = G.decode_case(**cfg), G.decode_case(**cfg, id_base=0)
        assert all(np.array_equal(a[k], b[k]) for k in ("seq_lens", "last_loc", "free_pages")) and a["tpb"] == b["tpb"]
        assert all(np.array_equal(x, y) for x, y in zip(a["owned"], b["owned"]))


def test_wide_cases_lie_on_both_sides_of_their_line():
    """The cases with an id_base are in the lists, and their token indices do what they are there for: straddle 2^31 or 2^32
    (bases next to a line) or exceed 2^40."""
    assert all(c in G.EXTEND_CASES for c in G.WIDE_EXTEND_CASES) and all(c in G.DECODE_CASES for c in G.WIDE_DECODE_CASES)
    assert len(G.WIDE_EXTEND_CASES) == len(G.WIDE_DECODE_CASES) == 9

    def check(ids, tpb, base):
        lo, hi = ids * tpb, ids * tpb + tpb - 1
        assert len(ids) >= 3 and ids.dtype == np.int64
        if base == 1 << 40:
            assert (lo >= (1 << 40)).all()
        else:
            line = min((1 << 31, 1 << 32), key=lambda x: abs(x - base * tpb))
            assert (lo < line).any() and (hi >= line).any(), (tpb, base)

    for cfg in G.WIDE_EXTEND_CASES:
        case = G.extend_case(**cfg)
        check(case["free_pages"], cfg["tpb"], cfg["id_base"])
        check(np.concatenate(case["owned"]), cfg["tpb"], cfg["id_base"])
    for cfg in G.WIDE_DECODE_CASES:
        check(G.decode_case(**cfg)["free_pages"], cfg["tpb"], cfg["id_base"])


def test_num_new_pages_host_helper():
    from kvcached_amd.integration.sglang.allocators import num_new_pages
    for cfg in G.EXTEND_CASES:
        c = G.extend_case(**cfg)
        assert num_new_pages(torch.tensor(c["seq_lens"]), c["tpb"], torch.tensor(c["prefix_lens"])) == len(c["free_pages"])
    for cfg in G.DECODE_CASES:
        c = G.decode_case(**cfg)
        assert num_new_pages(torch.tensor(c["seq_lens"]), c["tpb"], decode=True) == len(c["free_pages"])


def test_index_ops_need_a_gpu_device():
    """No CPU fallback: on the cpu device the C ABI refuses instead of computing something."""
    from kvcached_amd import capi, vmm_ops
    vmm_ops.init_kvcached("cpu", 2 << 20, False)
    try:
        buf = (capi._i64 * 16)()
        with pytest.raises(capi.KvcError) as e:
            capi.expand_block_ids([1, 2], 4, capi.ctypes.addressof(buf))
        assert e.value.code == capi.E_NO_GPU if hasattr(capi, "E_NO_GPU") else e.value.code < 0
        with pytest.raises(capi.KvcError):
            capi.unique_block_ids(capi.ctypes.addressof(buf), 4, 4, 16)
    finally:
        vmm_ops.shutdown_kvcached()
