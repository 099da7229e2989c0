"""The sparse reference model of the far-offset GPU tests (kvc_sparse_model.py), pinned on the CPU: on small dense regions,
where every page is present, its compact() equals the oracle's memcpy loop (okvc_compact_blocks) byte for byte and its
image() / scatter() equal the host-image expression the offload tests use - at block sizes that straddle the model's pages."""
import ctypes

import numpy as np
import pytest

import kvc_testlib as T
from kvc_sparse_model import SparseRegions, UnbackedError
from test_gpu_host_offload import _expected_image

BLOCK_BYTES = [16, 1040, 18432, 32768]


def _page_sizes(bb):
    return [2 * bb, 3 * bb // 2, 5 * bb + 8]      # blocks never / every other one / mostly straddle a page edge


def _dense(rng, n_regions, n_blocks, bb, page_bytes):
    n_pages = -(-n_blocks * bb // page_bytes)
    hosts = [rng.integers(0, 256, size=n_pages * page_bytes, dtype=np.uint8) for _ in range(n_regions)]
    model = SparseRegions(n_regions, page_bytes)
    for r, h in enumerate(hosts):
        for p in range(n_pages):
            model.load_page(r, p, h[p * page_bytes:(p + 1) * page_bytes])
    return hosts, model


def _flat(model, r):
    return np.concatenate([model.pages[r][p] for p in sorted(model.pages[r])])


@pytest.mark.parametrize("bb", BLOCK_BYTES)
def test_compact_equals_the_oracle(oracle_lib, bb):
    for k, page_bytes in enumerate(_page_sizes(bb)):
        rng = np.random.default_rng(bb + k)
        n_blocks, n_regions, n_moves = 41, 3, 13
        hosts, model = _dense(rng, n_regions, n_blocks, bb, page_bytes)
        ids = rng.choice(n_blocks, size=2 * n_moves, replace=False)
        src, dst = [int(x) for x in ids[:n_moves]], [int(x) for x in ids[n_moves:]]
        bases = (ctypes.c_void_p * n_regions)(*[h.ctypes.data for h in hosts])
        oracle_lib.okvc_compact_blocks(bases, n_regions, T._arr(src), T._arr(dst), n_moves, bb)
        model.compact(src, dst, bb)
        for r in range(n_regions):
            assert np.array_equal(_flat(model, r), hosts[r]), (bb, page_bytes, r)


@pytest.mark.parametrize("bb", BLOCK_BYTES)
def test_image_and_scatter_equal_the_offload_expression(bb):
    for k, page_bytes in enumerate(_page_sizes(bb)):
        rng = np.random.default_rng(100 + bb + k)
        n_blocks, n_regions, n = 37, 3, 11
        hosts, model = _dense(rng, n_regions, n_blocks, bb, page_bytes)
        ids = [int(x) for x in rng.choice(n_blocks, size=n, replace=False)]
        assert np.array_equal(model.image(ids, bb), _expected_image(hosts, ids, bb)), (bb, page_bytes)
        # scatter: exactly what test_kernels_copy_blocks_byte_for_byte expects of copy_blocks_from_host
        img = rng.integers(0, 256, size=n * n_regions * bb, dtype=np.uint8)
        model.scatter(img, ids, bb)
        want = img.reshape(n, n_regions, bb)
        for r in range(n_regions):
            exp = hosts[r].copy()
            exp[:n_blocks * bb].reshape(-1, bb)[ids] = want[:, r, :]
            assert np.array_equal(_flat(model, r), exp), (bb, page_bytes, r)
        assert np.array_equal(model.image(ids, bb), img)


def test_unbacked_pages_are_never_answered_for():
    m = SparseRegions(2, 64)
    m.load_page(0, 0, np.arange(64, dtype=np.uint8))
    m.load_page(0, 2, np.arange(64, dtype=np.uint8))
    assert np.array_equal(m.read_block(0, 3, 16), np.arange(48, 64, dtype=np.uint8))
    with pytest.raises(UnbackedError):
        m.read_block(0, 4, 16)                      # page 1
    with pytest.raises(UnbackedError):
        m.read_block(1, 0, 16)                      # another region
    with pytest.raises(UnbackedError):
        m.read(0, 48, 32)                           # straddles into page 1
    before = m.pages[0][0].copy()
    with pytest.raises(UnbackedError):
        m.write(0, 48, np.full(32, 9, dtype=np.uint8))
    assert np.array_equal(m.pages[0][0], before)    # a refused write changes nothing
    with pytest.raises(UnbackedError):
        m.compact([0], [4], 16)
    with pytest.raises(UnbackedError):
        m.image([8, 4], 16)                         # block 8 is on page 2, block 4 is not backed
    assert m.backed() == [(0, 0), (0, 2)]


def test_offsets_above_4_gib_are_plain_integers():
    """A block id times a block size is a Python int in the model: pages far above 2^32 bytes resolve exactly."""
    page = 1 << 12
    m = SparseRegions(1, page)
    far = (1 << 33) // page
    for p in (far - 1, far):
        m.load_page(0, p, np.full(page, p % 251, dtype=np.uint8))
    bb = 1040
    b = (1 << 33) // bb                             # straddles the 2^33 line
    got = m.read_block(0, b, bb)
    below = (1 << 33) - b * bb
    assert (got[:below] == (far - 1) % 251).all() and (got[below:] == far % 251).all()
    m.write_block(0, b, bb, np.arange(bb, dtype=np.uint64).astype(np.uint8))
    assert m.pages[0][far][0] == below % 256 and m.pages[0][far - 1][-1] == (below - 1) % 256


def test_the_far_offset_cases_are_far():
    """The geometry the GPU tests of test_gpu_far_offsets.py assert before they launch anything, checked here as well: every
    candidate block and its 32-bit alias lie on backed pages, ragged sizes straddle the byte lines, and a split of the
    candidates into moves that cross 2^31 and 2^32 in both directions exists for every (size, variant)."""
    import test_gpu_far_offsets as F
    model = SparseRegions(1, F.PAGE)
    for p in F.BACKED:
        model.load_page(0, p, np.zeros(F.PAGE, dtype=np.uint8))
    for bb in F.BLOCK_BYTES:
        ids = F.check_geometry(bb)
        assert len(ids) == 16
        for b in ids:
            model.read(0, b * bb, 16), model.read(0, (b + 1) * bb - 16, 16)      # the model agrees: backed from end to end
        for variant in F.COMPACT_VARIANTS:
            src, dst = F.split_moves(ids, bb, seed=bb + variant)
            assert len(src) == len(dst) == 8 and not set(src) & set(dst)
