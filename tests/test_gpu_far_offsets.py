"""The three byte movers (compact_blocks, copy_blocks_to_host, copy_blocks_from_host) where base + id * block_bytes lies
beyond 2^31, 2^32 and 2^33 bytes, on a real MI355X, against the sparse numpy model (kvc_sparse_model.py, pinned on the CPU in
test_sparse_model.py); then the same through KVCacheManager with block ids above 131072.

Four regions of 10 GiB of address space each, of which only 22 pages around the byte lines are backed. The default (PRT)
mode is set explicitly: an unbacked slot reads zero and drops writes, it never faults - and the block ids are chosen so that
even an offset truncated to 32 bits stays on backed, compared memory. After every operation EVERY backed page of every region
is compared with the model, which is what sees a write that landed 4 GiB too low."""
import os

import numpy as np
import pytest
import torch

from kvc_sparse_model import SparseRegions
from test_gpu_host_offload import GUARD, _holds, _manager_setup, _pattern, _pinned
from test_gpu_host_offload import lib  # noqa: F401  (fixture: default PRT mode set explicitly, shutdown afterwards)

pytestmark = pytest.mark.gpu

MiB = 1 << 20
PAGE = 2 * MiB
DEV = "cuda:0"
HALF_PAGES = 5120
HALF = HALF_PAGES * PAGE                                         # 10 GiB per region
LINES = [0, 1 << 31, 1 << 32, 1 << 33, HALF]
BACKED = sorted(set(range(0, 3)) | set(range(1021, 1027)) | set(range(2046, 2051)) | set(range(4094, 4099))
                | set(range(5117, 5120)))
N_REGIONS = 4
BLOCK_BYTES = [16, 1040, 2064, 18432, 32768, 49152, 497664, 2 * MiB]
COMPACT_VARIANTS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]


def candidates(bb):
    """Block ids L // bb + d around every byte line L, as far as they lie inside a region."""
    out = []
    for line in LINES:
        for d in (-2, -1, 0, 1):
            b = line // bb + d
            if b >= 0 and (b + 1) * bb <= HALF and b not in out:
                out.append(b)
    return out


def _pages_of(off, n):
    return set(range(off // PAGE, (off + n - 1) // PAGE + 1))


def check_geometry(bb):
    """What makes this a far-offset test, asserted before anything is launched: every candidate block lies wholly on backed
    pages; so does the place where an offset truncated to 32 bits would put it; and a block size that does not divide the
    page gives blocks that straddle the 2^31, 2^32 and 2^33 byte lines."""
    ids = candidates(bb)
    backed = set(BACKED)
    assert len(ids) >= 14 and len(set(ids)) == len(ids)
    for b in ids:
        off = b * bb
        assert _pages_of(off, bb) <= backed, (bb, b)
        assert _pages_of(off % (1 << 32), bb) <= backed, (bb, b)
    for line in (1 << 31, 1 << 32, 1 << 33):
        assert sum(1 for b in ids if b * bb >= line) >= 2 and sum(1 for b in ids if (b + 1) * bb <= line) >= 2
        if PAGE % bb:
            assert any(b * bb < line < (b + 1) * bb for b in ids), (bb, line)
    return ids


def _crosses(src, dst, bb, line):
    down = any(s * bb >= line > d * bb for s, d in zip(src, dst))
    up = any(d * bb >= line > s * bb for s, d in zip(src, dst))
    return down and up


def split_moves(ids, bb, seed):
    """Disjoint src / dst halves of the candidates, split at random: the first seed from `seed` on whose move list crosses
    the 2^31 and the 2^32 byte line in both directions."""
    half = len(ids) // 2
    for s in range(seed, seed + 2000):
        perm = [int(x) for x in np.random.default_rng(s).permutation(ids)]
        src, dst = perm[:half], perm[half:2 * half]
        if _crosses(src, dst, bb, 1 << 31) and _crosses(src, dst, bb, 1 << 32):
            return src, dst
    raise AssertionError(f"no split of {ids} crosses both lines in both directions")


class Far:
    def __init__(self, ops, capi, views):
        self.ops, self.capi, self.views = ops, capi, views
        self.model = SparseRegions(N_REGIONS, PAGE)
        rng = np.random.default_rng(2024)
        for r in range(N_REGIONS):
            for p in BACKED:
                self.model.load_page(r, p, rng.integers(0, 256, size=PAGE, dtype=np.uint8))
        self.keys = self.model.backed()

    def _dev_page(self, r, p):
        return self.views[r][p * PAGE:(p + 1) * PAGE]

    def upload(self):
        """The model's bytes onto the device: every test starts from the same, known state."""
        for r, p in self.keys:
            self._dev_page(r, p).copy_(torch.from_numpy(self.model.pages[r][p]))
        torch.cuda.synchronize()

    def assert_matches(self, what):
        """Every backed page of every region against the model."""
        torch.cuda.synchronize()
        got = torch.stack([self._dev_page(r, p) for r, p in self.keys]).cpu().numpy()
        bad = []
        for k, (r, p) in enumerate(self.keys):
            want = self.model.pages[r][p]
            if not np.array_equal(got[k], want):
                at = int(np.flatnonzero(got[k] != want)[0])
                bad.append((r, p, hex(p * PAGE + at)))
        assert not bad, f"{what}: (region, page, first differing byte offset) {bad[:12]} ({len(bad)} pages differ)"


@pytest.fixture(scope="module")
def far():
    from kvcached_amd import capi, vmm_ops
    saved = os.environ.get("KVCACHED_ZERO_BACKFILL")
    os.environ["KVCACHED_ZERO_BACKFILL"] = "true"   # the default (PRT): an unbacked slot reads 0 and drops writes, never faults
    try:
        vmm_ops.init_kvcached(DEV, PAGE, False)
        ts = vmm_ops.create_kv_tensors(2 * HALF, 1, DEV, 2, 2, 0, False)
        assert vmm_ops.map_to_kv_tensors([p * PAGE for p in BACKED])
        views = []
        for t in ts:
            u = t.view(torch.uint8)
            assert u.numel() == 2 * HALF
            views += [u[:HALF], u[HALF:]]
        assert [v.data_ptr() for v in views] == capi.get_region_bases(0) and len(views) == N_REGIONS
        f = Far(vmm_ops, capi, views)
        f.upload()
        f.assert_matches("after the first upload")
        yield f
    finally:
        vmm_ops.shutdown_kvcached()
        if saved is None:
            os.environ.pop("KVCACHED_ZERO_BACKFILL", None)
        else:
            os.environ["KVCACHED_ZERO_BACKFILL"] = saved


@pytest.mark.parametrize("variant", COMPACT_VARIANTS)
@pytest.mark.parametrize("bb", BLOCK_BYTES)
def test_far_compact_blocks(far, bb, variant):
    ids = check_geometry(bb)
    src, dst = split_moves(ids, bb, seed=bb + variant)
    assert not set(src) & set(dst)
    far.upload()
    far.capi.set_option(far.capi.OPT_COMPACT_VARIANT, variant)
    try:
        far.capi.compact_blocks(far.capi.get_region_bases(0), src, dst, bb)
    finally:
        far.capi.set_option(far.capi.OPT_COMPACT_VARIANT, 0)
    far.model.compact(src, dst, bb)
    far.assert_matches(f"compact_blocks variant {variant}, {bb}-byte blocks, moves {list(zip(src, dst))}")


@pytest.mark.parametrize("bb", BLOCK_BYTES)
def test_far_host_round_trip(far, bb):
    ids = check_geometry(bb)
    rng = np.random.default_rng(bb)
    ids = [int(x) for x in rng.permutation(ids)]
    far.upload()
    nbytes = len(ids) * N_REGIONS * bb
    # device -> host: the image, nothing behind it, nothing changed on the device
    host = _pinned(nbytes, 0xA5)
    far.capi.copy_blocks_to_host(0, ids, bb, host.data_ptr())
    h = host.numpy()
    want = far.model.image(ids, bb)
    if not np.array_equal(h[:nbytes], want):
        rows = np.flatnonzero((h[:nbytes].reshape(-1, bb) != want.reshape(-1, bb)).any(axis=1))
        raise AssertionError(f"{bb}-byte blocks: image rows (block * {N_REGIONS} + region) {rows[:16].tolist()} differ; "
                             f"ids {ids}")
    assert (h[nbytes:] == 0xA5).all() and h.size == nbytes + GUARD
    far.assert_matches(f"copy_blocks_to_host, {bb}-byte blocks")
    # host -> device: a fresh image becomes exactly these blocks
    img = rng.integers(0, 256, size=nbytes, dtype=np.uint8)
    src = _pinned(nbytes, 0x5A)
    src.numpy()[:nbytes] = img
    far.capi.copy_blocks_from_host(0, ids, bb, src.data_ptr())
    far.model.scatter(img, ids, bb)
    far.assert_matches(f"copy_blocks_from_host, {bb}-byte blocks, ids {ids}")
    assert np.array_equal(src.numpy()[:nbytes], img) and (src.numpy()[nbytes:] == 0x5A).all()


# ------------------------------------------------------------------ through the manager, block ids above 131072
BMEM = 32 * 1024
BPP = PAGE // BMEM                                               # 64 blocks per page
N_PAGES = 2304                                                   # 4.5 GiB per half: page 2048 starts at 2^32 bytes
FAR_PAGE = 2100


def _big_manager(ops, monkeypatch):
    m, views = _manager_setup(ops, monkeypatch, "per_layer", n_pages=N_PAGES, layers=1)
    assert len(views) == 2 and views[0].shape == (N_PAGES * BPP, BMEM)
    ids = m.alloc(N_PAGES * BPP)                                 # every block: 9 GiB of HBM while the test runs
    assert ids is not None and sorted(ids) == list(range(N_PAGES * BPP))
    return m, views


def _stamp_chunked(views, ids, chunk=2048):
    for k in range(0, len(ids), chunk):
        part = ids[k:k + chunk]
        idx = torch.tensor(part, device=DEV)
        for r, v in enumerate(views):
            v[idx] = _pattern(part, r, v.shape[1])


def _holds_chunked(views, new_ids, old_ids, chunk=2048):
    return all(_holds(views, new_ids[k:k + chunk], old_ids[k:k + chunk]) for k in range(0, len(new_ids), chunk))


def _page_blocks(p, keep):
    return list(range(p * BPP, p * BPP + keep))


@pytest.mark.parametrize("full_low", [True, False], ids=["far_to_near", "near_to_far"])
def test_manager_compaction_across_the_4_gib_line(lib, monkeypatch, full_low):
    """Sparse pages on one side of the 2^32-byte line are emptied into a nearly full page on the other side."""
    ops, capi = lib
    m, views = _big_manager(ops, monkeypatch)
    if full_low:      # page 0 keeps 60 of 64 blocks, pages >= 2100 keep one or two each
        full_pages, sparse_pages = [0], list(range(FAR_PAGE, FAR_PAGE + 40))
    else:             # the fullest page lies far, the sparse ones are low
        full_pages, sparse_pages = [N_PAGES - 1], list(range(3, 43))
    live = []
    for p in full_pages:
        live += _page_blocks(p, 60)
    for k, p in enumerate(sparse_pages):
        live += _page_blocks(p, 1 + k % 2)
    _stamp_chunked(views, live)
    torch.cuda.synchronize()
    keep = set(live)
    m.free([b for b in range(N_PAGES * BPP) if b not in keep])
    plan = m.plan_compaction()
    if full_low:
        assert any(s * BMEM >= (1 << 32) > d * BMEM for s, d in plan), plan[:8]
    else:
        assert any(d * BMEM >= (1 << 32) > s * BMEM for s, d in plan), plan[:8]
    assert sum(1 for _, d in plan if d // BPP == full_pages[0]) == 4       # its four free blocks are all filled
    inuse = m.page_allocator.get_num_inuse_pages()
    remap = m.compact()
    assert remap == dict(plan) and len(remap) >= 4
    assert m.page_allocator.get_num_inuse_pages() < inuse
    new = [remap.get(b, b) for b in live]
    assert len(set(new)) == len(new)
    m._check_live_blocks(new)
    torch.cuda.synchronize()
    assert _holds(views, new, live)
    m.free(new)


def test_manager_offload_and_restore_on_both_sides_of_the_line(lib, monkeypatch):
    ops, capi = lib
    m, views = _big_manager(ops, monkeypatch)
    line_block = (1 << 32) // BMEM                               # block 131072
    live = (list(range(5, 40)) + list(range(line_block - 70, line_block + 70))
            + _page_blocks(FAR_PAGE, 64) + list(range(N_PAGES * BPP - 33, N_PAGES * BPP)))
    rng = np.random.default_rng(5)
    live = [int(x) for x in rng.permutation(live)]
    _stamp_chunked(views, live)
    torch.cuda.synchronize()
    h = m.offload(live)
    assert h.block_ids == live and h.data.numel() == len(live) * 2 * BMEM
    img = torch.from_numpy(h.data.numpy().reshape(len(live), 2, BMEM))
    for r in range(2):
        assert torch.equal(img[:, r], _pattern(live, r, BMEM).cpu()), r
    # scribble over where they were (freed blocks are handed out again; FAR_PAGE's page went back whole)
    rest = m.alloc(len(live))
    assert rest is not None
    for v in views:
        v[torch.tensor(rest, device=DEV)] = 0xEE
    torch.cuda.synchronize()
    m.free(rest)
    new = m.restore(h)
    assert new is not None and len(new) == len(live)
    torch.cuda.synchronize()
    m._check_live_blocks(new)
    assert _holds(views, new, live)
    assert any(b >= line_block for b in new) and any(b < line_block for b in new)
    h.release()
    m.free(new)


def test_manager_offload_image_above_4_gib(lib, monkeypatch):
    """70 000 live blocks x 2 regions x 32 KiB = 4.27 GiB of pinned memory in one image: row offsets i * n_regions * block_bytes
    beyond 2^32 on the host side, 69 launches."""
    ops, capi = lib
    m, views = _big_manager(ops, monkeypatch)
    n = 70_000
    assert n * 2 * BMEM > (1 << 32)
    rng = np.random.default_rng(6)
    live = [int(x) for x in rng.choice(N_PAGES * BPP, size=n, replace=False)]
    _stamp_chunked(views, live)
    torch.cuda.synchronize()
    h = m.offload(live)
    assert h.data.is_pinned() and h.data.numel() == n * 2 * BMEM
    img = h.data.view(n, 2, BMEM)
    chunk = 2048
    for k in range(0, n, chunk):                                 # the whole image against the pattern, in pieces
        part = live[k:k + chunk]
        got = img[k:k + chunk].to(DEV)
        for r in range(2):
            assert torch.equal(got[:, r], _pattern(part, r, BMEM)), (k, r)
    rest = m.alloc(n)                                            # the freed blocks are handed out again and scribbled over
    assert rest is not None
    for v in views:
        for k in range(0, n, 8192):
            v[torch.tensor(rest[k:k + 8192], device=DEV)] = 0xEE
    torch.cuda.synchronize()
    m.free(rest)
    new = m.restore(h)
    assert new is not None and len(new) == n
    torch.cuda.synchronize()
    assert _holds_chunked(views, new, live)
    h.release()
    m.free(new)
