"""Offload of live blocks to pinned host memory and their restore (copy_blocks_to_host / copy_blocks_from_host, and
KVCacheManager.offload / .restore) on a real MI355X. Expected bytes come from a numpy restatement of the block-major host
image: image[i, r] = region r's bytes of block ids[i]."""
import os
import threading
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MiB = 1 << 20
PAGE = 2 * MiB
DEV = "cuda:0"
GUARD = 4096


@pytest.fixture()
def lib():
    from kvcached_amd import capi, vmm_ops
    saved = {k: os.environ.get(k) for k in ("KVCACHED_PHYS_RESERVE_MB", "KVCACHED_ZERO_BACKFILL")}
    os.environ["KVCACHED_ZERO_BACKFILL"] = "true"   # the default (compat, PRT): an unbacked slot reads 0, never faults
    yield vmm_ops, capi
    vmm_ops.shutdown_kvcached()
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _regions(ops, capi, n_regions, region_bytes):
    """Reserve and back `n_regions` regions of at least region_bytes each: 1 = the contiguous layout, else n_regions / 2
    layers with K and V halves. Returns uint8 views of the regions in kvc_get_region_bases order."""
    contiguous = n_regions == 1
    half = -(-region_bytes // PAGE) * PAGE
    ops.init_kvcached(DEV, PAGE, contiguous)
    if contiguous:
        ts = ops.create_kv_tensors(2 * half, 1, DEV, 1, 2, 0, False)   # one region of 2 * half bytes, 4 MiB slots
        assert ops.map_to_kv_tensors([k * 2 * PAGE for k in range(half // PAGE)])
        views = [ts[0].view(torch.uint8)]
    else:
        ts = ops.create_kv_tensors(2 * half, 1, DEV, n_regions // 2, 2, 0, False)
        assert ops.map_to_kv_tensors([k * PAGE for k in range(half // PAGE)])
        views = []
        for t in ts:
            u = t.view(torch.uint8)
            views += [u[:half], u[half:]]
    assert len(capi.get_region_bases(0)) == len(views) == n_regions
    assert [v.data_ptr() for v in views] == capi.get_region_bases(0)
    return views


def _ids(n, seed):
    """n distinct ids with gaps (every block has an untouched neighbour), shuffled."""
    rng = np.random.default_rng(seed)
    ids = rng.choice(np.arange(1, 3 * n + 2, 2), size=n, replace=False)   # odd ids only: the even ones are the canaries
    return [int(x) for x in ids]


def _fill(views, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    for v in views:
        v.copy_(torch.randint(0, 256, (v.numel(),), dtype=torch.uint8, device=DEV, generator=g))
    torch.cuda.synchronize()


def _pinned(nbytes, value):
    buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, pin_memory=True)
    buf.fill_(value)
    return buf


def _expected_image(regs, ids, bb):
    """numpy: image[i, r, :] = regs[r][ids[i]*bb : (ids[i]+1)*bb]"""
    stack = np.stack([r[:(max(ids) + 1) * bb].reshape(-1, bb) for r in regs])   # (R, blocks, bb)
    return np.ascontiguousarray(stack[:, ids, :].transpose(1, 0, 2)).reshape(-1)


N_MATRIX = [1, 37, 1024, 1025]
BB_MATRIX = [16, 2064, 18 * 1024, 32 * 1024, 48 * 1024]


@pytest.mark.parametrize("n_regions", [1, 2, 64])
@pytest.mark.parametrize("bb", BB_MATRIX)
def test_kernels_copy_blocks_byte_for_byte(lib, n_regions, bb):
    _copy_blocks_byte_for_byte(lib, n_regions, bb)


# Blocks of the contiguous layout (block_mem_size * layers * kv): 2 MiB for Llama-3-8B (128 tiles of 16 KiB), 497 664 B for the
# 27-layer MLA geometry (30 full tiles and a ragged 6 KiB one). One and two regions only: _regions backs 3 * max(ns) + 3 blocks
# per region, which at 64 regions would be 14 GiB of HBM for no extra coverage.
@pytest.mark.parametrize("n_regions", [1, 2])
@pytest.mark.parametrize("bb", [497664, 2 * MiB])
def test_kernels_copy_blocks_of_the_contiguous_layout(lib, n_regions, bb):
    _copy_blocks_byte_for_byte(lib, n_regions, bb)


def _copy_blocks_byte_for_byte(lib, n_regions, bb):
    ops, capi = lib
    ns = [n for n in N_MATRIX if n <= 37 or n * n_regions * bb <= 256 * MiB]   # 64 regions x 1024 large blocks: > 1 GiB images
    views = _regions(ops, capi, n_regions, (3 * max(ns) + 3) * bb)
    for n in ns:
        ids = _ids(n, seed=n * 7 + bb)
        _fill(views, seed=n + bb)
        regs = [v.cpu().numpy() for v in views]
        nbytes = n * n_regions * bb
        # device -> host: the image, nothing after it
        host = _pinned(nbytes, 0xA5)
        capi.copy_blocks_to_host(0, ids, bb, host.data_ptr())
        h = host.numpy()
        assert np.array_equal(h[:nbytes], _expected_image(regs, ids, bb)), (n, bb, n_regions)
        assert (h[nbytes:] == 0xA5).all()
        # host -> device: exactly the target blocks change, their neighbours (and everything else) do not
        rng = np.random.default_rng(n * 3 + bb)
        img = rng.integers(0, 256, size=nbytes, dtype=np.uint8)
        src = _pinned(nbytes, 0x5A)
        src.numpy()[:nbytes] = img
        capi.copy_blocks_from_host(0, ids, bb, src.data_ptr())
        want = img.reshape(n, n_regions, bb)
        for r, v in enumerate(views):
            exp = regs[r].copy()
            blocks = exp[:(max(ids) + 1) * bb].reshape(-1, bb)
            blocks[ids] = want[:, r, :]
            assert np.array_equal(v.cpu().numpy(), exp), (n, bb, n_regions, r)


def test_unbacked_block_and_pageable_buffer_are_refused(lib):
    ops, capi = lib
    bb = 32 * 1024
    ops.init_kvcached(DEV, PAGE, False)
    ts = ops.create_kv_tensors(8 * PAGE, 1, DEV, 2, 2, 0, False)
    assert ops.map_to_kv_tensors([0, PAGE, 3 * PAGE])          # page 2 of each half stays unbacked
    bpp = PAGE // bb
    host = _pinned(4 * 4 * bb, 0xC3)
    ids = capi.i64_array([1, bpp + 5, 2 * bpp + 7, 3 * bpp])  # the third lies on an unbacked slot
    for fn in (capi.lib.kvc_copy_blocks_to_host, capi.lib.kvc_copy_blocks_from_host):
        assert fn(0, ids, 4, bb, host.data_ptr(), None, 1) == capi.KVC_E_INVALID
        assert "not backed" in capi.last_error()
    torch.cuda.synchronize()
    assert (host.numpy() == 0xC3).all()
    # the same ids without the unbacked one pass; blocks beyond the tensors, a duplicate restore, bad sizes do not
    ok = capi.i64_array([1, bpp + 5, 3 * bpp])
    assert capi.lib.kvc_copy_blocks_to_host(0, ok, 3, bb, host.data_ptr(), None, 1) == capi.KVC_OK
    assert capi.lib.kvc_copy_blocks_to_host(0, capi.i64_array([4 * bpp]), 1, bb, host.data_ptr(), None, 1) == capi.KVC_E_INVALID
    assert capi.lib.kvc_copy_blocks_from_host(0, capi.i64_array([1, 1]), 2, bb, host.data_ptr(), None, 1) == capi.KVC_E_INVALID
    assert capi.lib.kvc_copy_blocks_to_host(0, capi.i64_array([1, 1]), 2, bb, host.data_ptr(), None, 1) == capi.KVC_OK
    assert capi.lib.kvc_copy_blocks_to_host(0, ok, 3, 24, host.data_ptr(), None, 1) == capi.KVC_E_INVALID
    assert capi.lib.kvc_copy_blocks_to_host(0, ok, 3, 0, host.data_ptr(), None, 1) == capi.KVC_E_INVALID
    assert capi.lib.kvc_copy_blocks_to_host(0, capi.i64_array([-1]), 1, bb, host.data_ptr(), None, 1) == capi.KVC_E_INVALID
    assert capi.lib.kvc_copy_blocks_to_host(0, ok, 3, bb, host.data_ptr() + 8, None, 1) == capi.KVC_E_INVALID
    # pageable memory
    pageable = np.full(4 * 4 * bb, 0x3C, dtype=np.uint8)
    for fn in (capi.lib.kvc_copy_blocks_to_host, capi.lib.kvc_copy_blocks_from_host):
        assert fn(0, ok, 3, bb, pageable.ctypes.data, None, 1) == capi.KVC_E_INVALID
        assert "pinned" in capi.last_error()
    assert (pageable == 0x3C).all()
    del ts


# ------------------------------------------------------------------ manager level
def _manager_setup(ops, monkeypatch, layout, n_pages=16, layers=4, prealloc=False, async_sched=False):
    """A KVCacheManager over backed-on-demand regions, and per-region (blocks, block_bytes) views in region order."""
    import kvcached_amd.kv_cache_manager as kcm
    contiguous = layout == "contiguous"
    kv = 1 if layout == "mla" else 2
    group = 1 if layout == "group1" else 0
    # MLA: one buffer per layer. (Its 18 KiB blocks straddle page edges, where available_size() promises blocks that alloc()
    # cannot hand out - the reference's accounting; the kernel-level matrix covers that block size and slot-straddling blocks.)
    cell = 2048
    bmem = 16 * cell
    monkeypatch.setattr(kcm, "CONTIGUOUS_LAYOUT", contiguous)
    monkeypatch.setattr(kcm, "PAGE_PREALLOC_ENABLED", prealloc)
    ops.init_kvcached(DEV, PAGE, contiguous)
    nb = n_pages * (PAGE // bmem)
    size = n_pages * PAGE * kv
    if group:
        ops.create_kv_tensors(size, 1, DEV, layers, kv, 0, False)   # group 0 exists too, untouched
    raw = ops.create_kv_tensors(size, 1, DEV, layers, kv, group, False)
    m = kcm.KVCacheManager(num_blocks=nb, block_size=16, cell_size=cell, num_layers=layers, num_kv_buffers=kv,
                           group_id=group, async_sched=async_sched)
    assert m._post_init_done.wait(10)
    if contiguous:   # [block][layer][kv][bmem]
        u = raw[0].view(torch.uint8)[:nb * layers * kv * bmem].view(nb, layers * kv, bmem)
        views = [u[:, j] for j in range(layers * kv)]
    else:
        views = []
        for t in raw:
            u = t.view(torch.uint8)
            half = u.numel() // kv
            views += [u[h * half:h * half + nb * bmem].view(nb, bmem) for h in range(kv)]
    assert len(m._block_geometry()[0]) == (1 if contiguous else len(views))   # (contiguous: views are parts of a block)
    return m, views


def _pattern(ids, r, bmem):
    ids_t = torch.tensor(ids, dtype=torch.int64, device=DEV)
    col = torch.arange(bmem, dtype=torch.int64, device=DEV)
    return ((col[None, :] * 7 + ids_t[:, None] * 131 + r * 17 + (col[None, :] >> 9) * ids_t[:, None]) % 251).to(torch.uint8)


def _stamp(views, ids):
    for r, v in enumerate(views):
        v[torch.tensor(ids, device=DEV)] = _pattern(ids, r, v.shape[1])


def _holds(views, new_ids, old_ids):
    for r, v in enumerate(views):
        got = v[torch.tensor(new_ids, device=DEV)]
        if not torch.equal(got, _pattern(old_ids, r, v.shape[1])):
            return False
    return True


@pytest.mark.parametrize("layout", ["per_layer", "contiguous", "mla", "group1"])
def test_offload_and_restore_through_the_manager(lib, monkeypatch, layout):
    ops, capi = lib
    m, views = _manager_setup(ops, monkeypatch, layout)
    bpp = views[0].shape[0] // 16
    ids = m.alloc(bpp * 6)
    live = ids[bpp:3 * bpp] + ids[4 * bpp:4 * bpp + 9] + ids[5 * bpp + 3:5 * bpp + 40]
    _stamp(views, ids)
    torch.cuda.synchronize()
    inuse = m.page_allocator.get_num_inuse_pages()
    h = m.offload(live)                              # two whole pages among them
    assert h.block_ids == live
    assert m.page_allocator.get_num_inuse_pages() == inuse - 2
    bases, bb = m._block_geometry()
    assert h.data.is_pinned() and h.data.numel() == len(live) * len(bases) * bb
    # the freed blocks are handed out again and scribbled over
    rest = m.alloc(m.available_size())
    for v in views:
        v[torch.tensor(rest, device=DEV)] = 0xEE
    torch.cuda.synchronize()
    assert m.restore(h) is None                      # the pool is full: nothing happens
    m.free(rest)
    new = m.restore(h)
    assert new is not None and len(new) == len(live)
    m._check_live_blocks(new)                        # allocated, not free / reserved
    assert _holds(views, new, live)
    # a second restore is a second, independent copy
    again = m.restore(h)
    assert again is not None and not set(again) & set(new)
    assert _holds(views, again, live) and _holds(views, new, live)
    untouched = [b for b in ids if b not in set(live)]
    assert _holds(views, untouched, untouched)
    h.release()
    assert h.data is None


def test_offload_and_restore_are_ordered_on_the_current_stream(lib, monkeypatch):
    """Llama-3-8B geometry (32 layers, K/V, 32 KiB blocks): writes queued just before offload are in the image; a read
    queued just after restore sees the data; a >= 1 GiB restore whose handle is dropped at once keeps its pinned buffer
    until the copy is over, even when new pinned tensors of the same size are filled right away."""
    ops, capi = lib
    m, views = _manager_setup(ops, monkeypatch, "per_layer", n_pages=16, layers=32)
    bpp = views[0].shape[0] // 16
    ids = m.alloc(bpp * 8)                                        # 512 blocks x 64 regions x 32 KiB = 1 GiB
    ids_t = torch.tensor(ids, device=DEV)
    pats = [_pattern(ids, r, v.shape[1]) for r, v in enumerate(views)]
    out = torch.empty(1 << 30, dtype=torch.uint8, pin_memory=True)
    big = torch.empty(1 << 30, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    big.fill_(1)                                                  # keeps the stream busy while the patterns queue up
    for v, p in zip(views, pats):                                 # device-side writes only, no synchronise
        v[ids_t] = p
    h = m.offload(ids, out=out)
    del out
    assert h.data.numel() == 1 << 30
    regs = [p.cpu().numpy() for p in pats]
    img = h.data.numpy().reshape(len(ids), len(views), -1)
    for r in range(len(views)):
        assert np.array_equal(img[:, r, :], regs[r]), r
    new = m.restore(h)
    got = [v[torch.tensor(new, device=DEV)].clone() for v in views[:4]]    # queued right behind the copy
    torch.cuda.synchronize()
    for r in range(4):
        assert torch.equal(got[r], _pattern(ids, r, views[r].shape[1])), r
    m.free(new)
    # drop the handle the moment the copy is queued, then reuse pinned memory of the same size at once
    new = m.restore(h)
    del h, img
    fresh = [torch.empty(1 << 30, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    for f in fresh:
        f.fill_(0xFF)
    torch.cuda.synchronize()
    assert _holds(views, new, ids)
    m.free(new)


def test_round_trips_next_to_background_mapping(lib, monkeypatch):
    """Default (PRT) mode, prealloc thread on, a second thread allocating and freeing other blocks in a loop: every
    offload / restore round trip is bit-exact."""
    ops, capi = lib
    m, views = _manager_setup(ops, monkeypatch, "per_layer", n_pages=32, layers=4, prealloc=True, async_sched=True)
    bpp = views[0].shape[0] // 32
    stop = threading.Event()
    errors = []

    def churn():
        rng = np.random.default_rng(1)
        try:
            while not stop.is_set():
                got = m.alloc(int(rng.integers(1, 3 * bpp)))
                time.sleep(0.001)
                if got:
                    m.free(got)
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)

    t = threading.Thread(target=churn, daemon=True)
    t.start()
    rounds = 0
    try:
        t0 = time.time()
        while time.time() - t0 < 4.0:
            ids = m.alloc(bpp + 17)
            assert ids is not None
            _stamp(views, ids)
            h = m.offload(ids)
            new = m.restore(h)
            assert new is not None
            torch.cuda.synchronize()
            assert _holds(views, new, ids), rounds
            m.free(new)
            rounds += 1
    finally:
        stop.set()
        t.join(10)
    assert not errors and rounds > 5


def test_offload_a_page_id_of_the_engine_geometry(lib, monkeypatch):
    """Lanes on, 64 regions (32 layers, K/V): offloading every block of one page id gives its memory back after trim()."""
    ops, capi = lib
    os.environ["KVCACHED_PHYS_RESERVE_MB"] = "0"
    m, views = _manager_setup(ops, monkeypatch, "per_layer", n_pages=16, layers=32)
    assert capi.get_option(capi.OPT_LANES_PER_BUFFER) > 0                               # page ids are backed by lanes
    bpp = views[0].shape[0] // 16
    ids = m.alloc(bpp * 4)
    _stamp(views, ids)
    torch.cuda.synchronize()
    m.trim()
    mapped = m.get_mapped_memory_size()
    page = ids[2 * bpp:3 * bpp]
    h = m.offload(page)
    m.trim()
    assert mapped - m.get_mapped_memory_size() == 32 * 2 * PAGE
    new = m.restore(h)
    torch.cuda.synchronize()
    assert _holds(views, new, page)
    others = ids[:2 * bpp] + ids[3 * bpp:]
    assert _holds(views, others, others)
