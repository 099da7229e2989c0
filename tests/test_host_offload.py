"""KVCacheManager.offload / .restore and their C entries, host side (the "cpu" device): every refusal happens before
anything changes, and the copies themselves refuse a device without a GPU. The bytes are checked on the MI355X
(tests/test_gpu_host_offload.py)."""
import ctypes
import os

import pytest
import torch

import kvc_testlib as T

MiB = 1 << 20
PAGE = 2 * MiB
BPP = 64   # 32 KiB blocks per 2 MiB page


@pytest.fixture()
def cpu_ops():
    from kvcached_amd import capi, vmm_ops
    vmm_ops.init_kvcached("cpu", PAGE, False)
    T.set_product_phys_pages(1 << 30, PAGE, 2, 2)
    yield vmm_ops, capi
    vmm_ops.shutdown_kvcached()
    capi.set_mem_info_override(0, 0)


def _manager(ops, **kw):
    import kvcached_amd.kv_cache_manager as kcm
    ops.create_kv_tensors(16 * PAGE * 2, 1, "cpu", 2, 2, 0, False)
    m = kcm.KVCacheManager(num_blocks=16 * BPP, block_size=16, cell_size=2048, num_layers=2, **kw)
    assert m._post_init_done.wait(10)
    return m


def _state(m):
    pa = m.page_allocator
    pages = {pid: sorted(p.get_free_blocks()) for pid, p in m.avail_pages.items()}
    return (m.available_size(), pa.get_num_inuse_pages(), pa._page_list(0), pa._page_list(1), pages,
            sorted(m.full_pages), list(m.reserved_blocks), m.num_avail_blocks)


def test_c_entries_refuse_the_cpu_device(cpu_ops):
    ops, capi = cpu_ops
    ops.create_kv_tensors(16 * PAGE * 2, 1, "cpu", 2, 2, 0, False)
    buf = (ctypes.c_char * (1 << 16))()
    ids = capi.i64_array([0, 1])
    assert capi.lib.kvc_copy_blocks_to_host(0, ids, 2, 16, ctypes.addressof(buf), None, 1) == capi.KVC_E_NO_GPU
    assert capi.lib.kvc_copy_blocks_from_host(0, ids, 2, 16, ctypes.addressof(buf), None, 1) == capi.KVC_E_NO_GPU
    with pytest.raises(capi.KvcError) as e:
        capi.copy_blocks_to_host(0, [0], 16, ctypes.addressof(buf))
    assert e.value.code == capi.KVC_E_NO_GPU


def test_offload_refusals_leave_the_manager_unchanged(cpu_ops):
    ops, capi = cpu_ops
    m = _manager(ops, reserve_null_block=True)
    ids = m.alloc(3 * BPP)
    assert ids is not None and 0 not in ids
    m.free(ids[10:20])                     # free blocks inside a page in use
    assert m.try_to_reserve(5)
    free_in_page = sorted(set(ids[10:20]) - set(m.reserved_blocks))[0]
    reserved = m.reserved_blocks[0]
    never_used = 15 * BPP + 3              # a block of a page that is not in use
    before = _state(m)
    for bad in ([], [ids[0], ids[1], ids[0]], [0, ids[0]], [ids[0], free_in_page], [never_used],
                [reserved], [ids[0], -1], [m.num_blocks]):
        with pytest.raises(ValueError):
            m.offload(bad)
        assert _state(m) == before, bad
    # an `out` that does not fit is refused before anything happens too
    with pytest.raises(ValueError):
        m.offload([ids[0]], out=torch.empty(16, dtype=torch.uint8))
    assert _state(m) == before


def test_offload_whose_copy_fails_keeps_every_block(cpu_ops):
    """The copy fails (no GPU): the blocks stay allocated, nothing is freed."""
    ops, capi = cpu_ops
    m = _manager(ops)
    ids = m.alloc(2 * BPP + 7)
    before = _state(m)
    with pytest.raises(capi.KvcError) as e:
        m.offload(ids[:BPP + 3])
    assert e.value.code == capi.KVC_E_NO_GPU
    assert _state(m) == before
    m.free(ids)                            # every one of them is still allocated
    assert m.page_allocator.get_num_inuse_pages() == 0


def test_offload_refuses_tensor_parallel_managers(cpu_ops):
    ops, capi = cpu_ops
    import kvcached_amd.kv_cache_manager as kcm
    from kvcached_amd import tp_ipc_util as tp
    ops.create_kv_tensors(32 * MiB, 1, "cpu", 2, 2, 0, False)
    servers = [tp.start_worker_listener_thread(r) for r in range(2)]
    try:
        m = kcm.KVCacheManager(num_blocks=512, block_size=16, cell_size=2048, num_layers=2, world_size=2)
        assert m._post_init_done.wait(10)
        got = m.alloc(10)
        with pytest.raises(RuntimeError, match="tensor parallelism"):
            m.offload(got[:4])
        fake = kcm.OffloadedBlocks([1], torch.zeros(64 * 1024, dtype=torch.uint8), (0, False, 4, 32 * 1024))
        with pytest.raises(RuntimeError):
            m.restore(fake)
        m.free(got)
        del m
    finally:
        tp._channels.close()
        for srv in servers:
            srv.close()


def test_restore_refuses_a_foreign_geometry(cpu_ops):
    ops, capi = cpu_ops
    import kvcached_amd.kv_cache_manager as kcm
    m = _manager(ops)
    bases, block_bytes = m._block_geometry()
    assert (len(bases), block_bytes) == (4, 32 * 1024)        # 2 layers x K/V, 16 tokens x 2 KiB
    before = _state(m)
    for geometry in ((1, False, 4, block_bytes), (0, True, 4, block_bytes), (0, False, 2, block_bytes),
                     (0, False, 4, 16 * 1024)):
        h = kcm.OffloadedBlocks([3, 4], torch.zeros(2 * 4 * block_bytes, dtype=torch.uint8), geometry)
        with pytest.raises(ValueError, match="geometry"):
            m.restore(h)
        assert _state(m) == before
    # the matching geometry passes the check and fails only at the copy (no GPU), with the blocks it took given back
    h = kcm.OffloadedBlocks([3, 4], torch.zeros(2 * 4 * block_bytes, dtype=torch.uint8), (0, False, 4, block_bytes))
    with pytest.raises(RuntimeError):
        m.restore(h)
    assert m.available_size() == before[0] and m.page_allocator.get_num_inuse_pages() == 0
    assert not m.avail_pages and not m.full_pages


def test_block_geometry_of_every_layout(cpu_ops, monkeypatch):
    """compact() and offload() share one derivation: one region per layer and K/V half, per layer for MLA, one region
    holding all layers and K/V of a block in the contiguous layout."""
    ops, capi = cpu_ops
    import kvcached_amd.kv_cache_manager as kcm
    ops.create_kv_tensors(16 * PAGE, 1, "cpu", 3, 1, 0, False)
    m = kcm.KVCacheManager(num_blocks=16 * 32, block_size=16, cell_size=4096, num_layers=3, num_kv_buffers=1)
    assert m._post_init_done.wait(10)
    bases, bb = m._block_geometry()
    assert (len(bases), bb) == (3, 64 * 1024)
    monkeypatch.setattr(kcm, "CONTIGUOUS_LAYOUT", True)
    assert m._block_geometry()[1] == 64 * 1024 * 3
