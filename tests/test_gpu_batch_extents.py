"""Run-sized extents of up to one batch (1024 x 2 MiB) and PRT rest mappings that follow the runs they replace, on a real
MI355X: a compat batch of 1024 adjacent slots is ONE page-table ioctl each way, and the two hazards a long mapping brings -
a page taken out of the middle of a 1024-page extent, single slots backed out of the middle of a 1024-slot PRT mapping
whose neighbours were just read - leave every word where it belongs."""
import os
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

MiB = 1 << 20
PAGE = 2 * MiB
DEV = "cuda:0"
WORDS = PAGE // 4


@pytest.fixture()
def compat():
    from kvcached_amd import capi, vmm_ops
    had = os.environ.get("KVCACHED_PHYS_RESERVE_MB")
    os.environ.setdefault("KVCACHED_PHYS_RESERVE_MB", "0")
    os.environ["KVCACHED_ZERO_BACKFILL"] = "true"
    try:
        vmm_ops.init_kvcached(DEV, PAGE, False)
    finally:
        os.environ.pop("KVCACHED_ZERO_BACKFILL", None)
    t = vmm_ops.create_kv_tensors(4096 * PAGE, 2, DEV, 1, 1, 0, True)[0]
    if capi.get_option(capi.OPT_EFFECTIVE_BACKEND) != 3 or capi.get_option(capi.OPT_KFD_CREATE_ACTIVE) != 1:
        vmm_ops.shutdown_kvcached()
        pytest.skip("needs the drm backend with pages straight from KFD")
    assert capi.get_option(capi.OPT_MAX_EXTENT_PAGES) == 1024
    capi.set_option(capi.OPT_PROFILE, 1)
    yield vmm_ops, capi, t.view(torch.int32).view(4096, WORDS)
    capi.set_option(capi.OPT_PROFILE, 0)
    vmm_ops.shutdown_kvcached()
    if had is None:
        os.environ.pop("KVCACHED_PHYS_RESERVE_MB", None)


def _slots(first, n, seed=0):
    offs = [(first + i) * PAGE for i in range(n)]
    random.Random(seed).shuffle(offs)
    return offs


def test_a_compat_batch_of_1024_slots_is_one_ioctl_each_way(compat):
    ops, capi, slots = compat
    capi.reset_stats()
    assert ops.map_to_kv_tensors(_slots(1024, 1024))
    assert capi.get_option(capi.OPT_SEG_MAP_IOCTL_COUNT) == 1
    assert int(torch.count_nonzero(slots[1024:2048])) == 0
    creates = capi.get_option(capi.OPT_KFD_CREATES)
    slots[1024:2048] = 7
    torch.cuda.synchronize()
    capi.reset_stats()
    assert ops.unmap_from_kv_tensors(_slots(1024, 1024, 1))
    assert capi.get_option(capi.OPT_SEG_UNMAP_IOCTL_COUNT) == 1
    assert int(torch.count_nonzero(slots[1024:2048])) == 0          # compat: a freed slot reads zero when unmap returns
    capi.reset_stats()
    assert ops.map_to_kv_tensors(_slots(2048, 1024, 2))               # other slots, the same 2 GiB extent
    st = capi.get_stats()
    assert capi.get_option(capi.OPT_SEG_MAP_IOCTL_COUNT) == 1 and st["handles_created"] == 0 and st["handles_reused"] == 1024
    assert capi.get_option(capi.OPT_KFD_CREATES) == creates
    assert int(torch.count_nonzero(slots[2048:3072])) == 0           # recycled, dirty, zero again
    assert ops.unmap_from_kv_tensors(_slots(2048, 1024))


def test_a_page_out_of_the_middle_of_a_1024_page_extent(compat):
    ops, capi, slots = compat
    assert ops.map_to_kv_tensors(_slots(0, 1024))
    stamp = torch.arange(1, 1025, dtype=torch.int32, device=DEV)
    slots[0:1024] = stamp[:, None]
    torch.cuda.synchronize()
    for mid in (511, 512, 64, 1000):
        before = int(slots[mid - 1:mid + 2].sum())                    # its neighbours are read (their translations are live)
        torch.cuda.synchronize()
        capi.reset_stats()
        assert ops.unmap_from_kv_tensors([mid * PAGE])
        assert capi.get_option(capi.OPT_SEG_UNMAP_IOCTL_COUNT) == 1
        assert int(torch.count_nonzero(slots[mid])) == 0
        assert int(slots[mid - 1:mid + 2].sum()) == before - (mid + 1) * WORDS
        assert ops.map_to_kv_tensors([mid * PAGE])                    # backed again: whichever page, it reads zero
        assert int(torch.count_nonzero(slots[mid])) == 0
        slots[mid] = mid + 1
        torch.cuda.synchronize()
        assert torch.equal(slots[0:1024], stamp[:, None].expand(1024, WORDS)), f"a slot lost its page after slot {mid}"
    assert ops.unmap_from_kv_tensors(_slots(0, 1024))


def test_single_slots_out_of_a_1024_slot_prt_mapping_whose_neighbours_were_read(compat):
    ops, capi, slots = compat
    assert capi.get_option(capi.OPT_PRT) == 1                         # unbacked slots rest in PRT, not in the zero extent
    assert ops.map_to_kv_tensors(_slots(1024, 1024))
    capi.reset_stats()
    assert ops.unmap_from_kv_tensors(_slots(1024, 1024))
    assert capi.get_option(capi.OPT_SEG_UNMAP_IOCTL_COUNT) == 1                     # one PRT mapping of 1024 slots now
    for round_, picks in enumerate(([1024 + 300], [1024 + 301, 1024 + 700], [1024 + 1, 1024 + 1022])):
        assert int(torch.count_nonzero(slots[1024:2048])) == 0       # every neighbour looked at: PRT entries in the TLBs
        torch.cuda.synchronize()
        assert ops.map_to_kv_tensors([p * PAGE for p in picks])
        for p in picks:
            slots[p] = p + 17 * round_
        torch.cuda.synchronize()
        for p in picks:
            assert int((slots[p] != p + 17 * round_).sum()) == 0, f"slot {p}: writes did not land or reads are stale"
        assert ops.unmap_from_kv_tensors([p * PAGE for p in picks])
    assert int(torch.count_nonzero(slots[1024:2048])) == 0
