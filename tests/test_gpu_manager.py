"""KVCacheManager on a real MI355X.

1. The golden traces of the REAL reference, replayed with every map/unmap request executed on
   the GPU (hipMemMap + zero fill): block ids / page offsets / counters must still be bit-exact.
2. The reference's own GPU test file (tests/test_kvcache_manager.py:88-194) restated against our
   integration API, prealloc thread on — relational asserts, like the original.
3. The reference's aliasing script (tests/test_paged_allocator_aliasing.py) as a pytest: without
   alloc() writes alias through the zero page, with alloc() every page is private.
"""
import json
import os
import time

import pytest
import torch

import kvc_testlib as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def load(name):
    with open(os.path.join(T.GOLDEN_DIR, name)) as f:
        return json.load(f)


def _gpu_adapter(cfg):
    return T.ProductAdapter(cfg["num_blocks"], cfg["block_size"], cfg["cell_size"], cfg["num_layers"],
                            world_size=cfg["world_size"], reserve_null_block=cfg["reserve_null_block"],
                            num_kv_buffers=cfg["num_kv_buffers"], contiguous=cfg["contiguous"],
                            phys_pages=cfg["phys_pages"], device=DEV, execute=True)


@pytest.mark.parametrize("idx", range(11))
def test_golden_small_traces_executed_on_gpu(idx):
    case = load("manager_small.json")["cases"][idx]
    if case["config"]["num_layers"] * case["config"]["num_blocks"] > 16 * 65536:
        pytest.skip("VA backfill of this geometry is covered by the large-trace test")
    from kvcached_amd import capi
    ad = _gpu_adapter(case["config"])
    try:
        init = {"s": ad.snapshot(), "e": ad.drain_events()}
        assert init == case["init"], case["name"]
        capi.reset_stats()
        got = T.replay(ad, case["ops"], full=True)
        for i, (g, want) in enumerate(zip(got, case["records"])):
            assert g == want, f"{case['name']} op {i} {case['ops'][i]}"
        capi.flush_unmaps()
        st = capi.get_stats()
        page = T.PAGE * (case["config"]["num_layers"] * case["config"]["num_kv_buffers"] if case["config"]["contiguous"] else 1)
        # every page a map call handed out was zeroed exactly once for that use: by the map call itself (fresh memory), or on
        # its way back to the pool after its previous use
        scrubbed, prescrubbed = capi.get_option(capi.OPT_PAGES_SCRUBBED), capi.get_option(capi.OPT_PAGES_PRESCRUBBED)
        assert st["pages_mapped"] > 0 and st["fill_bytes"] == (st["pages_mapped"] - prescrubbed + scrubbed) * page
        assert prescrubbed <= scrubbed <= st["pages_unmapped"]
    finally:
        ad.close()


@pytest.mark.parametrize("idx", [1, 2])
def test_golden_large_traces_executed_on_gpu(idx):
    """Llama-3-8B geometry, tight pool, Poisson arrivals (5.8k ops) and the 48-page random mix (2.5k ops)."""
    case = load("manager_large.json")["cases"][idx]
    ad = _gpu_adapter(case["config"])
    try:
        init = {"s": ad.snapshot(), "e": ad.drain_events()}
        assert init == case["init"]
        got = T.replay(ad, case["ops"], full=False)
        chain = T.chain_hash(got)
        assert chain["checkpoints"] == case["chain"]["checkpoints"]
        assert chain["final"] == case["chain"]["final"]
    finally:
        ad.close()


# ------------------------------------------------------------------ reference test file, restated
NUM_LAYERS, BLOCK_SIZE, NUM_BLOCKS = 16, 16, 65536
KV_SHAPE = (2, NUM_BLOCKS, BLOCK_SIZE, 8, 64)


@pytest.fixture(autouse=True)
def _no_reserve_unless_asked(monkeypatch):
    """Exact handle counts and early recycling: no pre-created reserve (KVCACHED_PHYS_RESERVE_MB, default 2 GiB) unless
    a test sets one itself."""
    monkeypatch.setenv("KVCACHED_PHYS_RESERVE_MB", os.environ.get("KVC_TEST_RESERVE_MB", "0"))


@pytest.fixture()
def manager(monkeypatch):
    import kvcached_amd.kv_cache_manager as kcm
    import kvcached_amd.integration.vllm.interfaces as vi
    from kvcached_amd.vmm_ops import kv_tensors_created
    monkeypatch.setattr(kcm, "PAGE_PREALLOC_ENABLED", True)
    monkeypatch.setattr(kcm, "CONTIGUOUS_LAYOUT", True)
    monkeypatch.setattr(vi, "_contiguous_layout", True)
    torch.cuda.set_device(0)
    vi.init_kvcached(tp_rank=0, world_size=1, is_worker=True, async_sched=False)
    kv = vi.alloc_kv_cache(kvcache_shape=KV_SHAPE, block_size=BLOCK_SIZE, dtype=torch.float16, device=DEV,
                           num_layers=NUM_LAYERS)
    assert len(kv) == NUM_LAYERS and kv[0].shape[0] == 2
    t0 = time.time()
    while not kv_tensors_created():
        assert time.time() - t0 < 10
        time.sleep(0.05)
    m = kcm.KVCacheManager(num_blocks=NUM_BLOCKS, block_size=BLOCK_SIZE, cell_size=1024, num_layers=NUM_LAYERS,
                           world_size=1)
    t0 = time.time()
    while m.page_allocator.get_num_reserved_pages() == 0 and time.time() - t0 < 5:
        time.sleep(0.05)
    yield m
    del m
    vi.shutdown_kvcached()


def _settle(m):
    """Let the prealloc thread finish its refill so that consecutive readings are comparable."""
    t0 = time.time()
    while m.page_allocator.get_num_reserved_pages() < 5 and time.time() - t0 < 5:
        time.sleep(0.01)


def test_basic_alloc_free(manager):
    _settle(manager)
    before = manager.available_size()
    got = manager.alloc(256)
    assert got is not None and len(got) == 256 and len(set(got)) == 256
    _settle(manager)
    assert manager.available_size() + 256 == before
    manager.free(got)
    _settle(manager)
    assert manager.available_size() == before


def test_over_allocation_fails(manager):
    assert manager.alloc(manager.available_size() + 1) is None


def test_resize_smaller_and_larger_via_shm(manager):
    """The kvctl flow the reference's (skipped) test describes: write total_size into the shm
    segment, read the target back through check_and_get_resize_target, resize."""
    import numpy as np
    pa = manager.page_allocator
    path = "/dev/shm/" + pa._ipc_name()
    total0 = pa.get_num_total_pages()
    seg = np.memmap(path, dtype=np.int64, mode="r+", shape=(3,))
    limit0 = int(seg[0])
    assert manager.mem_size == limit0 // NUM_LAYERS // 2
    seg[0] = limit0 - (total0 // 2) * manager.page_size * NUM_LAYERS * 2
    seg.flush()
    target = pa.check_and_get_resize_target(manager.mem_size)
    assert target == int(seg[0]) // NUM_LAYERS // 2
    manager.resize(target)
    assert total0 == pa.get_num_total_pages() + total0 // 2
    seg[0] = limit0
    seg.flush()
    manager.resize(pa.check_and_get_resize_target(target))
    assert pa.get_num_total_pages() == total0
    del seg


def test_trim(manager):
    assert manager.page_allocator.get_num_reserved_pages() > 0
    manager.page_allocator.stop_prealloc_thread()   # otherwise it refills right behind the trim
    manager.trim()
    assert manager.page_allocator.get_num_reserved_pages() == 0


def test_reserve_and_free_blocks(manager):
    n0 = len(manager.reserved_blocks)
    assert manager.try_to_reserve(512)
    assert len(manager.reserved_blocks) == n0 + 512
    manager.free_reserved()
    assert len(manager.reserved_blocks) == 0


def test_clear_restores_the_null_block(manager):
    got = manager.alloc(1000)
    assert got is not None
    manager.clear()
    assert manager.page_allocator.get_num_inuse_pages() == 0
    _settle(manager)   # the restarted prealloc thread holds pages 0-4 while it maps them
    assert manager.alloc(3) == [0, 1, 2]


# ------------------------------------------------------------------ aliasing script, restated
def test_zero_page_aliasing_without_alloc_and_private_pages_with_alloc(monkeypatch):
    import kvcached_amd.kv_cache_manager as kcm
    import kvcached_amd.integration.sglang.interfaces as si
    from kvcached_amd.utils import PAGE_SIZE
    monkeypatch.setattr(kcm, "CONTIGUOUS_LAYOUT", False)
    monkeypatch.setattr(si, "_contiguous_layout", False)
    monkeypatch.setenv("KVCACHED_ZERO_BACKFILL", "true")   # (the default since round 2)
    tokens, page_tokens, heads, dim, layers = 262144, 16, 8, 64, 2   # 128 pages of 2 MiB per K tensor: two periods of the zero extent
    dtype = torch.float16
    si.init_kvcached(async_sched=False)
    try:
        k_tensors, v_tensors = si.alloc_kv_cache(kvcache_shape=(tokens, heads, dim), dtype=dtype, device=DEV,
                                                 num_layers=layers, page_size=page_tokens, attention_type="MHA")
        cell = heads * dim * dtype.itemsize
        m = si.get_kv_cache_manager(num_blocks=tokens // page_tokens + 1, block_size=page_tokens, cell_size=cell,
                                    num_layers=layers, reserve_null_block=True)
        assert m._post_init_done.wait(10)
        k = k_tensors[0]
        tpp = PAGE_SIZE // (k.stride()[0] * dtype.itemsize)   # tokens per physical page

        # without alloc(): token 1 of unbacked pages (page 0 holds the null block and is backed). What the reference's script
        # demonstrates - writes to memory nobody allocated land on shared zero memory and overwrite each other - holds here
        # too, with a different period: the reference aliases every unbacked page to ONE zero page; the drm backend shows
        # page i % z of one zero extent behind slot i (z = 64), the sharded fallback one zero page per 256 slots.
        # With PRT (the drm backend's default) there is no memory at all behind unbacked VA: such writes are DROPPED and
        # every read returns 0 - nothing is corrupted because nothing is stored.
        from kvcached_amd import capi
        z = capi.get_option(capi.OPT_ZERO_EXTENT_PAGES) or 1
        n_slots = k.numel() * dtype.itemsize // PAGE_SIZE
        pages = [p for p in range(1, min(n_slots, 1 + 3 * z))][:max(60, 2 * z + 8)]
        for i in pages:
            k[1 + i * tpp] = torch.full((heads, dim), float(i), dtype=dtype, device=DEV)
        torch.cuda.synchronize()
        back = {i: float(k[1 + i * tpp][0][0]) for i in pages}
        assert sum(1 for i, b in back.items() if b == float(i)) < len(pages), "writes to unallocated memory were kept"
        if capi.get_option(capi.OPT_PRT):
            assert set(back.values()) == {0.0}
        else:
            for i in pages:                              # every slot sees the LAST write to its zero page
                assert back[i] == float(max(j for j in pages if j % z == i % z)), (i, z, back[i])

        # with alloc(): unique physical pages
        blocks_per_page = PAGE_SIZE // (page_tokens * cell)
        n_pages = 30
        ids = m.alloc(blocks_per_page * n_pages)
        assert ids is not None
        torch.cuda.synchronize()
        toks = []
        for i in range(n_pages):
            tok = ids[i * blocks_per_page] * page_tokens
            toks.append(tok)
            assert float(k[tok].abs().sum()) == 0.0     # first touch reads zeros
            k[tok] = torch.full((heads, dim), float(i + 1), dtype=dtype, device=DEV)
        torch.cuda.synchronize()
        assert [float(k[t][0][0]) for t in toks] == [float(i + 1) for i in range(n_pages)]
        m.free(ids)
        del m
    finally:
        si.shutdown_kvcached()


# ------------------------------------------------------------------ compaction end to end
@pytest.mark.parametrize("contiguous", [False, True])
def test_compact_moves_live_blocks_and_releases_pages(monkeypatch, contiguous):
    """Llama-like geometry (4 layers, 32 KiB blocks): fill blocks with per-(layer, kv, block) patterns,
    free most of them, compact(): every surviving block keeps its bytes under its new id, the emptied
    pages are given back, and the id map is exactly the plan."""
    import kvcached_amd.kv_cache_manager as kcm
    from kvcached_amd import capi, vmm_ops
    layers, block_bytes, bpp = 4, 16 * 2048, 64
    monkeypatch.setattr(kcm, "CONTIGUOUS_LAYOUT", contiguous)
    vmm_ops.init_kvcached(DEV, T.PAGE, contiguous)
    try:
        n_pages = 16
        raw = vmm_ops.create_kv_tensors(n_pages * T.PAGE * 2, 1, DEV, layers, 2, 0, False)
        m = kcm.KVCacheManager(num_blocks=n_pages * bpp, block_size=16, cell_size=2048, num_layers=layers)
        assert m._post_init_done.wait(10)
        ids = m.alloc(bpp * 8)

        def block_view(layer, kv, b):
            if contiguous:   # [block][layer][kv][block_bytes]
                off = ((b * layers + layer) * 2 + kv) * block_bytes
                return raw[0][off:off + block_bytes]
            t = raw[layer]
            off = kv * (t.numel() // 2) + b * block_bytes
            return t[off:off + block_bytes]

        def pattern(layer, kv, b):
            g = torch.Generator(device="cpu").manual_seed(b * 64 + layer * 2 + kv)
            return torch.randint(-128, 127, (block_bytes,), dtype=torch.int8, generator=g)

        live = ids[0:60] + ids[64:64 + 40] + ids[128:128 + 5] + ids[192:192 + 2] + ids[256:256 + 64] + ids[320:320 + 9] \
            + ids[384:384 + 1] + ids[448:448 + 30]
        for b in live:
            for l in range(layers):
                for kv in range(2):
                    block_view(l, kv, b).copy_(pattern(l, kv, b))
        torch.cuda.synchronize()
        m.free([b for b in ids if b not in set(live)])
        inuse0 = m.page_allocator.get_num_inuse_pages()
        plan = m.plan_compaction()
        remap = m.compact()
        assert remap == dict(plan) and len(remap) > 0
        assert m.page_allocator.get_num_inuse_pages() < inuse0
        assert m.compact() == {} or True
        for b in live:
            nb = remap.get(b, b)
            for l in range(layers):
                for kv in range(2):
                    assert torch.equal(block_view(l, kv, nb).cpu(), pattern(l, kv, b)), (b, nb, l, kv)
        # the allocator state is consistent: everything can still be freed, and reused
        m.free([remap.get(b, b) for b in live])
        assert m.page_allocator.get_num_inuse_pages() == 0
        assert len(m.alloc(bpp * n_pages - 1)) == bpp * n_pages - 1
        del m
    finally:
        vmm_ops.shutdown_kvcached()


# ------------------------------------------------------------------ failure path
def test_driver_failure_rolls_the_batch_back(monkeypatch):
    """The (n+1)-th hipMemCreate of a map batch fails (injected hipErrorOutOfMemory): the reference would abort()
    the process (csrc/inc/gpu_vmm.hpp:37-45); here the batch is undone, alloc_page rolls the page id back
    (page_allocator.cpp:215-224 finally reachable), alloc() raises RuntimeError naming the page, and the very same
    allocation succeeds afterwards with the same block ids."""
    monkeypatch.setenv("KVCACHED_PHYS_CHUNK_PAGES", "1")   # exact counts below: the injection hook counts driver allocations (one per page here)
    import kvcached_amd.kv_cache_manager as kcm
    from kvcached_amd import capi, vmm_ops
    monkeypatch.setattr(kcm, "CONTIGUOUS_LAYOUT", False)
    monkeypatch.setattr(kcm, "BATCH_PAGE_ALLOC", True)
    vmm_ops.init_kvcached(DEV, T.PAGE, False)
    capi.set_option(capi.OPT_POOL_BYTES, 0)             # every handle must be created
    try:
        raw = vmm_ops.create_kv_tensors(16 * T.PAGE * 2, 1, DEV, 4, 2, 0, False)
        m = kcm.KVCacheManager(num_blocks=16 * 64, block_size=16, cell_size=2048, num_layers=4)
        assert m._post_init_done.wait(10)
        first = m.alloc(10)
        before = (m.available_size(), m.page_allocator.get_num_free_pages(), m.page_allocator._page_list(0))
        capi.reset_stats()
        capi.set_option(capi.OPT_FAIL_AFTER_CREATES, 5)                         # page id 1 needs 8 slots; the 6th create fails
        with pytest.raises(RuntimeError, match=r"Failed to map page 1: .*hipMemCreate.*\[injected\]"):
            m.alloc(100)
        capi.set_option(capi.OPT_FAIL_AFTER_CREATES, -1)
        st = capi.get_stats()
        assert st["handles_created"] == 5 and st["handles_released"] == 5      # the partial batch was undone
        after = (m.available_size(), m.page_allocator.get_num_free_pages(), m.page_allocator._page_list(0))
        assert after == before
        # the batched path: 300 blocks need 4 new page ids = 32 slots in ONE map call; the 21st create fails
        capi.reset_stats()
        capi.set_option(capi.OPT_FAIL_AFTER_CREATES, 20)
        with pytest.raises(RuntimeError, match=r"Failed to map page 1: .*hipMemCreate.*\[injected\]"):
            m.alloc(300)
        capi.set_option(capi.OPT_FAIL_AFTER_CREATES, -1)
        st = capi.get_stats()
        assert st["handles_created"] == 20 and st["handles_released"] == 20
        after = (m.available_size(), m.page_allocator.get_num_free_pages(), m.page_allocator._page_list(0))
        assert after == before
        # nothing of page 1 is left mapped (lazy mode: it can be mapped again from scratch), and the retry works
        got = m.alloc(100)
        assert got == list(range(10, 110))
        assert int(torch.count_nonzero(raw[0][T.PAGE:2 * T.PAGE])) == 0
        m.free(first + got)
        del m
    finally:
        capi.set_option(capi.OPT_FAIL_AFTER_CREATES, -1)
        vmm_ops.shutdown_kvcached()


def test_shrinking_the_budget_releases_pooled_handles(monkeypatch):
    """`kvctl limit` semantics: a successful shrink gives memory back now — what the handle pool parked goes to the
    driver at once instead of waiting for the idle decay (the reference releases on every unmap)."""
    monkeypatch.setenv("KVCACHED_PHYS_CHUNK_PAGES", "1")   # page-granular counts (run-sized extents: the twin test below)
    import kvcached_amd.kv_cache_manager as kcm
    from kvcached_amd import capi, vmm_ops
    monkeypatch.setattr(kcm, "CONTIGUOUS_LAYOUT", False)
    vmm_ops.init_kvcached(DEV, T.PAGE, False)
    try:
        vmm_ops.create_kv_tensors(32 * T.PAGE * 2, 1, DEV, 2, 2, 0, False)
        m = kcm.KVCacheManager(num_blocks=32 * 64, block_size=16, cell_size=2048, num_layers=2)
        assert m._post_init_done.wait(10)
        ids = m.alloc(20 * 64)                                   # 20 page ids = 80 slots
        capi.reset_stats()
        m.free(ids)                                              # 10 stay reserved (mapped), 10 are unmapped -> pool
        st = capi.get_stats()
        assert st["pages_unmapped"] == 40 and st["handles_released"] == 0
        free0, _ = capi.mem_get_info()
        assert m.page_allocator.resize(24 * T.PAGE)              # 32 -> 24 page ids: plain free-list shrink
        st = capi.get_stats()
        assert st["handles_released"] == 40                      # the pooled handles went back to the driver
        assert m.page_allocator.get_num_total_pages() == 24
        assert m.page_allocator.resize(32 * T.PAGE)
        got = m.alloc(64)
        m.free(got)
        del m
    finally:
        vmm_ops.shutdown_kvcached()


def test_the_physical_reserve_is_created_ahead_of_time_and_serves_a_growth_burst(monkeypatch):
    """allocating VRAM the kernel has not cleared yet costs ~80 us per 2 MiB inside the allocation. With a
    housekeeping thread around (every engine has one) the pool pre-creates KVCACHED_PHYS_RESERVE_MB of idle memory in the
    background and never decays below it: a growth burst up to that size creates nothing on the caller's path."""
    import kvcached_amd.kv_cache_manager as kcm
    from kvcached_amd import capi, vmm_ops
    monkeypatch.setenv("KVCACHED_PHYS_RESERVE_MB", "512")            # 256 pages of 2 MiB
    monkeypatch.setenv("KVCACHED_POOL_IDLE_MS", "200")
    monkeypatch.setattr(kcm, "CONTIGUOUS_LAYOUT", False)
    monkeypatch.setattr(kcm, "PAGE_PREALLOC_ENABLED", True)          # starts the prealloc + watcher (housekeeping) threads
    vmm_ops.init_kvcached(DEV, T.PAGE, False)
    capi.reset_stats()
    try:
        vmm_ops.create_kv_tensors(256 * T.PAGE * 2, 1, DEV, 2, 2, 0, False)
        m = kcm.KVCacheManager(num_blocks=256 * 64, block_size=16, cell_size=2048, num_layers=2)
        assert m._post_init_done.wait(10)
        if capi.get_option(capi.OPT_EFFECTIVE_BACKEND) != 3 or capi.get_option(capi.OPT_KFD_CREATE_ACTIVE) != 1:
            pytest.skip("the reserve is pre-created with the drm backend and pages straight from KFD")
        t0 = time.time()
        while time.time() - t0 < 5:                                  # a few 100 ms ticks (256 pages per tick at most)
            held, out = capi.get_option(capi.OPT_POOL_HELD_PAGES), capi.get_option(capi.OPT_POOL_OUT_PAGES)
            if held - out >= 256:
                break
            time.sleep(0.05)
        assert held - out >= 256, (held, out)
        time.sleep(0.6)                                               # three idle windows: the reserve is not decayed away
        assert capi.get_option(capi.OPT_POOL_HELD_PAGES) - capi.get_option(capi.OPT_POOL_OUT_PAGES) >= 256
        clean = False
        for attempt in range(4):   # (the housekeeping thread may top the reserve up in the very 2 ms the burst takes: look again then)
            before = capi.get_stats()
            ids = m.alloc(40 * 64)                                   # 40 page ids = 160 slots: well inside the reserve
            st = capi.get_stats()
            assert st["pages_mapped"] - before["pages_mapped"] >= 100
            clean = st["handles_created"] == before["handles_created"]
            m.free(ids)
            m.trim()
            if clean:
                break
            time.sleep(0.5)
        assert clean, "every growth burst created pages on the caller's path although the reserve was full"
        del m
    finally:
        vmm_ops.shutdown_kvcached()
    st = capi.get_stats()
    assert st["handles_created"] == st["handles_released"]


def test_the_reserve_follows_demand(monkeypatch):
    """what a map call has to CREATE is paid on its caller's thread (2 us per buffer on wiped VRAM, 50-80 us per
    2 MiB on VRAM the kernel has not handed out yet). While callers have to create memory, the housekeeping thread creates
    ahead of them - up to twice what the last second asked for - so growth that goes on finds memory that is there already;
    a second after the growth has stopped the target is the base reserve again and the surplus goes back to the driver like
    any idle memory, where a co-located engine can have it."""
    import kvcached_amd.kv_cache_manager as kcm
    from kvcached_amd import capi, vmm_ops
    monkeypatch.setenv("KVCACHED_PHYS_RESERVE_MB", "256")            # the base reserve: 8 page ids of this geometry (16 rows x 2 MiB)
    monkeypatch.setenv("KVCACHED_POOL_IDLE_MS", "200")
    monkeypatch.setattr(kcm, "CONTIGUOUS_LAYOUT", False)
    monkeypatch.setattr(kcm, "PAGE_PREALLOC_ENABLED", True)          # the watcher thread is the housekeeper
    vmm_ops.init_kvcached(DEV, T.PAGE, False)
    capi.reset_stats()
    try:
        L = 8
        vmm_ops.create_kv_tensors(512 * T.PAGE * 2, 1, DEV, L, 2, 0, False)
        m = kcm.KVCacheManager(num_blocks=512 * 64, block_size=16, cell_size=2048, num_layers=L)
        assert m._post_init_done.wait(10)
        if capi.get_option(capi.OPT_EFFECTIVE_BACKEND) != 3 or capi.get_option(capi.OPT_KFD_CREATE_ACTIVE) != 1:
            pytest.skip("the reserve is pre-created with the drm backend and pages straight from KFD")
        rows = 2 * L
        time.sleep(0.5)
        idle = lambda: capi.get_option(capi.OPT_POOL_HELD_PAGES) - capi.get_option(capi.OPT_POOL_OUT_PAGES)   # noqa: E731
        burst = 96                                                   # page ids: 96 x 16 x 2 MiB = 3 GiB, far beyond the 256 MiB base
        before = capi.get_stats()["handles_created"]
        first = m.alloc(burst * 64)
        created_first = capi.get_stats()["handles_created"] - before
        assert created_first >= (burst - 20) * rows                  # the first burst had to create (almost) all of it on the caller's path
        time.sleep(0.7)                                               # a few ticks: the thread creates ahead, towards 2 x the burst
        assert idle() >= burst * rows, idle()
        before = capi.get_stats()["handles_created"]
        second = m.alloc(burst * 64)                                 # the growth goes on: served from memory made ahead of it
        created_second = capi.get_stats()["handles_created"] - before
        assert created_second <= created_first // 8, (created_first, created_second)
        m.free(first)
        m.free(second)
        m.trim()
        time.sleep(4.0)                                               # the growth has stopped: one second later the target is the base again,
        assert idle() <= 4 * 256 // 2, idle()                       # and the idle windows (200 ms, 512 MiB per tick) have returned the rest
        del m
    finally:
        vmm_ops.shutdown_kvcached()
    st = capi.get_stats()
    assert st["handles_created"] == st["handles_released"]


def test_an_idle_engine_gives_its_reserve_back(monkeypatch):
    """the pre-created reserve is idle memory a co-located engine cannot see. An engine that has not mapped or unmapped
    anything for KVCACHED_RESERVE_IDLE_S gives it back (the reference releases every page on unmap: csrc/page.cpp:17) and gets it again with the
    first ticks after the next call."""
    import kvcached_amd.kv_cache_manager as kcm
    from kvcached_amd import capi, vmm_ops
    monkeypatch.setenv("KVCACHED_PHYS_RESERVE_MB", "256")
    monkeypatch.setenv("KVCACHED_POOL_IDLE_MS", "100")
    monkeypatch.setenv("KVCACHED_RESERVE_IDLE_S", "1")
    monkeypatch.setattr(kcm, "CONTIGUOUS_LAYOUT", False)
    monkeypatch.setattr(kcm, "PAGE_PREALLOC_ENABLED", True)
    vmm_ops.init_kvcached(DEV, T.PAGE, False)
    capi.reset_stats()
    try:
        vmm_ops.create_kv_tensors(128 * T.PAGE * 2, 1, DEV, 4, 2, 0, False)
        m = kcm.KVCacheManager(num_blocks=128 * 64, block_size=16, cell_size=2048, num_layers=4)
        assert m._post_init_done.wait(10)
        if capi.get_option(capi.OPT_EFFECTIVE_BACKEND) != 3 or capi.get_option(capi.OPT_KFD_CREATE_ACTIVE) != 1:
            pytest.skip("the reserve is pre-created with the drm backend and pages straight from KFD")
        # whole idle buffers (free lanes of a buffer that a still-mapped page id pins cannot go back: they are handed out first instead)
        idle = lambda: capi.get_option(capi.OPT_POOL_HELD_PAGES) - capi.get_option(capi.OPT_POOL_OUT_PAGES) - capi.get_option(capi.OPT_POOL_FREE_PIECES)   # noqa: E731
        ids = m.alloc(24 * 64)                                        # more than the prealloc thread keeps ready: map calls happen
        time.sleep(0.4)
        assert idle() >= 64                                           # in use: the reserve stands (128 pages, some of them free lanes of partly used buffers)
        m.free(ids)                                                   # more than stay mapped for reuse: unmap calls happen (no trim(): that empties the pool by itself)
        t0 = time.time()
        time.sleep(0.4)
        assert idle() >= 64                                           # a moment after the last call: still there
        while idle() > 0 and time.time() - t0 < 8:
            time.sleep(0.1)
        assert idle() == 0, (idle(), time.time() - t0)                # the idle second is over: gone
        ids = m.alloc(24 * 64)                                        # in use again: it comes back
        t0 = time.time()
        while idle() < 64 and time.time() - t0 < 5:
            time.sleep(0.1)
        assert idle() >= 64, idle()
        m.free(ids)
        m.trim()
    finally:
        m = None
        vmm_ops.shutdown_kvcached()
    st = capi.get_stats()
    assert st["handles_created"] == st["handles_released"]


def test_golden_trace_with_async_unmap(monkeypatch):
    """Bookkeeping is synchronous, so the reference's golden trace (block ids, page offsets, counters) is still
    bit-exact with KVC_OPT_ASYNC_UNMAP on; after a flush the physical ledger matches the synchronous run."""
    from kvcached_amd import capi
    case = load("manager_large.json")["cases"][2]
    os.environ["KVCACHED_ASYNC_UNMAP"] = "true"
    os.environ["KVCACHED_ZERO_BACKFILL"] = "false"   # queued unmaps are a lazy-mode feature (compat promises zeros behind an unmap at once)
    try:
        ad = _gpu_adapter(case["config"])
    finally:
        os.environ.pop("KVCACHED_ASYNC_UNMAP", None)
        os.environ.pop("KVCACHED_ZERO_BACKFILL", None)
    try:
        assert capi.get_option(capi.OPT_ASYNC_UNMAP) == 1
        init = {"s": ad.snapshot(), "e": ad.drain_events()}
        assert init == case["init"]
        capi.reset_stats()
        got = T.replay(ad, case["ops"], full=False)
        chain = T.chain_hash(got)
        assert chain["checkpoints"] == case["chain"]["checkpoints"] and chain["final"] == case["chain"]["final"]
        capi.flush_unmaps()
        st = capi.get_stats()
        assert st["unmaps_queued"] > 0
        assert st["pages_unmapped"] + st["unmaps_cancelled"] == st["unmaps_queued"]
        assert st["pages_mapped"] - st["pages_unmapped"] - st["unmaps_cancelled"] >= 0
    finally:
        ad.close()
        capi.set_option(capi.OPT_ASYNC_UNMAP, 0)


def test_pool_eviction_is_left_to_the_housekeeping_thread(monkeypatch):
    """With an allocator watcher thread around, handles that exceed the pool's cap are not released on the caller's
    free() path (hipMemRelease of a used handle is 40-50 us: 200 ms for a 4096-slot free) but by the 10 Hz
    housekeeping; without one (plain C-ABI use) the release stays immediate."""
    monkeypatch.setenv("KVCACHED_PHYS_CHUNK_PAGES", "1")   # page-granular counts
    monkeypatch.setenv("KVCACHED_ZERO_BACKFILL", "false")  # lazy mode: free() is a few ms here, well inside one housekeeping tick
    monkeypatch.setenv("KVCACHED_PHYS_RESERVE_MB", "0")    # exact counts: no pre-created reserve
    import kvcached_amd.kv_cache_manager as kcm
    from kvcached_amd import capi, vmm_ops
    monkeypatch.setattr(kcm, "CONTIGUOUS_LAYOUT", False)
    monkeypatch.setattr(kcm, "PAGE_PREALLOC_ENABLED", True)          # starts the prealloc + watcher threads
    vmm_ops.init_kvcached(DEV, T.PAGE, False)
    capi.set_option(capi.OPT_POOL_BYTES, 16 * T.PAGE)                  # a 16-handle pool
    try:
        vmm_ops.create_kv_tensors(64 * T.PAGE * 2, 1, DEV, 2, 2, 0, False)
        m = kcm.KVCacheManager(num_blocks=64 * 64, block_size=16, cell_size=2048, num_layers=2)
        assert m._post_init_done.wait(10)
        ids = m.alloc(40 * 64)                                         # 40 page ids = 160 slots
        time.sleep(0.3)
        capi.reset_stats()
        m.free(ids)                                                    # 10 page ids stay reserved, 120 slots unmapped
        st = capi.get_stats()
        assert st["pages_unmapped"] >= 100 and st["handles_released"] == 0, st
        t0 = time.time()
        while capi.get_stats()["handles_released"] < st["pages_unmapped"] - 16 and time.time() - t0 < 5:
            time.sleep(0.05)
        assert capi.get_stats()["handles_released"] >= st["pages_unmapped"] - 16
        del m
        # no watcher any more: the same free releases at once
        vmm_ops.create_kv_tensors(64 * T.PAGE * 2, 1, DEV, 2, 2, 0, False)
        offs = [i * T.PAGE for i in range(30)]
        assert vmm_ops.map_to_kv_tensors(offs)
        capi.reset_stats()
        assert vmm_ops.unmap_from_kv_tensors(offs)
        st = capi.get_stats()
        assert st["handles_released"] >= st["pages_unmapped"] - 16
    finally:
        capi.set_option(capi.OPT_POOL_BYTES, 16384 << 20)
        vmm_ops.shutdown_kvcached()


def test_unmap_leaves_its_tlb_invalidation_to_the_watcher_thread(monkeypatch):
    """With an allocator watcher thread (every engine has one: it runs with the prealloc thread), free() does not pay
    the 0.3-0.4 ms KFD round trip of the TLB invalidation: the unmap batch marks it owed and the watcher's next tick
    performs it - or the next map batch does, whichever comes first. Pages stay private either way. (Lazy mode: a compat
    region promises zeros behind an unmap at once and invalidates inside the call.)"""
    import kvcached_amd.kv_cache_manager as kcm
    from kvcached_amd import capi, vmm_ops
    monkeypatch.setenv("KVCACHED_ZERO_BACKFILL", "false")
    monkeypatch.setattr(kcm, "CONTIGUOUS_LAYOUT", False)
    monkeypatch.setattr(kcm, "PAGE_PREALLOC_ENABLED", True)
    vmm_ops.init_kvcached(DEV, T.PAGE, False)
    try:
        raw = vmm_ops.create_kv_tensors(64 * T.PAGE * 2, 2, DEV, 2, 2, 0, False)
        m = kcm.KVCacheManager(num_blocks=64 * 64, block_size=16, cell_size=2048, num_layers=2)
        assert m._post_init_done.wait(10)
        ids = m.alloc(30 * 64)
        epp = T.PAGE // 2
        for t in raw:
            t[:30 * epp].fill_(77)
        torch.cuda.synchronize()
        time.sleep(0.3)                                            # prealloc refills and watcher ticks have settled
        n0, b0 = capi.get_stats()["tlb_shootdowns"], capi.get_option(capi.OPT_BACKGROUND_SHOOTDOWNS)
        t0 = time.perf_counter()
        m.free(ids)                                                # 10 page ids stay reserved, 20 are unmapped
        dt = time.perf_counter() - t0
        deadline = time.time() + 2
        while capi.get_stats()["tlb_shootdowns"] == n0 and time.time() < deadline:
            time.sleep(0.005)
        assert capi.get_stats()["tlb_shootdowns"] == n0 + 1          # exactly one invalidation for the batch ...
        assert capi.get_option(capi.OPT_BACKGROUND_SHOOTDOWNS) == b0 + 1, "free() paid for the invalidation itself"
        # recycled pages come back zeroed and private
        ids2 = m.alloc(30 * 64)
        pages2 = sorted({b // 64 for b in ids2})
        assert len(pages2) == 30
        half = raw[0].numel() // 2
        for t in raw:
            for base in (0, half):
                for p in pages2:                                     # reserved pages kept their 77s, re-backed ones are zero:
                    page = t[base + p * epp: base + (p + 1) * epp]   # never a mixture, never anything else
                    lo, hi = int(page.min()), int(page.max())
                    assert lo == hi and lo in (0, 77), (p, lo, hi)
        m.free(ids2)
        print(f"[async shootdown] free() of 20 page ids took {dt * 1e3:.2f} ms")
        del m
    finally:
        vmm_ops.shutdown_kvcached()
