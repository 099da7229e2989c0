"""HostBlockStore, KVCacheManager.offload_to / .restore_from and the host tier of ElasticBlockPool's prefix cache, host side
(the "cpu" device and fakes): the free list, the refusals that leave everything unchanged, and the pool's bookkeeping over
an in-memory store that records its calls. The bytes are checked on the MI355X (tests/test_gpu_host_store.py)."""
import ctypes
from unittest import mock

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
    return (m.available_size(), pa.get_num_inuse_pages(), pages, sorted(m.full_pages), m.num_avail_blocks)


# ------------------------------------------------------------------ the store and the two manager methods
def test_free_list_hands_out_the_lowest_slot_first(cpu_ops):
    ops, capi = cpu_ops
    from kvcached_amd.host_store import HostBlockStore
    m = _manager(ops)
    store = HostBlockStore(m, 6)
    assert store.geometry == (0, False, 4, 32 * 1024) and store.record_bytes == 32 * 1024
    assert store.data.numel() == 6 * 4 * 32 * 1024 and store.data.dtype == torch.uint8
    assert (len(store), store.free_slots) == (0, 6)
    assert store._take(3) == [0, 1, 2] and (len(store), store.free_slots) == (3, 3)
    store.free([1])
    assert store._take(2) == [1, 3]
    store.free([3, 0])
    assert store._take(1) == [0]
    assert store._take(4) is None and (len(store), store.free_slots) == (3, 3)     # full: None, nothing changed
    assert store._take(3) == [3, 4, 5] and store._take(1) is None
    for bad in ([6], [-1], [2, 2]):                                                 # foreign slots, a slot twice
        with pytest.raises(ValueError):
            store.free(bad)
        assert len(store) == 6
    store.free([4])
    with pytest.raises(ValueError):
        store.free([4])                                                             # double free
    with pytest.raises(ValueError):
        store.free([5, 4])                                                          # refused as a whole
    assert (len(store), store.free_slots) == (5, 1)
    store.release()
    assert store.data is None
    with pytest.raises(ValueError):
        store._take(1)


def test_store_sizes_follow_the_codec(cpu_ops):
    ops, capi = cpu_ops
    from kvcached_amd.host_store import HostBlockStore
    m = _manager(ops)
    store = HostBlockStore(m, 3, codec="mxfp8", dtype=torch.bfloat16)
    assert store.codec_id == capi.KVC_CODEC_MXFP8_BF16 and store.record_bytes == 16 * 1024 + 512
    assert store.data.numel() == 3 * 4 * store.record_bytes
    for kw in (dict(codec="mxfp8"), dict(codec="zip", dtype=torch.bfloat16), dict(dtype=torch.float16)):
        with pytest.raises(ValueError):
            HostBlockStore(m, 3, **kw)
    with pytest.raises(ValueError):
        HostBlockStore(m, 0)


def test_c_entries_refuse_the_cpu_device(cpu_ops):
    ops, capi = cpu_ops
    ops.create_kv_tensors(16 * PAGE * 2, 1, "cpu", 2, 2, 0, False)
    buf = (ctypes.c_char * (1 << 16))()
    ids, slots = capi.i64_array([0, 1]), capi.i64_array([3, 1])
    for codec in (0, capi.KVC_CODEC_MXFP8_BF16, capi.KVC_CODEC_MXFP8_F16):
        assert capi.lib.kvc_copy_blocks_to_host_slots(0, ids, slots, 2, 1024, codec, ctypes.addressof(buf), 4, None,
                                                      1) == capi.KVC_E_NO_GPU
        assert capi.lib.kvc_copy_blocks_from_host_slots(0, ids, slots, 2, 1024, codec, ctypes.addressof(buf), 4, None,
                                                        1) == capi.KVC_E_NO_GPU
    with pytest.raises(capi.KvcError) as e:
        capi.copy_blocks_to_host_slots(0, [0], [0], 16, 0, ctypes.addressof(buf), 1)
    assert e.value.code == capi.KVC_E_NO_GPU
    with pytest.raises(ValueError):
        capi.copy_blocks_from_host_slots(0, [0, 1], [0], 16, 0, ctypes.addressof(buf), 1)


def test_offload_to_whose_copy_fails_changes_nothing(cpu_ops):
    """No GPU: the library refuses the copy; the blocks are still allocated and the slots are back."""
    ops, capi = cpu_ops
    from kvcached_amd.host_store import HostBlockStore
    m = _manager(ops, reserve_null_block=True)
    store = HostBlockStore(m, 8)
    ids = m.alloc(BPP + 7)
    assert store._take(2) == [0, 1]
    before = _state(m)
    with pytest.raises(capi.KvcError) as e:
        m.offload_to(store, ids[:5])
    assert e.value.code == capi.KVC_E_NO_GPU
    assert _state(m) == before and (len(store), store.free_slots) == (2, 6)
    assert store._take(1) == [2]                           # the lowest slot again
    # what offload() refuses is refused before a slot is taken
    for bad in ([], [ids[0], ids[0]], [0], [15 * BPP + 3], [-1]):
        with pytest.raises(ValueError):
            m.offload_to(store, bad)
        assert _state(m) == before and len(store) == 3
    assert m.offload_to(store, ids[:6]) is None            # 5 free slots: None, nothing changed
    assert _state(m) == before and len(store) == 3
    m.free(ids)                                            # every one of them is still allocated
    assert m.page_allocator.get_num_inuse_pages() == 1     # (the null block's page)


def test_restore_from_refusals(cpu_ops):
    ops, capi = cpu_ops
    from kvcached_amd.host_store import HostBlockStore
    m = _manager(ops)
    store = HostBlockStore(m, 4)
    assert store._take(2) == [0, 1]
    before = _state(m)
    for bad in ([2], [0, 4], [-1], []):                    # not in use, outside the arena, none at all
        with pytest.raises(ValueError):
            m.restore_from(store, bad)
        assert _state(m) == before and len(store) == 2
    for geometry in ((1, False, 4, 32 * 1024), (0, True, 4, 32 * 1024), (0, False, 2, 32 * 1024), (0, False, 4, 16 * 1024)):
        with mock.patch.object(store, "geometry", geometry):
            with pytest.raises(ValueError, match="geometry"):
                m.restore_from(store, [0])
            with pytest.raises(ValueError, match="geometry"):
                m.offload_to(store, [0])
        assert _state(m) == before and len(store) == 2
    # the copy fails (no GPU): the blocks it took are given back, the slots stay in use
    with pytest.raises(capi.KvcError):
        m.restore_from(store, [1, 0, 1])
    assert m.available_size() == before[0] and m.page_allocator.get_num_inuse_pages() == 0 and len(store) == 2
    store.release()
    with pytest.raises(ValueError, match="released"):
        m.restore_from(store, [0])


def test_host_store_refuses_tensor_parallel_managers(cpu_ops):
    ops, capi = cpu_ops
    from kvcached_amd.host_store import HostBlockStore
    m = _manager(ops)
    store = HostBlockStore(m, 4)
    ids = m.alloc(3)
    store._take(1)
    with mock.patch.object(m, "_kv_remote", True):
        with pytest.raises(RuntimeError, match="tensor parallelism"):
            m.offload_to(store, ids)
        with pytest.raises(RuntimeError):
            m.restore_from(store, [0])
    assert len(store) == 1
    m.free(ids)


# ------------------------------------------------------------------ the pool over a store that records its calls
class FakeStore:
    """The three operations of a store over a FifoBlockManager: offload frees the blocks and remembers what they "held"
    (their ids, standing in for the bytes), restore allocates new ones. Lowest free slot first, as HostBlockStore."""

    def __init__(self, manager, capacity, fail=False):
        self.manager, self.capacity, self.fail = manager, capacity, fail
        self.slots = {}          # slot -> id of the block whose bytes it holds
        self.restored = {}       # new block id -> id of the block whose bytes it got
        self.calls = []

    def offload(self, block_ids):
        self.calls.append(("offload", list(block_ids)))
        if self.fail:
            raise RuntimeError("the link is down")
        free = [s for s in range(self.capacity) if s not in self.slots][:len(block_ids)]
        if len(free) < len(block_ids):
            return None
        self.slots.update(zip(free, block_ids))
        self.manager.free(list(block_ids))
        return free

    def restore(self, slots, wait=False):
        self.calls.append(("restore", list(slots), wait))
        assert all(s in self.slots for s in slots)
        ids = self.manager.alloc(len(slots))
        if ids is not None:
            self.restored.update(zip(ids, (self.slots[s] for s in slots)))
        return ids

    def free(self, slots):
        self.calls.append(("free", list(slots)))
        for s in slots:
            del self.slots[s]


def _pool(num_blocks, host_cache_blocks, capacity=None, fail=False, with_store=True, **kw):
    from kvcached_amd.integration.vllm.block_pool import build_elastic_block_pool
    manager = T.FifoBlockManager(num_blocks)
    store = FakeStore(manager, capacity if capacity is not None else host_cache_blocks, fail) if with_store else None
    cls = build_elastic_block_pool(T.FakeBlockPool, T.FakeKVCacheBlock)
    with mock.patch("kvcached_amd.integration.vllm.interfaces.get_kv_cache_manager", return_value=manager):
        pool = cls(num_gpu_blocks=num_blocks, block_size=16, cell_size=1024, num_layers=1, enable_caching=True,
                   max_cached_blocks=kw.pop("max_cached_blocks", 1000), host_cache_blocks=host_cache_blocks, host_store=store,
                   **kw)
    return pool, manager, store


def _cache(pool, hashes, group=0):
    """Allocate, register under `hashes`, release: the blocks end up cached and evictable, oldest first."""
    blocks = pool.get_new_blocks(len(hashes))
    pool.cache_full_blocks(T.FakeRequest(hashes), blocks, 0, len(hashes), 16, group)
    pool.free_blocks(blocks)
    return [b.block_id for b in blocks]


def test_a_hit_after_eviction_comes_back_under_its_key():
    from kvcached_amd.integration.vllm.block_pool import make_cache_key
    pool, manager, store = _pool(8, 4)                    # block 0 is the null block: 7 to hand out
    ids = _cache(pool, [b"a", b"b", b"c"])
    assert ids == [1, 2, 3] and pool.get_num_free_blocks() == 7
    held = pool.get_new_blocks(6)                         # 4 free + the two oldest evictable ones
    assert store.calls == [("offload", [1, 2])] and store.slots == {0: 1, 1: 2}
    assert list(pool._host_lru) == [make_cache_key(b"a", 0), make_cache_key(b"b", 0)]
    assert pool.get_num_free_blocks() == 1 and pool.get_usage() == 1.0 - 1 / 8     # host entries are not counted
    assert pool.get_cached_block(b"c", [0])[0].block_id == 3
    # no room and nothing to evict but... block 3 is evictable and not a hit of this lookup: it spills to make room
    hit = pool.get_cached_block(b"a", [0])
    assert hit is not None and len(hit) == 1
    blk = hit[0]
    assert store.restored[blk.block_id] == 1              # the bytes of the block that was cached under b"a"
    assert pool._cached_blocks[make_cache_key(b"a", 0)] is blk and pool._block_id_to_key[blk.block_id] == make_cache_key(b"a", 0)
    assert blk.ref_cnt == 0 and blk.block_id in pool._evictable_blocks
    assert make_cache_key(b"a", 0) not in pool._host_lru and make_cache_key(b"c", 0) in pool._host_lru
    assert ("restore", [0], True) in store.calls and store.calls[-1] == ("free", [0])
    assert pool.get_cached_block(b"a", [0])[0] is blk     # now a GPU hit: no further store call
    assert store.calls[-1] == ("free", [0])
    pool.touch(hit)
    assert blk.ref_cnt == 1 and blk.block_id not in pool._evictable_blocks
    pool.free_blocks(held + hit)


def test_old_call_form_looks_on_the_host_too():
    pool, manager, store = _pool(8, 4)
    _cache(pool, [b"a"])
    held = pool.get_new_blocks(7)
    assert store.slots == {0: 1}
    assert pool.get_cached_block(b"a") is None            # the pool is full and nothing is evictable: a miss
    assert [c[0] for c in store.calls] == ["offload"]
    pool.free_blocks(held[:1])
    blk = pool.get_cached_block(b"a")
    assert blk is not None and store.restored[blk.block_id] == 1 and not store.slots


def test_host_lru_drops_its_oldest_entries_at_capacity():
    from kvcached_amd.integration.vllm.block_pool import make_cache_key
    pool, manager, store = _pool(8, 3)
    _cache(pool, [b"a", b"b"])
    held = pool.get_new_blocks(7)                          # evicts a, b
    assert sorted(store.slots.values()) == [1, 2]
    pool.free_blocks(held)
    _cache(pool, [b"c", b"d"])
    held = pool.get_new_blocks(7)                          # evicts c, d: a has to go
    assert [k[:-4] for k in pool._host_lru] == [b"b", b"c", b"d"] and len(store.slots) == 3
    assert ("free", [0]) in store.calls                    # a's slot, before the offload that reuses it
    assert store.calls.index(("free", [0])) < len(store.calls) - 1 and store.calls[-1][0] == "offload"
    assert pool.get_cached_block(b"a", [0]) is None
    pool.free_blocks(held)
    assert make_cache_key(b"b", 0) in pool._host_lru


def test_victims_beyond_the_capacity_are_freed():
    pool, manager, store = _pool(8, 2)
    ids = _cache(pool, [b"a", b"b", b"c", b"d", b"e"])
    assert ids == [1, 2, 3, 4, 5]
    pool.get_new_blocks(7)                                 # all five are evicted in one go; the youngest two are spilled
    assert store.calls == [("offload", [4, 5])]
    assert [k[:-4] for k in pool._host_lru] == [b"d", b"e"]
    assert manager.available_size() == 0 and pool.get_num_free_blocks() == 0


def test_uncached_victims_are_never_spilled():
    pool, manager, store = _pool(8, 4)
    ids = _cache(pool, [b"a", b"b"])
    pool.evict_blocks([ids[0]])                            # by block id: gone from the GPU index, freed, not spilled
    assert store.calls == [] and manager.available_size() == 6
    pool.get_new_blocks(7)
    assert store.calls == [("offload", [2])]
    pool.evict_blocks([2])                                 # leaves the host entry alone
    assert len(pool._host_lru) == 1


def test_lookup_over_two_groups_is_all_or_nothing():
    pool, manager, store = _pool(8, 4)
    _cache(pool, [b"a"], group=0)
    held = pool.get_new_blocks(6)                          # leaves one free block, and a/0 still on the GPU
    pool.free_blocks(held[:1])
    more = pool.get_new_blocks(2)                          # evicts a/0 to the host
    assert store.calls == [("offload", [1])]
    n_calls, free = len(store.calls), manager.available_size()
    lru, cached, evictable = list(pool._host_lru.items()), dict(pool._cached_blocks), list(pool._evictable_blocks)
    assert pool.get_cached_block(b"a", [0, 1]) is None     # group 1 is nowhere: no store call, nothing changed
    assert len(store.calls) == n_calls and manager.available_size() == free
    assert (list(pool._host_lru.items()), dict(pool._cached_blocks), list(pool._evictable_blocks)) == (lru, cached, evictable)
    assert pool.get_cached_block(b"zz", [0]) is None and len(store.calls) == n_calls
    pool.free_blocks(more + held[1:])


def test_a_lookup_never_evicts_its_own_hits():
    from kvcached_amd.integration.vllm.block_pool import make_cache_key
    pool, manager, store = _pool(8, 4)
    _cache(pool, [b"h"], group=1)                          # block 1: will go to the host
    held = pool.get_new_blocks(7)
    pool.free_blocks(held)
    assert store.slots == {0: 1}
    g0 = _cache(pool, [b"h"], group=0)                     # the same hash in group 0: stays on the GPU, the OLDEST evictable
    younger = _cache(pool, [b"y"])
    held = pool.get_new_blocks(manager.available_size())   # no free block left; evictable: g0 (oldest), younger
    assert manager.available_size() == 0 and list(pool._evictable_blocks) == g0 + younger
    hit = pool.get_cached_block(b"h", [0, 1])
    assert hit is not None and hit[0].block_id == g0[0]    # not evicted, although it was the oldest
    assert store.restored[hit[1].block_id] == 1
    assert make_cache_key(b"y", 0) in pool._host_lru       # the younger block made the room
    assert pool._cached_blocks[make_cache_key(b"h", 0)] is hit[0] and pool._cached_blocks[make_cache_key(b"h", 1)] is hit[1]
    # both groups on the GPU and both evictable, but the pool is full: a host hit with nothing else to evict is a miss
    pool.touch(hit)
    _ = held
    pool2, manager2, store2 = _pool(4, 4)
    _cache(pool2, [b"k"], group=1)
    h2 = pool2.get_new_blocks(3)
    pool2.free_blocks(h2[:1])
    only = _cache(pool2, [b"k"], group=0)
    assert manager2.available_size() == 0 and list(pool2._evictable_blocks) == only
    before = (list(pool2._host_lru.items()), dict(pool2._cached_blocks), len(store2.calls))
    assert pool2.get_cached_block(b"k", [0, 1]) is None
    assert (list(pool2._host_lru.items()), dict(pool2._cached_blocks), len(store2.calls)) == before


def test_promotion_keeps_its_entries_while_room_is_made():
    """Capacity 1: the victim that makes room spills into a full store, which must not drop the entry being promoted."""
    pool, manager, store = _pool(4, 1)
    _cache(pool, [b"a"])
    held = pool.get_new_blocks(3)
    assert store.slots == {0: 1}
    pool.free_blocks(held[:1])
    _cache(pool, [b"b"])                                   # takes the free block: evictable, pool full
    assert manager.available_size() == 0
    hit = pool.get_cached_block(b"a", [0])
    assert hit is not None and store.restored[hit[0].block_id] == 1
    assert not pool._host_lru and not store.slots          # b found no room on the host (its only slot was held): dropped
    assert pool.get_cached_block(b"b", [0]) is None


def test_a_key_computed_again_replaces_its_host_entry():
    pool, manager, store = _pool(8, 4)
    _cache(pool, [b"a"])
    held = pool.get_new_blocks(7)
    pool.free_blocks(held)
    assert store.slots == {0: 1}
    again = _cache(pool, [b"a"])                           # registered on the GPU while a host entry exists
    pool.get_new_blocks(7)
    assert list(store.slots.values()) == again and len(pool._host_lru) == 1     # one entry, one slot: nothing leaked


def test_reset_clears_the_host_lru():
    pool, manager, store = _pool(8, 4)
    _cache(pool, [b"a", b"b"])
    held = pool.get_new_blocks(7)
    assert len(pool._host_lru) == 2
    assert pool.reset_prefix_cache()
    assert not pool._host_lru and not store.slots and store.calls[-1] == ("free", [0, 1])
    assert pool.get_cached_block(b"a", [0]) is None
    pool.free_blocks(held)
    assert pool.get_num_free_blocks() == 7


def test_a_failing_spill_degrades_to_plain_eviction():
    pool, manager, store = _pool(8, 4, fail=True)
    _cache(pool, [b"a", b"b"])
    blocks = pool.get_new_blocks(7)                        # nothing raised: the victims are freed as without a tier
    assert len(blocks) == 7 and [c[0] for c in store.calls] == ["offload"]
    assert not pool._host_lru and pool.get_cached_block(b"a", [0]) is None
    # a store that has no room (None) degrades the same way
    pool, manager, store = _pool(8, 4, capacity=1)
    _cache(pool, [b"a", b"b"])
    assert len(pool.get_new_blocks(7)) == 7 and not pool._host_lru and not store.slots


def test_the_tier_is_off_by_default(monkeypatch):
    monkeypatch.delenv("KVCACHED_HOST_CACHE_BLOCKS", raising=False)
    pool, manager, store = _pool(8, 0, capacity=4)
    assert pool._host_store is None
    _cache(pool, [b"a", b"b"])
    pool.get_new_blocks(7)
    assert store.calls == [] and pool.get_cached_block(b"a", [0]) is None
    with mock.patch("kvcached_amd.host_store.HostBlockStore") as made:
        pool, manager, _ = _pool(8, 0, with_store=False)
        _cache(pool, [b"a"])
        pool.get_new_blocks(7)
        assert not made.called and pool._host_store is None
        # without prefix caching there is nothing to keep on the host
        from kvcached_amd.integration.vllm.block_pool import build_elastic_block_pool
        cls = build_elastic_block_pool(T.FakeBlockPool, T.FakeKVCacheBlock)
        with mock.patch("kvcached_amd.integration.vllm.interfaces.get_kv_cache_manager", return_value=T.FifoBlockManager(8)):
            off = cls(num_gpu_blocks=8, block_size=16, cell_size=1024, num_layers=1, enable_caching=False, host_cache_blocks=4)
        assert off._host_store is None and not made.called


def test_the_switches_come_from_the_environment(monkeypatch):
    """Engine patches construct the pool with the reference's arguments: size and codec are read from the environment."""
    monkeypatch.setenv("KVCACHED_HOST_CACHE_BLOCKS", "5")
    monkeypatch.setenv("KVCACHED_HOST_CACHE_CODEC", "mxfp8:fp16")
    with mock.patch("kvcached_amd.host_store.HostBlockStore") as made:
        pool, manager, _ = _pool(8, 0, with_store=False)
    made.assert_called_once_with(manager, 5, codec="mxfp8", dtype=torch.float16)
    assert pool._host_store is made.return_value and pool._host_capacity == 5
    monkeypatch.setenv("KVCACHED_HOST_CACHE_CODEC", "zip")
    with pytest.raises(ValueError, match="KVCACHED_HOST_CACHE_CODEC"):
        _pool(8, 0, with_store=False)
    # a manager whose KV tensors live in other processes: one log line, the tier stays off
    monkeypatch.delenv("KVCACHED_HOST_CACHE_CODEC")
    from kvcached_amd.integration.vllm.block_pool import build_elastic_block_pool
    remote = T.FifoBlockManager(8)
    remote._kv_remote = True
    cls = build_elastic_block_pool(T.FakeBlockPool, T.FakeKVCacheBlock)
    with mock.patch("kvcached_amd.integration.vllm.interfaces.get_kv_cache_manager", return_value=remote):
        with mock.patch("kvcached_amd.host_store.HostBlockStore") as made:
            pool = cls(num_gpu_blocks=8, block_size=16, cell_size=1024, num_layers=1, enable_caching=True)
    assert pool._host_store is None and not made.called
