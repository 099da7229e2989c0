"""The slot-granular host store on a real MI355X: copy_blocks_{to,from}_host_slots (raw and through the MXFP8 codec),
KVCacheManager.offload_to / .restore_from over a HostBlockStore, and the host tier of ElasticBlockPool's prefix cache.

Expected bytes come from three places: a numpy restatement of the arena ([slot][region][record]: row slots[i] holds block
ids[i]), the dense entries (kvc_copy_blocks_to_host and the codec pair, which tests/test_gpu_host_offload.py and
tests/test_gpu_kv_codec.py pin bit for bit: record slots[i] of the arena must equal record i of the dense image), and for the
pool under mxfp8 the CPU restatement of the codec (tests/kvc_mx_ref.py).

Sizes. The launcher splits a request every 768 ids (kMaxSlotIdsPerLaunch) and every 128 regions, in two independent loops, so
n runs over {1, 37, 768, 769} and the regions over {1, 2, 64, 130}; as in tests/test_gpu_host_offload.py a case whose image
n * regions * block_bytes would pass 256 MiB (an arena three times that, pinned) keeps n <= 37, which at 32 KiB leaves the id
split to 1 and 2 regions and the region split to n <= 37 - each loop is still crossed at every block size."""
import numpy as np
import pytest
import torch

import kvc_mx_ref as R
import kvc_testlib as T
from test_gpu_host_offload import (DEV, GUARD, MiB, PAGE, _expected_image, _fill, _holds, _ids, _manager_setup,  # noqa: F401
                                   _pinned, _regions, _stamp, lib)

pytestmark = pytest.mark.gpu

LIMIT = 768                                   # kMaxSlotIdsPerLaunch (kernels.hpp)
N_MATRIX = [1, 37, LIMIT, LIMIT + 1]
FILL = 0xA5


def _sizes(n_regions, bb):
    return [n for n in N_MATRIX if n <= 37 or n * n_regions * bb <= 256 * MiB]


def _slot_sets(n, seed):
    """Slot lists for n blocks in an arena of 3n + 2 slots: a shuffled subset with gaps that holds slot 0 and the last slot
    (n == 1: one list for each of the two)."""
    n_slots = 3 * n + 2
    if n == 1:
        return n_slots, [[0], [n_slots - 1]]
    rng = np.random.default_rng(seed)
    inner = rng.choice(np.arange(1, n_slots - 1), size=n - 2, replace=False)
    slots = np.concatenate([inner, [0, n_slots - 1]])
    rng.shuffle(slots)
    assert len(set(slots.tolist())) == n
    return n_slots, [[int(s) for s in slots]]


def _arena(n_slots, row, value=FILL):
    buf = _pinned(n_slots * row, value)       # with GUARD bytes behind it
    return buf, buf.numpy()[:n_slots * row].reshape(n_slots, row)


# ------------------------------------------------------------------ kernels, raw
@pytest.mark.parametrize("n_regions", [1, 2, 64, 130])
@pytest.mark.parametrize("bb", [16, 2064, 32 * 1024])
def test_slot_copies_byte_for_byte(lib, n_regions, bb):
    ops, capi = lib
    ns = _sizes(n_regions, bb)
    views = _regions(ops, capi, n_regions, (3 * max(ns) + 3) * bb)
    row = n_regions * bb
    for n in ns:
        ids = _ids(n, seed=n * 7 + bb)
        n_slots, sets = _slot_sets(n, seed=n * 11 + bb)
        for slots in sets:
            _fill(views, seed=n + bb)
            regs = [v.cpu().numpy() for v in views]
            # device -> host: the written rows are the blocks' images; every other row and the guard keep their fill byte
            buf, rows = _arena(n_slots, row)
            capi.copy_blocks_to_host_slots(0, ids, slots, bb, 0, buf.data_ptr(), n_slots)
            want = np.full((n_slots, row), FILL, dtype=np.uint8)
            want[slots] = _expected_image(regs, ids, bb).reshape(n, row)
            assert np.array_equal(rows, want), (n, bb, n_regions)
            assert (buf.numpy()[n_slots * row:] == FILL).all()
            # host -> device: exactly the target blocks change (so the copy above changed none); a slot named twice fills two
            # blocks with the same bytes
            rng = np.random.default_rng(n * 3 + bb)
            src, src_rows = _arena(n_slots, row, 0x5A)
            src_rows[:] = rng.integers(0, 256, size=(n_slots, row), dtype=np.uint8)
            image = src.numpy().copy()
            gather = list(slots)
            if n > 1:
                gather[-1] = gather[0]
            capi.copy_blocks_from_host_slots(0, ids, gather, bb, 0, src.data_ptr(), n_slots)
            got = [v.cpu().numpy() for v in views]
            picked = src_rows[gather].reshape(n, n_regions, bb)
            for r in range(n_regions):
                exp = regs[r].copy()
                exp[:(max(ids) + 1) * bb].reshape(-1, bb)[ids] = picked[:, r, :]
                assert np.array_equal(got[r], exp), (n, bb, n_regions, r)
                if n > 1:
                    blocks = got[r][:(max(ids) + 1) * bb].reshape(-1, bb)
                    assert np.array_equal(blocks[ids[-1]], blocks[ids[0]])
            assert np.array_equal(src.numpy(), image)


# ------------------------------------------------------------------ every codec against the dense entries
def _fill_floats(views, dt, seed):
    """Normal deviates times a per-group power of two, and a sprinkle of infinities and NaNs (their groups encode to 0xFF)."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    for v in views:
        groups = v.numel() // 64
        k = torch.randint(-8, 8, (groups, 1), device=DEV, generator=gen)
        x = torch.ldexp(torch.randn(groups, 32, device=DEV, generator=gen), k.expand(groups, 32))
        x[::97, 5] = float("inf")
        x[::89, 7] = float("nan")
        v.view(dt).copy_(x.to(dt).reshape(-1))
    torch.cuda.synchronize()


CODECS = [(0, torch.bfloat16), (R.CODEC[torch.bfloat16], torch.bfloat16), (R.CODEC[torch.float16], torch.float16)]


@pytest.mark.parametrize("codec,dt", CODECS, ids=["raw", "bf16", "fp16"])
@pytest.mark.parametrize("n_regions", [2, 130])
@pytest.mark.parametrize("bb", [1024, 32 * 1024])
def test_slot_image_equals_the_dense_image(lib, n_regions, bb, codec, dt):
    ops, capi = lib
    ns = [n for n in (37, LIMIT + 1) if n <= 37 or n * n_regions * bb <= 256 * MiB]
    views = _regions(ops, capi, n_regions, (3 * max(ns) + 3) * bb)
    rec = capi.codec_record_bytes(codec, bb) if codec else bb
    assert rec == (R.record_bytes(bb) if codec else bb)
    row = n_regions * rec
    _fill_floats(views, dt, seed=bb + n_regions + codec)
    before = [v.clone() for v in views]
    for n in ns:
        ids = _ids(n, seed=n * 7 + bb)
        n_slots, (slots,) = _slot_sets(n, seed=n * 13 + bb)
        dense = _pinned(n * row, FILL)
        if codec:
            capi.encode_blocks_to_host(0, ids, bb, codec, dense.data_ptr())
        else:
            capi.copy_blocks_to_host(0, ids, bb, dense.data_ptr())
        buf, rows = _arena(n_slots, row)
        capi.copy_blocks_to_host_slots(0, ids, slots, bb, codec, buf.data_ptr(), n_slots)
        want = np.full((n_slots, row), FILL, dtype=np.uint8)
        want[slots] = dense.numpy()[:n * row].reshape(n, row)
        assert np.array_equal(rows, want), (n, bb, n_regions, codec)
        assert (buf.numpy()[n_slots * row:] == FILL).all()
        # back into other blocks (the even ids are _ids' canaries; ids + 1 is even): the dense decode, then the slot decode
        targets = [i + 1 for i in ids]
        if codec:
            capi.decode_blocks_from_host(0, targets, bb, codec, dense.data_ptr())
        else:
            capi.copy_blocks_from_host(0, targets, bb, dense.data_ptr())
        from_dense = [v.clone() for v in views]
        for v, b in zip(views, before):
            v.copy_(b)
        torch.cuda.synchronize()
        capi.copy_blocks_from_host_slots(0, targets, slots, bb, codec, buf.data_ptr(), n_slots)
        for r, (v, d, b) in enumerate(zip(views, from_dense, before)):
            assert torch.equal(v, d), (n, bb, n_regions, codec, r)
            assert not torch.equal(d, b)
            v.copy_(b)
        torch.cuda.synchronize()


# ------------------------------------------------------------------ refusals
def test_refusals_touch_neither_the_arena_nor_the_device(lib):
    ops, capi = lib
    bb = 32 * 1024
    ops.init_kvcached(DEV, PAGE, False)
    ts = ops.create_kv_tensors(8 * PAGE, 1, DEV, 2, 2, 0, False)
    assert ops.map_to_kv_tensors([0, PAGE, 3 * PAGE])          # page 2 of each half stays unbacked
    bpp = PAGE // bb
    backed = [t.view(torch.uint8)[h * 4 * PAGE + p * PAGE:h * 4 * PAGE + (p + 1) * PAGE] for t in ts for h in range(2)
              for p in (0, 1, 3)]
    g = torch.Generator(device=DEV).manual_seed(3)
    for v in backed:
        v.copy_(torch.randint(0, 256, (v.numel(),), dtype=torch.uint8, device=DEV, generator=g))
    before = [v.clone() for v in backed]
    n_slots, row = 8, 4 * bb
    buf, rows = _arena(n_slots, row, 0xC3)
    to_host, from_host = capi.lib.kvc_copy_blocks_to_host_slots, capi.lib.kvc_copy_blocks_from_host_slots
    ok_ids = capi.i64_array([1, bpp + 5, 3 * bpp])

    def refused(fn, ids, slots, n, host=None, codec=0, size=bb, text=None):
        assert fn(0, ids, capi.i64_array(slots), n, size, codec, host or buf.data_ptr(), n_slots, None, 1) == capi.KVC_E_INVALID
        if text:
            assert text in capi.last_error(), capi.last_error()

    for fn in (to_host, from_host):
        refused(fn, ok_ids, [0, -1, 2], 3, text="slot -1")
        refused(fn, ok_ids, [0, n_slots, 2], 3, text=f"slot {n_slots}")
        refused(fn, capi.i64_array([1, bpp + 5, 2 * bpp + 7]), [0, 1, 2], 3, text="not backed")     # an unbacked block
        refused(fn, capi.i64_array([1, 4 * bpp, 2]), [0, 1, 2], 3)                                   # beyond the tensors
        refused(fn, capi.i64_array([1, -1, 2]), [0, 1, 2], 3)
        refused(fn, ok_ids, [0, 1, 2], 3, size=24)
        refused(fn, ok_ids, [0, 1, 2], 3, codec=7, text="codec")
        refused(fn, ok_ids, [0, 1, 2], 3, codec=1, size=2064)                                        # no whole 1 KiB pieces
        refused(fn, ok_ids, [0, 1, 2], 3, host=buf.data_ptr() + 8)
        assert fn(0, ok_ids, None, 3, bb, 0, buf.data_ptr(), n_slots, None, 1) == capi.KVC_E_INVALID
    refused(to_host, ok_ids, [5, 2, 5], 3, text="duplicate slot")                                     # the writes would race
    refused(from_host, capi.i64_array([1, 2, 1]), [0, 1, 2], 3, text="duplicate block id")
    # pageable memory
    pageable = np.full(n_slots * row, 0x3C, dtype=np.uint8)
    for fn in (to_host, from_host):
        refused(fn, ok_ids, [0, 1, 2], 3, host=pageable.ctypes.data, text="pinned")
    torch.cuda.synchronize()
    assert (pageable == 0x3C).all() and (buf.numpy() == 0xC3).all()
    for v, b in zip(backed, before):
        assert torch.equal(v, b)
    # what is legal passes: the same slots and ids, a slot read twice, an empty request
    assert to_host(0, ok_ids, capi.i64_array([5, 2, 7]), 3, bb, 0, buf.data_ptr(), n_slots, None, 1) == capi.KVC_OK
    assert from_host(0, ok_ids, capi.i64_array([5, 2, 5]), 3, bb, 0, buf.data_ptr(), n_slots, None, 1) == capi.KVC_OK
    assert to_host(0, None, None, 0, bb, 0, buf.data_ptr(), n_slots, None, 1) == capi.KVC_OK
    assert (rows[[0, 1, 3, 4, 6]] == 0xC3).all() and (buf.numpy()[n_slots * row:] == 0xC3).all()
    del ts


# ------------------------------------------------------------------ slots beyond 4 GiB
def test_slots_whose_offsets_straddle_4_gib(lib):
    """An arena of 65 538 rows of 2 regions x 32 KiB, just over 4 GiB: the rows of slots 65 534 .. 65 537 lie on both sides of
    byte 2^32 (slot 65 535 ends on it). Only they are written; a gather from them reads what was written."""
    ops, capi = lib
    bb, n_regions = 32 * 1024, 2
    views = _regions(ops, capi, n_regions, 16 * bb)
    row = n_regions * bb
    first = (1 << 32) // row - 2
    n_slots = first + 4
    assert (first + 1) * row < (1 << 32) == (first + 2) * row < n_slots * row
    _fill(views, seed=5)
    regs = [v.cpu().numpy() for v in views]
    ids, slots = [3, 9, 1, 12], [first + 2, first, first + 3, first + 1]
    buf = torch.empty(n_slots * row + GUARD, dtype=torch.uint8, pin_memory=True)
    words = buf[:n_slots * row].view(torch.int64)
    words.fill_(-1)
    buf[n_slots * row:].fill_(0xFF)
    capi.copy_blocks_to_host_slots(0, ids, slots, bb, 0, buf.data_ptr(), n_slots)
    below = words[:first * row // 8]                                   # every row below them: bytes 0xFF, int64 -1
    assert int(below.min()) == -1 and int(below.max()) == -1
    assert (buf[n_slots * row:] == 0xFF).all()
    got = buf.numpy()[first * row:n_slots * row].reshape(4, row)
    want = _expected_image(regs, ids, bb).reshape(4, row)
    for i, s in enumerate(slots):
        assert np.array_equal(got[s - first], want[i]), s
    back = [2, 4, 6, 8]
    capi.copy_blocks_from_host_slots(0, back, slots, bb, 0, buf.data_ptr(), n_slots)
    for r, v in enumerate(views):
        exp = regs[r].copy()
        exp.reshape(-1, bb)[back] = exp.reshape(-1, bb)[ids]
        assert np.array_equal(v.cpu().numpy(), exp), r


# ------------------------------------------------------------------ manager and store
def test_offload_to_and_restore_from_through_the_manager(lib, monkeypatch):
    from kvcached_amd.host_store import HostBlockStore
    ops, capi = lib
    m, views = _manager_setup(ops, monkeypatch, "per_layer")
    bpp = views[0].shape[0] // 16
    ids = m.alloc(bpp * 4)
    _stamp(views, ids)                                   # every block signed in every region
    torch.cuda.synchronize()
    store = HostBlockStore(m, 96)
    assert store.data.is_pinned() and store.data.numel() == 96 * len(views) * 32 * 1024
    first, second = ids[5:25], ids[bpp:2 * bpp] + ids[3 * bpp + 1:3 * bpp + 11]      # a whole page among the second batch
    inuse = m.page_allocator.get_num_inuse_pages()
    s1 = m.offload_to(store, first)
    s2 = m.offload_to(store, second)
    assert s1 == list(range(20)) and s2 == list(range(20, 20 + len(second))) and len(store) == 20 + len(second)
    assert m.page_allocator.get_num_inuse_pages() == inuse - 1
    assert m.offload_to(store, ids[:3]) is None and len(store) == 20 + len(second)   # 96 slots: no room for 3 more...
    gone = set(first + second)
    with pytest.raises(ValueError):
        m.offload_to(store, first[:1])                   # ...and a block that has left is free
    rest = m.alloc(m.available_size())                   # the freed blocks are handed out again and scribbled over
    for v in views:
        v[torch.tensor(rest, device=DEV)] = 0xEE
    torch.cuda.synchronize()
    rng = np.random.default_rng(8)
    pick = [int(k) for k in rng.permutation(len(s1 + s2))[:23]]
    mix, origin = [(s1 + s2)[k] for k in pick], [(first + second)[k] for k in pick]
    assert set(mix) & set(s1) and set(mix) & set(s2)
    assert m.restore_from(store, mix) is None            # the pool is full: nothing happens
    m.free(rest)
    new = m.restore_from(store, mix)                     # one gather from both batches, in shuffled order
    assert new is not None and len(new) == len(mix)
    m._check_live_blocks(new)
    # the slots go back and are taken again AT ONCE, by other blocks: the restore above still reads the old bytes
    store.free(mix)
    others = [b for b in ids if b not in gone][:len(mix)]
    s3 = m.offload_to(store, others)
    assert sorted(s3) == sorted(mix)
    torch.cuda.synchronize()
    assert _holds(views, new, origin)
    # the slots that stayed can be restored again, and the new tenants of the reused ones come back as themselves
    keep = [s for s in s1 + s2 if s not in set(mix)][:7]
    keep_origin = [(first + second)[(s1 + s2).index(s)] for s in keep]
    again = m.restore_from(store, keep + s3[:5] + keep[:1])
    torch.cuda.synchronize()
    assert _holds(views, again, keep_origin + others[:5] + keep_origin[:1])
    assert _holds(views, new, origin)
    with pytest.raises(ValueError):
        m.restore_from(store, [95])                      # not in use
    store.release()
    assert store.data is None


# ------------------------------------------------------------------ the pool's host tier
@pytest.mark.parametrize("codec", [None, "mxfp8"])
def test_prefix_cache_hits_come_back_from_the_host(monkeypatch, codec):
    """ElasticBlockPool over the real manager on cuda:0 (stub vLLM classes, as tests/test_prefix_cache_golden.py): cached
    blocks are evicted to the host tier by allocation pressure and overwritten; a lookup returns blocks whose bytes are the
    originals - or, under mxfp8, tests/kvc_mx_ref.py's encode-then-decode of them."""
    import kvcached_amd.integration.vllm.interfaces as vi
    from kvcached_amd import capi, vmm_ops
    from kvcached_amd.integration.vllm.block_pool import build_elastic_block_pool
    layers, tokens, cell, n_pages = 2, 16, 2048, 2
    bmem = tokens * cell
    nb = n_pages * (PAGE // bmem)
    dt = torch.bfloat16
    vmm_ops.init_kvcached(DEV, PAGE, False)
    monkeypatch.setattr(vi, "_kvcached_initialized", True)
    monkeypatch.setattr(vi, "_is_worker", True)
    try:
        raw = vmm_ops.create_kv_tensors(n_pages * PAGE * 2, 1, DEV, layers, 2, 0, False)
        cls = build_elastic_block_pool(T.FakeBlockPool, T.FakeKVCacheBlock)
        pool = cls(num_gpu_blocks=nb, block_size=tokens, cell_size=cell, num_layers=layers, enable_caching=True,
                   host_cache_blocks=16, host_cache_codec=codec, host_cache_dtype=dt if codec else None)
        assert pool.kv_cache_manager._post_init_done.wait(20)
        assert pool._host_store is not None and pool._host_store.data.is_pinned()
        views = []
        for t in raw:
            u = t.view(torch.uint8)
            half = u.numel() // 2
            views += [u[h * half:h * half + nb * bmem].view(nb, bmem).view(dt) for h in range(2)]
        hashes = [b"h%d" % i for i in range(10)]
        blocks = pool.get_new_blocks(len(hashes))
        gen = torch.Generator(device=DEV).manual_seed(12)
        originals = {}
        for h, b in zip(hashes, blocks):                 # "compute" the blocks: every region gets its own values
            k = torch.randint(-8, 8, (len(views), bmem // 64, 1), device=DEV, generator=gen)
            x = torch.ldexp(torch.randn(len(views), bmem // 64, 32, device=DEV, generator=gen), k.expand(-1, -1, 32)).to(dt)
            x = x.reshape(len(views), -1)
            for r, v in enumerate(views):
                v[b.block_id] = x[r]
            originals[h] = x.cpu()
        pool.cache_full_blocks(T.FakeRequest(hashes), blocks, 0, len(hashes), tokens, 0)
        pool.free_blocks(blocks)
        held = pool.get_new_blocks(pool.get_num_free_blocks())      # pressure: all ten are evicted, to the host
        assert len(pool._host_lru) == 10 and len(pool._host_store) == 10 and not pool._evictable_blocks
        for v in views:
            v[torch.tensor([b.block_id for b in held], device=DEV)] = 1.0
        torch.cuda.synchronize()
        assert pool.get_cached_block(hashes[3], [0]) is None        # no room, nothing evictable: a miss
        pool.free_blocks(held[:4])
        free = pool.get_num_free_blocks()
        for h in (hashes[7], hashes[2], hashes[9]):
            hit = pool.get_cached_block(h, [0])
            assert hit is not None and hit[0].ref_cnt == 0 and hit[0].block_id in pool._evictable_blocks
            want = originals[h]
            if codec:
                want = torch.stack([R.decode(*R.encode(row), dt) for row in want])
            got = torch.stack([v[hit[0].block_id] for v in views]).cpu()   # on the default stream: the pool has waited
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), h
            pool.touch(hit)
        assert pool.get_num_free_blocks() == free - 3 and len(pool._host_lru) == 7 and len(pool._host_store) == 7
        assert pool.reset_prefix_cache() and len(pool._host_store) == 0
        del pool
    finally:
        vmm_ops.shutdown_kvcached()
        capi.set_mem_info_override(0, 0)
