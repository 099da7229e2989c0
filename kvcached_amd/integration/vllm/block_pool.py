"""ElasticBlockPool — vLLM's BlockPool interface on top of KVCacheManager, with a lazy-eviction prefix cache.

Behaviourally identical to the class the reference injects into `vllm.v1.core.block_pool`
(kvcached/integration/vllm/patches.py:308-614); tests/golden/prefix_cache.json holds traces recorded
from that class. It is built by a factory because its base class and block type belong to vLLM:

    ElasticBlockPool = build_elastic_block_pool(block_pool_mod.BlockPool, block_pool_mod.KVCacheBlock)

State:
  _cached_blocks     (block_hash, group) key -> block      prefix-cache index
  _block_id_to_key   block id -> key                        reverse index, O(1) eviction
  _evictable_blocks  OrderedDict id -> block                ref_cnt == 0 but still cached; LRU = insertion order
Rules the goldens pin: a block whose ref count drops to 0 is kept (evictable) iff it is cached, otherwise
freed at once; evictable blocks count as free; allocation evicts the oldest evictable blocks only when the
manager cannot satisfy the request; `max_cached_blocks` (>= 0) caps the evictable set after every free
(-1 = unlimited, 0 = evict immediately); lookups over several groups are all-or-nothing.

Addition, off by default: a host tier under the prefix cache (`host_cache_blocks` > 0, or KVCACHED_HOST_CACHE_BLOCKS). Evicted
blocks that have a cache key are spilled to a HostBlockStore (kvcached_amd/host_store.py) instead of being dropped, and a
lookup that finds a key there brings the block back. Extra state:
  _host_lru          OrderedDict key -> host slot           spilled blocks, oldest first
Host entries are not blocks: they count neither as free nor as used, and `evict_blocks` (by block id) leaves them alone.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import Any, Iterable, List, Optional, Tuple

from kvcached_amd.utils import get_kvcached_logger


def make_cache_key(block_hash: Any, group_id: int) -> bytes:
    """Prefix-cache key: the block hash's bytes followed by the 4-byte big-endian KV-cache group id
    (hybrid models keep several groups in one pool). Reference: patches.py:259-274."""
    if isinstance(block_hash, str):
        block_hash = block_hash.encode()
    return bytes(block_hash) + group_id.to_bytes(4, "big", signed=False)


def _host_cache_settings(blocks: int, codec: Optional[str], dtype: Any) -> Tuple[int, Optional[str], Any]:
    """(host_cache_blocks, codec, dtype) with what the constructor left unset taken from KVCACHED_HOST_CACHE_BLOCKS and
    KVCACHED_HOST_CACHE_CODEC ("mxfp8:bf16" or "mxfp8:fp16"): engine patches construct the pool with the reference's arguments."""
    if not blocks:
        blocks = int(os.environ.get("KVCACHED_HOST_CACHE_BLOCKS", "0") or 0)
    spec = os.environ.get("KVCACHED_HOST_CACHE_CODEC", "")
    if codec is None and spec:
        name, _, elem = spec.partition(":")
        if name != "mxfp8" or elem not in ("bf16", "fp16"):
            raise ValueError(f"KVCACHED_HOST_CACHE_CODEC={spec!r}: expected 'mxfp8:bf16' or 'mxfp8:fp16'")
        import torch
        codec, dtype = name, {"bf16": torch.bfloat16, "fp16": torch.float16}[elem]
    return max(0, int(blocks)), codec, dtype


def build_elastic_block_pool(block_pool_cls: type, kv_cache_block_cls: type, logger=None) -> type:
    log = logger or get_kvcached_logger()

    class ElasticBlockPool(block_pool_cls):  # type: ignore[misc, valid-type]
        """BlockPool whose blocks are backed on demand by kvcached."""

        def __init__(self, num_gpu_blocks: int, block_size: int, cell_size: int, num_layers: int, enable_caching: bool,
                     enable_kv_cache_events: bool = False, num_kv_buffers: int = 2, max_cached_blocks: int = 1000,
                     host_cache_blocks: int = 0, host_cache_codec: Optional[str] = None, host_cache_dtype: Any = None,
                     host_store: Any = None) -> None:
            assert isinstance(num_gpu_blocks, int) and num_gpu_blocks > 0
            assert not enable_kv_cache_events, "KV cache events are not supported in ElasticBlockPool"
            self.enable_prefix_cache = enable_caching
            self.max_cached_blocks = max_cached_blocks          # -1 unlimited, 0 disabled, > 0 cap
            if enable_caching:
                log.info("Prefix caching enabled for ElasticBlockPool")
            self.num_gpu_blocks = num_gpu_blocks
            self.enable_kv_cache_events = enable_kv_cache_events
            self.kv_event_queue: list = []
            self.kv_block_pool = [kv_cache_block_cls(i) for i in range(num_gpu_blocks)]

            from kvcached_amd.integration.vllm.interfaces import get_kv_cache_manager
            self.kv_cache_manager = get_kv_cache_manager(num_gpu_blocks, block_size, cell_size, num_layers,
                                                         num_kv_buffers=num_kv_buffers)
            # vLLM's pool reserves block 0 as the "null" block for skipped positions; here it is a real,
            # backed block so that kernels may read it (their results are masked)
            null_ids = self.kv_cache_manager.alloc(1)
            assert null_ids is not None and len(null_ids) == 1
            self.null_block = self.kv_block_pool[null_ids[0]]
            self.null_block.is_null = True

            self._cached_blocks: dict = {}
            self._block_id_to_key: dict = {}
            self._evictable_blocks: "OrderedDict[int, Any]" = OrderedDict()

            # host tier (off unless asked for): host_store is any object with offload(block_ids) -> slots | None,
            # restore(slots, wait=True) -> block ids | None and free(slots), as HostBlockStore has them
            self._host_store: Any = None
            self._host_capacity = 0
            self._host_pinned = 0                # slots a running promotion holds outside the LRU
            self._host_lru: "OrderedDict[bytes, int]" = OrderedDict()
            blocks, codec, dtype = _host_cache_settings(host_cache_blocks, host_cache_codec, host_cache_dtype)
            if blocks > 0 and enable_caching:
                if getattr(self.kv_cache_manager, "_kv_remote", False):
                    log.info("Host tier of the prefix cache is off: the KV tensors are not in this process")
                else:
                    if host_store is None:
                        from kvcached_amd.host_store import HostBlockStore
                        host_store = HostBlockStore(self.kv_cache_manager, blocks, codec=codec, dtype=dtype)
                    self._host_store, self._host_capacity = host_store, blocks
                    log.info(f"Host tier of the prefix cache: {blocks} blocks")

        # ---- lookup / registration
        def get_cached_block(self, block_hash: Any, kv_cache_group_ids: Optional[Iterable[int]] = None):
            if not self.enable_prefix_cache:
                return None
            if kv_cache_group_ids is None:       # old call form: one block, group 0
                key = make_cache_key(block_hash, 0)
                block = self._cached_blocks.get(key)
                if block is None and key in self._host_lru and self._promote_from_host([key], ()):
                    block = self._cached_blocks.get(key)
                return block
            if isinstance(kv_cache_group_ids, int):
                kv_cache_group_ids = [int(kv_cache_group_ids)]
            keys = [make_cache_key(block_hash, int(gid)) for gid in kv_cache_group_ids]
            on_host = []
            for key in keys:                      # resolve every group before anything changes
                if key in self._cached_blocks:
                    continue
                if key not in self._host_lru:
                    return None                   # every group must hit
                if key not in on_host:
                    on_host.append(key)
            if on_host and not self._promote_from_host(on_host, [self._cached_blocks[k].block_id for k in keys
                                                                 if k in self._cached_blocks]):
                return None
            return [self._cached_blocks[k] for k in keys] or None

        def _promote_from_host(self, keys: List[bytes], keep: Iterable[int]) -> bool:
            """Bring the blocks of `keys` (all in the host LRU) back with one restore: each is registered under its key and
            idle (evictable, ref_cnt 0), and its host slot is freed. Room is made as get_new_blocks makes it, oldest
            evictable first, but never from `keep`, the GPU hits of the same lookup. False, with nothing changed, when
            room cannot be made or the restore fails."""
            manager, store = self.kv_cache_manager, self._host_store
            short = len(keys) - manager.available_size()
            victims: List[int] = []
            if short > 0:
                keep = set(keep)
                victims = [bid for bid in self._evictable_blocks if bid not in keep][:short]
                if len(victims) < short:
                    return False
            # out of the LRU while room is made: the victims spill in turn, and that must not drop these entries
            slots = [self._host_lru.pop(k) for k in keys]
            self._host_pinned = len(slots)
            ids = None
            try:
                if victims:
                    self._evict_blocks(victims)
                ids = store.restore(slots, wait=True)   # waited for: the engine's attention stream is not known here
            except Exception as e:
                log.warning(f"Host tier: restore failed ({e}); treated as a miss")
            finally:
                self._host_pinned = 0
            if ids is None:
                self._host_lru.update(zip(keys, slots))
                return False
            for key, bid in zip(keys, ids):
                block = self.kv_block_pool[bid]
                block.ref_cnt = 0
                self._cached_blocks[key] = block
                self._block_id_to_key[bid] = key
                self._evictable_blocks[bid] = block
            store.free(slots)
            return True

        def cache_full_blocks(self, request, blocks, *args: Any, **kwargs: Any) -> None:
            """Accepts every call form vLLM has used: (request, blocks, [block_hashes,] num_cached_blocks,
            num_full_blocks, block_size[, kv_cache_group_id][, hash_fn]) positionally or by keyword."""
            if not self.enable_prefix_cache:
                return
            block_hashes = kwargs.pop("block_hashes", None)
            num_cached = kwargs.pop("num_cached_blocks", None)
            num_full = kwargs.pop("num_full_blocks", None)
            block_size = kwargs.pop("block_size", None)
            group_id = kwargs.pop("kv_cache_group_id", 0)
            kwargs.pop("hash_fn", None)
            rest = list(args)
            if block_hashes is None and rest and isinstance(rest[0], (list, tuple)):
                block_hashes = rest.pop(0)
            if num_cached is None and rest:
                num_cached = rest.pop(0)
            if num_full is None and rest:
                num_full = rest.pop(0)
            if block_size is None and rest:
                block_size = rest.pop(0)
            if rest and isinstance(rest[0], int):
                group_id = rest.pop(0)
            if num_cached is None or num_full is None:
                raise TypeError("cache_full_blocks requires num_cached_blocks and num_full_blocks")
            num_cached, num_full, group_id = int(num_cached), int(num_full), int(group_id)
            if num_cached >= num_full:
                return
            if block_hashes is None:
                assert hasattr(request, "block_hashes"), "Request missing block_hashes attribute"
                block_hashes = request.block_hashes
            assert len(block_hashes) >= num_full, f"Request has {len(block_hashes)} hashes but need {num_full}"
            for i, block in enumerate(blocks[num_cached:num_full]):
                if getattr(block, "is_null", False):
                    continue
                key = make_cache_key(block_hashes[num_cached + i], group_id)
                if key in self._cached_blocks:
                    continue                       # idempotent: first registration wins
                self._cached_blocks[key] = block
                self._block_id_to_key[block.block_id] = key

        # ---- allocation / release
        def _evict_blocks_from_pool(self, num_to_evict: int) -> int:
            n = min(num_to_evict, len(self._evictable_blocks))
            return self._evict_blocks(list(self._evictable_blocks)[:n])      # oldest first

        def _evict_blocks(self, victims: List[int]) -> int:
            """Evictable blocks `victims`, oldest first, leave the GPU: to the host tier where there is one, else freed."""
            spill: List[Tuple[int, bytes]] = []
            for bid in victims:
                del self._evictable_blocks[bid]
                key = self._block_id_to_key.pop(bid, None)
                if key is not None:
                    self._cached_blocks.pop(key, None)
                    spill.append((bid, key))
            if victims:
                spilled = self._spill_to_host(spill) if self._host_store is not None and spill else set()
                rest = [bid for bid in victims if bid not in spilled]
                if rest:
                    self.kv_cache_manager.free(rest)
            return len(victims)

        def _spill_to_host(self, spill: List[Tuple[int, bytes]]) -> set:
            """One offload of the youngest `capacity` of (block id, key), oldest first; the oldest host entries make room.
            Returns the block ids that went (the store has freed them); on any failure none, and nothing is raised."""
            room = self._host_capacity - self._host_pinned
            spill = spill[-room:] if room > 0 else []
            if not spill:
                return set()
            store = self._host_store
            try:
                # an entry of the same key (the block was computed again instead of looked up) is stale: the block replaces it
                gone = [self._host_lru.pop(key) for _, key in spill if key in self._host_lru]
                for _ in range(len(self._host_lru) + len(spill) - room):
                    gone.append(self._host_lru.popitem(last=False)[1])
                if gone:
                    store.free(gone)
                slots = store.offload([bid for bid, _ in spill])
            except Exception as e:
                log.warning(f"Host tier: spill of {len(spill)} blocks failed ({e}); they are dropped")
                return set()
            if slots is None:
                return set()
            for (_, key), slot in zip(spill, slots):
                self._host_lru[key] = slot
            return {bid for bid, _ in spill}

        def get_new_blocks(self, num_blocks: int):
            if num_blocks > self.get_num_free_blocks():
                raise ValueError(f"Cannot get {num_blocks} free blocks from the pool")
            ids = None
            for _ in range(2):
                if self.enable_prefix_cache:
                    have = self.kv_cache_manager.available_size()
                    if have < num_blocks and self._evictable_blocks:
                        self._evict_blocks_from_pool(num_blocks - have)
                ids = self.kv_cache_manager.alloc(num_blocks)
                if ids is not None:
                    break
            if ids is None:
                raise ValueError("Unable to allocate KV cache blocks from physical pool; "
                                 f"requested={num_blocks}, available={self.kv_cache_manager.available_size()}")
            assert len(ids) == num_blocks, f"alloc returned {len(ids)} blocks, expected {num_blocks}"
            out = []
            for bid in ids:
                block = self.kv_block_pool[bid]
                block.ref_cnt = 1
                out.append(block)
            return out

        def touch(self, blocks) -> None:
            if not self.enable_prefix_cache:
                return
            groups = blocks if isinstance(blocks, tuple) else (blocks,)
            for group in groups:
                for block in group:
                    block.ref_cnt += 1
                    self._evictable_blocks.pop(block.block_id, None)     # in use again

        def free_blocks(self, ordered_blocks: Iterable[Any]) -> None:
            if not self.enable_prefix_cache:
                ids = [b.block_id for b in ordered_blocks if b is not None and not getattr(b, "is_null", False)]
                if ids:
                    self.kv_cache_manager.free(ids)
                return
            to_free: List[int] = []
            for block in ordered_blocks:
                if block is None or getattr(block, "is_null", False):
                    continue
                block.ref_cnt -= 1
                if block.ref_cnt == 0:
                    if block.block_id in self._block_id_to_key:
                        self._evictable_blocks[block.block_id] = block    # keep for later requests
                    else:
                        to_free.append(block.block_id)                    # never cached (e.g. partial block)
            if to_free:
                self.kv_cache_manager.free(to_free)
            if self.max_cached_blocks >= 0 and len(self._evictable_blocks) > self.max_cached_blocks:
                self._evict_blocks_from_pool(len(self._evictable_blocks) - self.max_cached_blocks)

        def evict_blocks(self, block_ids) -> None:
            """By block id: a block that has gone to the host tier has no id, so host entries stay."""
            if not self.enable_prefix_cache:
                return
            removed, to_free = 0, []
            for bid in block_ids:
                key = self._block_id_to_key.pop(bid, None)
                if key is not None:
                    self._cached_blocks.pop(key, None)
                    removed += 1
                if bid in self._evictable_blocks:
                    self._evictable_blocks.pop(bid)
                    to_free.append(bid)
            if to_free:
                self.kv_cache_manager.free(to_free)
            if removed:
                log.debug(f"Evicted {removed} blocks from prefix cache")

        def reset_prefix_cache(self) -> bool:
            if not self.enable_prefix_cache:
                return True
            if self._evictable_blocks:
                ids = list(self._evictable_blocks.keys())
                self._evictable_blocks.clear()
                self.kv_cache_manager.free(ids)
            self._cached_blocks.clear()
            self._block_id_to_key.clear()
            if self._host_lru:
                slots = list(self._host_lru.values())
                self._host_lru.clear()
                self._host_store.free(slots)
            log.info("Prefix cache reset")
            return True

        # ---- accounting
        def get_num_free_blocks(self) -> int:
            free = self.kv_cache_manager.available_size()
            return free + len(self._evictable_blocks) if self.enable_prefix_cache else free

        def get_usage(self) -> float:
            return 1.0 - (self.get_num_free_blocks() / self.num_gpu_blocks)

        def take_events(self) -> list:
            return []

    return ElasticBlockPool
