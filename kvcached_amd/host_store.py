"""HostBlockStore — a slot-granular pinned host store for KV blocks.

One pinned uint8 arena, allocated once: `capacity` slots, each the row [region][record] of one block (record = the
block's bytes in one region, or their MXFP8 encoding). KVCacheManager.offload_to() copies blocks into free slots and frees
them; KVCacheManager.restore_from() gathers any set of slots into newly allocated blocks with one launch
(copy_blocks_{to,from}_host_slots HIP kernels). Where an OffloadedBlocks handle is one dense image that leaves and returns
as a whole (a paused request), a store is filled and read slot by slot (a prefix cache: blocks are evicted one by one, and a
later prompt hits any subset of them), and nothing is allocated on the eviction path.

The free list hands out the lowest free slot first. A slot that was freed is not handed out again while a restore that
reads it may still be running: every restore leaves an event, and a freed slot waits for the events that were pending when
it was freed.
"""
from __future__ import annotations

import heapq
from typing import Any, List, Optional, Sequence, Tuple


class HostBlockStore:
    """HostBlockStore(manager, capacity, codec=None, dtype=None): `capacity` slots for blocks of `manager`'s geometry.

    codec / dtype: as KVCacheManager.offload ("mxfp8" with torch.bfloat16 or torch.float16; None: the bytes themselves).
    data: the pinned arena, [slot][region][record]; geometry: (group_id, contiguous layout, regions, block_bytes), the key
    an OffloadedBlocks handle carries; record_bytes: bytes of one (slot, region) record.
    offload / restore / free are what a prefix cache needs of a store (ElasticBlockPool's host tier)."""

    def __init__(self, manager: Any, capacity: int, codec: Optional[str] = None, dtype: Any = None):
        import torch
        from kvcached_amd import capi
        from kvcached_amd.kv_cache_manager import _codec_number
        if capacity <= 0:
            raise ValueError("a host store needs a capacity of at least one slot")
        manager._wait_post_init()
        bases, block_bytes = manager._block_geometry()
        self.codec_id = _codec_number(codec, dtype)
        self.record_bytes = capi.codec_record_bytes(self.codec_id, block_bytes) if self.codec_id else block_bytes
        if not self.record_bytes:
            raise ValueError(f"codec {codec!r} needs blocks of a multiple of 1024 bytes, not {block_bytes}")
        self.manager = manager
        self.capacity = int(capacity)
        self.codec, self.dtype = (codec, dtype) if self.codec_id else (None, None)
        self.geometry: Tuple[int, bool, int, int] = manager._geometry_key(len(bases), block_bytes)
        # pinned wherever a GPU exists; without one the library refuses the copies anyway (KVC_E_NO_GPU)
        self.data: Optional["torch.Tensor"] = torch.empty(self.capacity * len(bases) * self.record_bytes, dtype=torch.uint8,
                                                          pin_memory=torch.cuda.is_available())
        self._free: List[int] = list(range(self.capacity))      # a heap: the lowest slot first
        self._used: set = set()
        self._events: List[Any] = []                             # behind the restore copies that may still run
        self._held: List[Tuple[List[Any], List[int]]] = []       # (events, freed slots that wait for them)

    # ---- the free list
    def __len__(self) -> int:
        """Slots in use."""
        return len(self._used)

    @property
    def free_slots(self) -> int:
        return self.capacity - len(self._used)

    def _take(self, n: int) -> Optional[List[int]]:
        """The n lowest free slots, now in use; None (nothing changed) when fewer are free."""
        self._check_open()
        if n > self.free_slots:
            return None
        for events, slots in self._held:       # the copy that follows waits for its bytes anyway
            for ev in events:
                ev.synchronize()
            for s in slots:
                heapq.heappush(self._free, s)
        self._held = []
        slots = [heapq.heappop(self._free) for _ in range(n)]
        self._used.update(slots)
        return slots

    def _give_back(self, slots: Sequence[int]) -> None:
        """Undo a _take whose copy did not happen: nothing has read these slots."""
        for s in slots:
            self._used.discard(s)
            heapq.heappush(self._free, s)

    def _check_in_use(self, slots: Sequence[int], what: str) -> List[int]:
        self._check_open()
        out = [int(s) for s in slots]
        for s in out:
            if s not in self._used:
                raise ValueError(f"slot {s} is not in use ({what})")
        return out

    def _check_open(self) -> None:
        if self.data is None:
            raise ValueError("the host store was released")

    def _record(self) -> None:
        """An event behind the restore copy just queued on the current stream."""
        import torch
        self._events = [e for e in self._events if not e.query()]
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self._events.append(ev)

    def free(self, slots: Sequence[int]) -> None:
        """Give slots back. ValueError (nothing changed) for a slot that is not in use, twice in the list included."""
        slots = self._check_in_use(slots, "free")
        if len(set(slots)) != len(slots):
            raise ValueError("duplicate slot in free")
        self._used.difference_update(slots)
        self._events = [e for e in self._events if not e.query()]
        if self._events:
            self._held.append((list(self._events), slots))
        else:
            for s in slots:
                heapq.heappush(self._free, s)

    def wait(self) -> None:
        """Block until every restore copy queued so far has finished."""
        for ev in self._events:
            ev.synchronize()
        self._events = []

    def release(self) -> None:
        """Wait for the restore copies still reading the arena, then drop it. The store is unusable afterwards."""
        self.wait()
        self.data = None
        self._free, self._used, self._held = [], set(), []

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    # ---- the three operations of a prefix cache's host tier
    def offload(self, block_ids: Sequence[int]) -> Optional[List[int]]:
        """manager.offload_to(self, block_ids)"""
        return self.manager.offload_to(self, block_ids)

    def restore(self, slots: Sequence[int], wait: bool = False) -> Optional[List[int]]:
        """manager.restore_from(self, slots); wait: return only when the bytes are in the blocks."""
        ids = self.manager.restore_from(self, slots)
        if ids is not None and wait:
            self.wait()
        return ids
