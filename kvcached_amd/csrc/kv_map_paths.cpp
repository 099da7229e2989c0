// kv_map_paths.cpp — the per-slot map batch and the two halves of unmap (see kv_allocator.hpp).
#include "kv_allocator_impl.hpp"

#include <algorithm>

#include "kernels.hpp"

namespace kvc {

// Async unmap, map side: when the pool has nothing idle, the page of a slot that is released but not yet
// unmapped is the cheapest handle there is (one hipMemUnmap, which was owed anyway) - and the handle population
// stays what it would be with synchronous unmaps instead of growing by hipMemCreate (O(live handles)). Needs mu_.
// The stale translation of the victim's VA is covered by the caller's TLB invalidation (before its fill).
bool KvAllocator::steal_pending(size_t ps, Phys *out) {
  while (!pending_.empty()) {
    Slot s = pending_.front();
    pending_.pop_front();
    KvRegion &r = *s.region;
    if (r.mapped[s.index] != UnmapQueued || r.page_size != ps) continue;
    const int64_t t0 = now_ns();
    if (r.rest_direct() && vmm_direct_bo(r.handle[s.index])) {
      if (rest_replace(r, s.index, 1) != 0) throw GpuError("putting a released slot back into its rest state failed");
    } else {
      vmm_unmap(r.base + s.index * ps, ps, r.handle[s.index]);
      if (r.rest_direct() && rest_map(r, s.index, 1) != 0) KVC_LOG(LOG_ERROR, "putting slot %zu back into its rest state failed", s.index);
    }
    if (vmm_extent_pages(r.handle[s.index]) > 1) // one page out of a larger mapping: see unmap_collect
      if (void *bo = vmm_direct_bo(r.handle[s.index])) (void)DrmVm::instance().refresh_mappings_of(bo, ps);
    stats().t_unmap += now_ns() - t0;
    r.mapped[s.index] = Unbacked;
    r.stale_epoch[s.index] = ctx_->next_flush_epoch();
    *out = Phys{r.handle[s.index], r.seq[s.index]};
    g_pending_unmap_bytes -= std::min(ps, g_pending_unmap_bytes.load());
    stats().pages_unmapped++;
    return true;
  }
  return false;
}

// Pages for `want` adjacent slots - at least one, at most `want`: the caller comes back for the rest - from the cheapest
// source that has any: what the pool holds idle; where the caller allows it (`stolen` != nullptr; async unmap) the page of
// a slot that is released but not yet unmapped, instead of creating one - a single page, so never where the unit is a
// lane; pages of an earlier unmap that wait for their invalidation - have it now rather than create; new memory.
// *stolen: the page's old address was live a moment ago (steal_pending has set tlb_stale): the caller waits for the
// invalidation that starts from now before the page is used.
size_t KvAllocator::acquire_pages(ExtentPool *pool, size_t want, Phys *out, bool *stolen) {
  bool recycled = false;
  size_t n = pool->acquire_run(want, out, &recycled, false);
  if (n) return n;
  if (stolen && (*stolen = steal_pending(pool->page_bytes(), out))) return 1;
  if (ctx_->limbo_bytes()) {
    ctx_->flush_limbo();
    n = pool->acquire_run(want, out, &recycled, false);
    if (n) return n;
  }
  return pool->acquire_run(want, out, &recycled, true);
}

// Settles a map batch: nothing may reach its new pages through a stale translation of their own addresses. What the
// batch's REPLACEs split - PRT mappings, the zero extent's group mappings (§4.8's hazard) - still carries fragments that
// span the new pages and is rewritten before the invalidation that covers it (DrmVm::refresh_prt_remainders,
// refresh_mappings_of). `replaced`: a translation this batch replaced (or, KVCACHED_MAP_SHOOTDOWN=always, made) is owed an
// invalidation that the caller has not noted in tlb_stale / need_epoch yet. Then only the invalidations that cover THESE
// slots' last unmaps have to be waited for (`need_epoch`): a stale translation of some other address cannot shadow a mapping
// made here, and it is gone a moment later anyway (every unmap batch has its invalidation under way on the context's
// thread). KVCACHED_MAP_WAITS_FOR_ALL_FLUSHES=true restores the blanket wait.
void settle_batch(GpuContext *ctx, size_t ps, bool &prt_dirty, void *&zx_dirty, uint64_t &need_epoch, bool replaced) {
  const int64_t t_rw = now_ns();
  if (prt_dirty) {
    if (!KVC_TEST_HOOK("SKIP_PRT_REMAINDER_REFRESH") && !DrmVm::instance().refresh_prt_remainders()) // (hook: prove the test has teeth)
      throw GpuError("rewriting the remainders of split PRT mappings failed");
    prt_dirty = false;
    replaced = true;
  }
  if (zx_dirty) {
    if (!DrmVm::instance().refresh_mappings_of(zx_dirty, ps)) KVC_LOG(LOG_ERROR, "rewriting the remaining mappings of the zero extent failed");
    zx_dirty = nullptr;
    replaced = true;
  }
  stats().seg[kSegMapRemainderRewrite] += now_ns() - t_rw;
  if (replaced) {
    tlb_stale().store(true);
    need_epoch = ctx->next_flush_epoch();
  }
  if (options().map_waits_for_all_flushes.load() || options().map_shootdown_always.load())
    ctx->ensure_flushed();
  else
    ctx->ensure_flushed_through(need_epoch);
}

// The state of one map_slots() batch on the GPU. Per slot: [register with HIP, once per 64 MiB group] -> [unmap the zero
// alias] -> pooled handle -> map (drm backend: one GEM_VA ioctl; else map + one set_access per contiguous run);
// zero_fill_pages launches that run on the GPU while the host keeps issuing driver calls for the next slots (3/4 of the
// batch, then the rest); a TLB invalidation before the first fill only if one is owed; one stream sync at the end.
struct KvAllocator::MapBatch {
  KvAllocator &a;
  GpuContext *const ctx;
  const size_t ps;
  ExtentPool *const pool;
  const std::vector<phys_handle_t> *const imported; // a peer's pages, one per slot, instead of pages from the pool
  std::vector<uint8_t> *const imported_consumed;
  const bool fill;
  const size_t max_run_bytes;
  // Run-sized extents (KVCACHED_PHYS_CHUNK_PAGES > 1, drm backend): the unbacked slots of the batch are collected
  // first and then backed run by run - adjacent slots get adjacent pages of one buffer and ONE map ioctl.
  const bool chunked;
  const bool hip_reg = vmm_hip_registered();
  // A TLB invalidation is owed before the new pages are touched only where a translation of these VAs (or of these
  // pages) may still sit in a TLB: an unmap whose invalidation was deferred, a slot whose zero alias or PRT entry is
  // being replaced, a page taken from a slot that was released but not yet unmapped. The translation of an UNMAPPED
  // address is never cached on GFX9+ - KFD itself flushes after unmap only on this GPU family, and re-backing slots
  // between busy neighbours with no invalidation after the map reads back right (tools/drm_vmm_probe.cpp mode 3) - so
  // a plain map of an unmapped slot whose last unmap was invalidated needs nothing (KVCACHED_MAP_SHOOTDOWN=always
  // restores it). A PRT entry is another matter: cached once looked at (tools/prt_tlb_probe.cpp).
  const bool always_flush = options().map_shootdown_always.load() != 0;
  bool dirty_tlb;           // an invalidation is owed before anything of this batch is touched
  uint64_t need_epoch = 0;  // ... and it is this one (settle_batch)
  void *zx_dirty = nullptr; // compat mode, zero extent: its group mappings were split by this batch's REPLACEs (§4.8's hazard)
  bool prt_dirty = false;   // PRT mappings were split by this batch: what is left of them carries fragments that span the new pages
  // Pages become usable in chunks: driver calls for <=`chunk` slots, ONE TLB shootdown (its cost grows only
  // mildly with the number of new mappings: 0.31 ms @256, 0.40 ms @1024), then the fill kernel
  // for exactly those slots runs on the GPU while the host issues the driver calls of the next chunk.
  // Fill launches: the kernel for the slots mapped so far runs while the host issues the driver calls for the rest, so
  // only the LAST launch is exposed. Large launches are more efficient (ramp and tail are ~10 us whatever the size:
  // 6.8 TB/s at 2 GiB, 6.4 at 512 MiB), the exposed one should be short: a batch of n >= 512 slots is filled as
  // 3/4 + 1/4 (1024 pages: 768 pages hidden behind the last 256 maps, 256 pages = 0.09 ms exposed instead of 0.33 ms
  // for one launch; p50 map batch 2.85 -> 2.6 ms). KVCACHED_FILL_CHUNK_SLOTS caps a launch (and while a TLB
  // invalidation is owed per chunk - compat mode, deferred unmaps - larger chunks mean fewer of them).
  const size_t chunk = (size_t)std::max<int64_t>(1, options().fill_chunk_slots.load());
  size_t next_cut;
  std::vector<void *> pending; // addresses mapped and not yet filled
  bool launched = false;
  uint64_t max_ticket = 0; // pages that were zeroed on their way back: nothing to launch, only that scrub to wait for
  std::vector<void *> run_pages; // mapped, hipMemSetAccess still owed: [run_start, run_start + run_len)
  char *run_start = nullptr;
  size_t run_len = 0;
  size_t next_import = 0;
  std::vector<Slot> done; // backed by this batch
  std::vector<Slot> kept; // async unmap: released but not yet unmapped -> simply kept, only zero-filled again
  SegTimer sg;

  MapBatch(KvAllocator &alloc, const std::vector<Slot> &slots, const std::vector<phys_handle_t> *imp, std::vector<uint8_t> *consumed)
      : a(alloc), ctx(alloc.ctx_), ps(slots[0].region->page_size), pool(ctx->extents(ps, alloc.exportable_)), imported(imp),
        imported_consumed(consumed), fill(options().zero_fill.load() && !imp),
        max_run_bytes(ps * (size_t)std::max<int64_t>(1, options().access_run_slots.load())), chunked(pool->multi_page() && !imp),
        dirty_tlb(ctx->tlb_owed()) {
    if (!a.exportable_ && !imported && !ctx->primary_pool()) ctx->set_primary_pool(pool); // the engine's own pool: the reserve is its
    for (auto &s : slots) need_epoch = std::max(need_epoch, s.region->stale_epoch[s.index]);
    // (with run-sized extents the driver calls of a whole batch take less time than a launch: nothing to hide a first
    // instalment behind, and one large launch is the more efficient one)
    const size_t n_total = slots.size();
    next_cut = (n_total >= 512 && !pool->multi_page()) ? std::min(chunk, n_total - std::max<size_t>(128, n_total / 4)) : chunk;
    done.reserve(n_total);
    sg.t = now_ns();
  }

  // only if one of these slots (or, compat mode, an alias replaced in this batch) is still owed an invalidation
  void settle() {
    settle_batch(ctx, ps, prt_dirty, zx_dirty, need_epoch, always_flush && dirty_tlb);
    dirty_tlb = false;
  }

  void launch_pending(bool all) {
    size_t i = 0;
    while (pending.size() - i >= next_cut || (all && i < pending.size())) {
      const size_t end = i + std::min(next_cut, pending.size() - i);
      settle();
      for (; i < end; i += std::min<size_t>(kMaxPtrsPerLaunch, end - i))
        ctx->zero_fill(pending.data() + i, std::min<size_t>(kMaxPtrsPerLaunch, end - i), ps, nullptr);
      launched = true;
      next_cut = chunk; // after the first launch: whatever is left, in launches of at most `chunk`
    }
    pending.erase(pending.begin(), pending.begin() + i);
  }

  void flush_run() {
    if (!run_len) return;
    const int64_t ta = now_ns();
    vmm_set_access(run_start, run_len, ctx->dev());
    stats().t_access += now_ns() - ta;
    if (always_flush) dirty_tlb = true;
    if (fill) {
      pending.insert(pending.end(), run_pages.begin(), run_pages.end());
      launch_pending(false);
    }
    run_pages.clear();
    run_len = 0;
  }

  // A rest mapping of `r` has just been taken away (CLEAR) or replaced. What was there may sit in a TLB: a zero alias is a
  // live translation (and the split remainders of its mapping are rewritten first), and a PRT entry is cached like one as
  // soon as anything has read or written the address (tools/prt_tlb_probe.cpp: after a chip-wide read of PRT slots,
  // backing them without an invalidation left every read stale and lost 0.8 % of the writes). Invalidate before use.
  void rest_mapping_gone(const KvRegion &r) {
    if (r.zx) zx_dirty = DrmVm::instance().find(r.zx_handle);
    if (r.prt) prt_dirty = true;
    tlb_stale().store(true);
    dirty_tlb = true;
    need_epoch = ctx->next_flush_epoch();
  }

  // A page that was just mapped: what still stands between the caller and zeros in it. True: nothing but a scrub that is
  // under way (the page was zeroed on its way back) - nothing to launch, only that ticket to wait for; false: it needs a
  // fill of its own (where one is wanted). (`ticket` by reference: the run loop keeps it in a register.)
  static bool prescrubbed(bool fill, const Phys &ph, uint64_t &ticket) {
    ticket = std::max(ticket, ph.wait_ticket); // (any older fill through the alias must be over before the caller writes)
    if (!fill || !ph.scrub_ticket) return false;
    ticket = std::max(ticket, ph.scrub_ticket);
    return true;
  }

  // Slots that are backed already: true if `s` was one (released but not yet unmapped: kept; anything else: logged, skipped)
  bool keep_or_skip(const Slot &s) {
    KvRegion &r = *s.region;
    if (r.mapped[s.index] == UnmapQueued && !imported) {
      r.mapped[s.index] = Own; // its queue entry is dropped by the reclaimer (no longer UnmapQueued)
      kept.push_back(s);
      g_pending_unmap_bytes -= std::min(ps, g_pending_unmap_bytes.load());
      stats().unmaps_cancelled++;
      if (fill) pending.push_back(r.base + s.index * ps);
      return true;
    }
    if (r.mapped[s.index]) { // reference: log + skip, the batch still succeeds (ftensor.cpp:104-107)
      KVC_LOG(LOG_ERROR, "Page %zu is already mapped.", s.index);
      if (imported) ++next_import;
      return true;
    }
    return false;
  }

  // One unbacked slot with driver calls of its own: single-page pools, zero aliases through ROCr, imports
  void back_slot(const Slot &s) {
    KvRegion &r = *s.region;
    char *va = r.base + s.index * ps;
    int64_t t0 = now_ns();
    if (hip_reg && !r.registered[s.index]) a.register_slot(r, s.index); // once per slot
    if (r.rest_direct() && !chunked) { // (chunked: replaced run by run in back_runs())
      if (DrmVm::instance().clear(va, ps) != 0) throw GpuError("dropping the rest mapping of a slot failed");
      rest_mapping_gone(r);
    } else if (r.backfilled && !r.rest_direct()) {
      vmm_unmap(va, ps);
      dirty_tlb = true; // the alias's translation is live
      need_epoch = ctx->next_flush_epoch();
    }
    int64_t t1 = now_ns();
    Phys ph;
    size_t import_index = 0;
    if (imported) {
      import_index = next_import;
      ph = Phys{(*imported)[next_import++], 0};
    } else {
      bool stolen = false;
      (void)a.acquire_pages(pool, 1, &ph, &stolen);
      if (stolen) {
        dirty_tlb = true;
        need_epoch = ctx->next_flush_epoch(); // (the page's old address was live a moment ago: conservative)
      }
    }
    int64_t t2 = now_ns();
    bool needs_access = true;
    try {
      needs_access = vmm_map(va, ps, ph.h);
    } catch (...) {
      if (!imported) pool->release(ph);
      if (r.rest_direct())
        (void)a.rest_map(r, s.index, 1); // (its rest mapping was cleared above)
      else if (r.backfilled && vmm_try_map(va, ps, r.zero_of(s.index)))
        (void)vmm_try_set_access(va, ps, ctx->dev());
      throw;
    }
    int64_t t3 = now_ns();
    stats().t_unmap_alias += t1 - t0;
    stats().t_acquire += t2 - t1;
    stats().t_map += t3 - t2;
    r.handle[s.index] = ph.h;
    r.seq[s.index] = ph.seq;
    r.mapped[s.index] = imported ? Imported : Own;
    if (imported && imported_consumed) (*imported_consumed)[import_index] = 1; // the slot owns it now (rollback releases it)
    if (!needs_access) { // mapped readable+writable in one ioctl (drm backend): straight to the fill queue
      if (always_flush) dirty_tlb = true;
      done.push_back(s);
      if (prescrubbed(fill, ph, max_ticket)) {
        stats().pages_prescrubbed++;
      } else if (fill) {
        pending.push_back(va);
        launch_pending(false);
      }
      return;
    }
    done.push_back(s);
    if (!(run_len && va == run_start + run_len && run_len < max_run_bytes)) {
      flush_run();
      run_start = va;
    }
    run_len += ps;
    run_pages.push_back(va);
  }

  // The fresh slots, run by run: as many neighbours as one extent can serve at a time, one ioctl each
  void back_runs(const std::vector<SlotRun> &runs) {
    std::vector<Phys> got(kMaxExtentPages);
    stats().seg[kSegMapRunCount] += (int64_t)runs.size();
    sg.mark(kSegMapRuns);
    for (const SlotRun &run : runs) {
      KvRegion &r = *run.r;
      // A region whose map path owes no invalidation (lazy mode: plain unmapped VA behind unbacked slots) keeps its mappings
      // at 512 MiB at most. Observed: a 2 GiB lazy map of recycled extent pages, with no invalidation on the map path, faulted
      // on its first read (tests/test_gpu_vmm.py::test_async_unmap_queue_reclaimer_and_rebacking); at <= 512 MiB it does
      // not. Not established why. One candidate: a run of 1 GiB or more may be written as a 1 GiB page-directory entry
      // where the TLBs still hold a pointer to a table. Regions with a rest mapping invalidate after their REPLACE anyway
      // and take whole batches.
      const size_t max_run = r.rest_direct() ? (size_t)-1 : std::max<size_t>(1, (512u << 20) / ps);
      for (size_t at = run.first, end = run.first + run.count; at < end;) {
        const int64_t t1 = now_ns();
        sg.mark(kSegMapBookkeeping);
        bool stolen = false;
        const size_t n = a.acquire_pages(pool, std::min(end - at, max_run), got.data(), &stolen);
        if (stolen) need_epoch = ctx->next_flush_epoch(); // (its unmap has set tlb_stale: flushed before the fill)
        const int64_t t2 = now_ns();
        sg.mark(kSegMapPool);
        char *va = r.base + at * ps;
        try {
          if (r.rest_direct()) { // the slots carry their rest mapping: pages take its place in the same ioctl
            vmm_replace_pieces(va, ps, n, got[0].h, /*live=*/true);
            rest_mapping_gone(r);
          } else {
            vmm_map_pieces(va, ps, n, got[0].h);
          }
        } catch (...) {
          pool->release_batch(got.data(), n);
          throw;
        }
        stats().t_acquire += t2 - t1;
        stats().t_map += now_ns() - t2;
        stats().seg[kSegMapIoctlCount]++;
        sg.mark(kSegMapIoctls);
        // (per page of the batch: everything this loop updates is a local or the regions' arrays - nothing is re-read
        // through `this` - and nothing in it can throw while `done` has entries that are not filled in yet)
        const bool want_fill = fill;
        uint64_t ticket = max_ticket;
        size_t clean = 0;
        done.resize(done.size() + n);
        Slot *d = done.data() + done.size() - n;
        for (size_t k = 0; k < n; ++k) {
          r.handle[at + k] = got[k].h;
          r.seq[at + k] = got[k].seq;
          r.mapped[at + k] = Own;
          d[k] = Slot{&r, at + k};
          clean += prescrubbed(want_fill, got[k], ticket);
        }
        if (want_fill && clean < n) // fresh memory, or pages that came back unscrubbed
          for (size_t k = 0; k < n; ++k)
            if (!got[k].scrub_ticket) pending.push_back(r.base + (at + k) * ps);
        max_ticket = ticket;
        if (clean) stats().pages_prescrubbed += (int64_t)clean;
        if (always_flush) dirty_tlb = true;
        if (fill) launch_pending(false);
        at += n;
      }
    }
  }

  // the last fills, the invalidation if one is still owed, and the wait for everything that was launched or was in flight
  void finish() {
    sg.mark(kSegMapBookkeeping);
    if (fill) launch_pending(true);
    settle(); // nothing may reach the new mappings through a stale translation of their own addresses
    sg.mark(kSegMapInvalidation);
    const int64_t ts = now_ns();
    if (launched) ctx->sync(nullptr);
    sg.mark(kSegMapWaitFill);
    ctx->wait_scrub(max_ticket);
    stats().t_sync += now_ns() - ts;
    sg.mark(kSegMapWaitScrub);
    if (max_ticket) stats().seg[kSegMapScrubsBehind] += (int64_t)(ctx->scrubs_issued() - max_ticket); // (diagnostics: how many scrubs behind the newest the one waited for was)
  }

  // leave the regions as they were before this call; PageAllocator rolls the page ids back
  void rollback() {
    roll_back(ctx, launched, [&]() {
      for (auto &k : kept) { // still in the reclaimer's queue: just hand them back to it
        k.region->mapped[k.index] = UnmapQueued;
        g_pending_unmap_bytes += ps;
      }
      for (auto it = done.rbegin(); it != done.rend(); ++it) {
        KvRegion &r = *it->region;
        char *va = r.base + it->index * ps;
        if (r.rest_direct()) { // back to its rest state, the page dropped in the same ioctl
          (void)a.rest_replace(r, it->index, 1);
        } else {
          (void)vmm_try_unmap(va, ps, r.handle[it->index]);
        }
        if (vmm_extent_pages(r.handle[it->index]) > 1)
          if (void *bo = vmm_direct_bo(r.handle[it->index])) (void)DrmVm::instance().refresh_mappings_of(bo, ps);
        if (r.mapped[it->index] == Own)
          pool->release(Phys{r.handle[it->index], r.seq[it->index]});
        else
          (void)vmm_try_release(r.handle[it->index]);
        r.mapped[it->index] = Unbacked;
        if (r.backfilled && !r.rest_direct() && vmm_try_map(va, ps, r.zero_of(it->index))) (void)vmm_try_set_access(va, ps, ctx->dev());
      }
    });
  }
};

void KvAllocator::map_slots(const std::vector<Slot> &slots, const std::vector<phys_handle_t> *imported,
                            std::vector<uint8_t> *imported_consumed) {
  if (slots.empty()) return;
  if (!dev_.is_gpu) { // reference CPUPage::map is a no-op (page.cpp:34-37); keep the double-map diagnostics
    for (auto &s : slots) {
      if (s.region->mapped[s.index] == UnmapQueued) { // async unmap: released, not yet reclaimed -> kept
        s.region->mapped[s.index] = Own;
        g_pending_unmap_bytes -= std::min(s.region->page_size, g_pending_unmap_bytes.load());
        stats().unmaps_cancelled++;
        stats().pages_mapped++;
        continue;
      }
      if (s.region->mapped[s.index]) {
        KVC_LOG(LOG_ERROR, "Page %zu is already mapped.", s.index);
        continue;
      }
      s.region->mapped[s.index] = Own;
      stats().pages_mapped++;
    }
    return;
  }
  ctx_->bind();
  MapBatch b(*this, slots, imported, imported_consumed);
  RunScan fresh; // chunked: the unbacked slots, backed run by run once every slot has been looked at
  const bool chunked = b.chunked, hip_reg = b.hip_reg;
  try {
    for (auto &s : slots) {
      KvRegion &r = *s.region;
      if (chunked && r.mapped[s.index] == Unbacked && (!r.backfilled || r.rest_direct())) { // the common case, nothing per slot but a bit
        if (hip_reg && !r.registered[s.index]) {
          const int64_t t0 = now_ns();
          register_slot(r, s.index); // once per slot
          stats().t_unmap_alias += now_ns() - t0;
        }
        // the same slot listed twice in one call: the reference logs "already mapped" for the second and goes on (ftensor.cpp:104-107)
        if (!fresh.add(&r, s.index)) KVC_LOG(LOG_ERROR, "Page %zu is already mapped.", s.index);
      } else if (!b.keep_or_skip(s)) {
        b.back_slot(s);
      }
    }
    b.flush_run();
    b.sg.mark(kSegMapClassify);
    if (fresh.size()) b.back_runs(fresh.collect());
    b.finish();
  } catch (...) {
    b.rollback();
    throw;
  }
  stats().pages_mapped += (int64_t)(b.done.size() + b.kept.size());
  if (b.pool->creations() > 0 && !imported && !exportable_) cold_start_reserve(b.pool); // (the reserve belongs to the engine's own pool, not to the exportable twin)
}

// Cold start: the first map calls of an allocator bring the reserve along (KVCACHED_PHYS_RESERVE_MB): pages
// that come back are zeroed behind the unmap, and a free()+alloc() cycle that can draw on an idle batch never waits for that
// fill. In instalments of 512 MiB per map call until it has stood once (the whole 2 GiB inside the first call was
// 7.6 ms in the smoke run and ~80 ms on VRAM the kernel has not wiped) - a bare C-ABI caller has no housekeeping thread to make
// it; where one exists (an engine: PageAllocator's watcher, 512 MiB per 100 ms tick) it takes over after the first instalment
// and keeps it up from then on.
void KvAllocator::cold_start_reserve(ExtentPool *pool) {
  if (reserve_built_) return;
  const size_t unit = pool->page_bytes();
  const size_t want = ctx_->reserve_target_bytes() / unit;
  if (!want || pool->idle_bytes() / unit >= want) {
    reserve_built_ = true;
    return;
  }
  (void)pool->refill_reserve(want, std::max<size_t>(1, (512u << 20) / unit));
  if (ctx_->has_housekeeper()) reserve_built_ = true; // (the thread makes the rest)
}

void KvAllocator::unmap_slots(const std::vector<Slot> &slots) {
  if (slots.empty()) return;
  if (!dev_.is_gpu) {
    for (auto &s : slots) {
      if (!s.region->mapped[s.index]) {
        KVC_LOG(LOG_ERROR, "Page %zu is not mapped.", s.index);
        continue;
      }
      s.region->mapped[s.index] = Unbacked;
      stats().pages_unmapped++;
    }
    return;
  }
  Unmapped u;
  unmap_collect(slots, u);
  unmap_finish(u, true);
}

// Driver unmaps (and, in compat mode, the re-aliasing) of `slots`; the handles are only collected. Needs mu_.
void KvAllocator::unmap_collect(const std::vector<Slot> &slots, Unmapped &u) {
  GpuContext *ctx = ctx_;
  ctx->bind();
  const size_t ps = slots[0].region->page_size;
  u.page_size = ps;
  char *run_start = nullptr;
  size_t run_len = 0;
  const size_t max_run = ps * (size_t)std::max<int64_t>(1, options().access_run_slots.load());
  auto flush_run = [&]() {
    if (!run_len) return;
    vmm_set_access(run_start, run_len, ctx->dev());
    run_len = 0;
  };
  u.own.reserve(slots.size());
  // Pages of a multi-page extent may have been mapped together with their neighbours in one ioctl; taking some of them
  // out splits that mapping, and what is left of it must be rewritten (DrmVm::refresh_mappings_of) before the TLBs are
  // invalidated. An extent that loses ALL its mapped pages in this batch leaves nothing behind to rewrite.
  ExtentPool *xpool = u.pool = ctx->extents(ps, exportable_);
  KeyGroups<uint32_t> touched(slots.size()); // extent -> pieces of it that this batch takes back
  std::vector<std::pair<KvRegion *, size_t>> gone;
  gone.reserve(slots.size());
  // drm backend, lazy regions: slots of this batch that are neighbours in VA go in runs - one CLEAR ioctl per run of up
  // to `clear_run_slots` instead of one UNMAP per slot (whatever the order the caller listed them in). Everything
  // inside such a run is a direct mapping of a page this very call gives up, so "drop all mappings in the range" is exact.
  std::vector<uint8_t> cleared(slots.size(), 0);
  SegTimer sg;
  const bool own_direct = xpool->multi_page(); // our own pages are direct DRM buffers (extent pools exist only on that path)
  { // PRT / zero extent: a run of adjacent slots goes back to its rest state with ONE ioctl that replaces whatever is
    // mapped there (zero extent: runs end at the extent's group boundaries - slot i shows page i % Z)
    RunScan scan;
    for (uint32_t i = 0; i < slots.size(); ++i) {
      KvRegion &r = *slots[i].region;
      const uint8_t m = r.mapped[slots[i].index];
      // (a page ROCr mapped is ROCr's to unmap; our own pages of an extent pool are KFD buffers imported into DRM, all of them:
      // no need to ask DrmVm about each one. A slot listed twice: the second mention is logged as "not mapped" below)
      if (r.rest_direct() && ((m == Own && own_direct) || ((m == Own || m == Imported) && vmm_direct_bo(r.handle[slots[i].index]))))
        if (scan.add(&r, slots[i].index)) cleared[i] = 2; // (2: and its extent is counted in `touched` with its run)
    }
    const std::vector<SlotRun> runs = scan.collect([](const KvRegion &r) { return r.rest_group(); });
    sg.mark(kSegUnmapRuns);
    for (const SlotRun &run : runs) {
      const int64_t t0 = now_ns();
      const int rc = rest_replace(*run.r, run.first, run.count);
      if (rc != 0) throw GpuError(std::string("DRM_AMDGPU_GEM_VA replace (back to the rest state) failed: ") + strerror(rc < 0 ? -rc : rc));
      stats().t_unmap += now_ns() - t0;
      stats().seg[kSegUnmapIoctlCount]++;
      // the extents these pages belong to, in address order: neighbours share theirs, so the list stays short
      if (own_direct)
        for (size_t k = run.first; k < run.first + run.count; ++k) {
          const phys_handle_t h = run.r->handle[k];
          if (run.r->mapped[k] == Own && is_piece(h)) ++touched.at(chunk_of(h));
        }
    }
  }
  sg.mark(kSegUnmapIoctls);
  size_t max_clear = (size_t)options().clear_run_slots.load();
  if (max_clear >= 2 && xpool->multi_page()) max_clear = std::max<size_t>(max_clear, xpool->max_extent_pages()); // a whole extent in one go
  if (max_clear >= 2 && vmm_backend() == kVmmDrm && DrmVm::instance().can_clear()) {
    RunScan scan; // (a slot listed twice: its second mention is logged as "not mapped" below)
    for (uint32_t i = 0; i < slots.size(); ++i) {
      KvRegion &r = *slots[i].region;
      const uint8_t m = r.mapped[slots[i].index];
      if (!r.backfilled && !r.rest_direct() && ((m == Own && own_direct) || ((m == Own || m == Imported) && vmm_direct_bo(r.handle[slots[i].index]))))
        if (scan.add(&r, slots[i].index)) cleared[i] = 1;
    }
    for (const SlotRun &run : scan.collect([](const KvRegion &) { return (size_t)-1; }, max_clear)) {
      const int64_t t0 = now_ns();
      vmm_unmap_run(run.r->base + run.first * ps, run.count * ps);
      stats().t_unmap += now_ns() - t0;
    }
  }
  for (size_t si = 0; si < slots.size(); ++si) {
    const Slot &s = slots[si];
    KvRegion &r = *s.region;
    if (r.mapped[s.index] != Own && r.mapped[s.index] != Imported) { // reference: log + skip (ftensor.cpp:124-127)
      KVC_LOG(LOG_ERROR, "Page %zu is not mapped.", s.index);
      continue;
    }
    char *va = r.base + s.index * ps;
    if (!cleared[si]) {
      const int64_t t0 = now_ns();
      vmm_unmap(va, ps, r.handle[s.index]);
      stats().t_unmap += now_ns() - t0;
    }
    const bool own = r.mapped[s.index] == Own;
    if (own)
      u.own.push_back(Phys{r.handle[s.index], r.seq[s.index]});
    else
      u.imported.push_back(r.handle[s.index]);
    r.mapped[s.index] = Unbacked;
    gone.emplace_back(&r, s.index);
    ++u.n;
    if (own && own_direct && cleared[si] != 2 && is_piece(r.handle[s.index])) ++touched.at(chunk_of(r.handle[s.index])); // (a tagged handle of our own pool: a page of a multi-page extent; those of the runs above are counted already)
    if (r.rest_direct()) {
      // Its rest state is back already (REPLACE above). In compat mode the invalidation happens inside this call:
      // "unbacked VA reads as zeros" holds from the moment unmap returns (an asynchronous invalidation would let a read
      // that follows at once still see the old page - observable, so not done); a lazy region's runs behind the call.
      if (r.backfilled) u.any_backfilled = true;
      if (!cleared[si] && rest_map(r, s.index, 1) != 0) // unmapped through ROCr just now (a page imported that way)
        KVC_LOG(LOG_ERROR, "putting slot %zu back into its rest state failed", s.index);
    } else if (r.backfilled) { // put the shared zero page back (ftensor.cpp:135-136), access ranged per run
      u.any_backfilled = true;
      const int64_t tr = now_ns();
      vmm_map(va, ps, r.zero_of(s.index));
      stats().t_realias += now_ns() - tr;
      if (!(run_len && va == run_start + run_len && run_len < max_run)) {
        flush_run();
        run_start = va;
      }
      run_len += ps;
    }
  }
  flush_run();
  u.foreign = !u.imported.empty();
  sg.mark(kSegUnmapBookkeeping);
  if (!touched.items().empty() && !KVC_TEST_HOOK("SKIP_REMAINDER_REFRESH")) { // hook: prove the test has teeth
    for (auto &kv : touched.items()) {
      // pieces still handed out beyond the ones this batch takes back = pages of the extent that stay mapped
      if (xpool->pieces_out(kv.first) > kv.second)
        if (void *bo = DrmVm::instance().find(kv.first))
          if (!DrmVm::instance().refresh_mappings_of(bo, ps)) KVC_LOG(LOG_ERROR, "rewriting the remaining mappings of an extent failed");
    }
    tlb_stale().store(true);
  }
  sg.mark(kSegUnmapRemainders);
  { // every driver call that removed or rewrote a translation has returned: the next invalidation to START covers them all
    const uint64_t epoch = ctx->next_flush_epoch();
    for (auto &g : gone) g.first->stale_epoch[g.second] = epoch;
    u.epoch = epoch;
  }
  sg.mark(kSegUnmapEpochs);
}

namespace {
// Zero pages on their way back: the fill is queued (through the alias mappings of their buffers) BEFORE they are on
// offer again, and whoever gets them next only waits for that ticket (GpuContext::scrub). `rows` == 0: `own` are single
// pages of a plain pool; otherwise lanes of `rows` pages each - page (row, lane) of a buffer of k lanes sits at
// (row x k + lane). Returns the scrub's ticket (0: nothing was queued).
uint64_t scrub_on_the_way_back(GpuContext *ctx, ExtentPool *pool, const std::vector<Phys> &own, size_t rows, size_t ps) {
  if (!options().zero_fill.load() || !options().scrub_on_release.load() || own.empty()) return 0;
  std::vector<uint64_t> addrs;
  if (!rows) {
    if (!pool->multi_page()) return 0;
    addrs.resize(own.size());
    if (!pool->scrub_addresses(own.data(), own.size(), addrs.data())) return 0;
  } else {
    addrs.reserve(own.size() * rows);
    for (const Phys &l : own)
      if (const uint64_t tag = pool->tag_of(l.h)) {
        const uint64_t ke = pages_of(l.h), j = piece_of(l.h);
        for (size_t r = 0; r < rows; ++r) addrs.push_back(tag + ((uint64_t)r * ke + j) * ps);
      }
    if (addrs.empty()) return 0;
  }
  return ctx->scrub(addrs.data(), addrs.size(), ps);
}
} // namespace

// TLB invalidation, then the handles go back to the pool / the driver. Touches no allocator state (the async
// reclaimer calls it without mu_).
void KvAllocator::unmap_finish(Unmapped &u, bool may_defer_shootdown) {
  if (!u.n) return;
  GpuContext *ctx = ctx_;
  ExtentPool *pool = u.pool;
  // Stale TLB entries still translate the unmapped VAs to the old physical pages. Who can be hurt by them?
  //   * a reader of the VA itself: only in compat mode is that legal (unbacked VA reads as zeros), so there the
  //     invalidation happens now;
  //   * the next owner of the physical page: if it stays in OUR pool, its next use is a map_slots() batch, which
  //     invalidates before anything touches the page - the invalidation CAN wait for that (or for the moment the
  //     pool gives handles back to the driver: ExtentDriver::before_release). Optional and off by default
  //     (KVC_OPT_DEFER_UNMAP_SHOOTDOWN): measured, the cost is conserved, not saved - the invalidation mostly waits
  //     for the page-table updates the unmaps queued, so it only moves from free() into the next alloc()
  //     (per page: unmap 354 -> 21 us, next map 205 -> 379 us; batches unchanged).
  //   * memory leaving this process (imported pages, pool evictions): invalidate first.
  //   * who pays: with an allocator watcher thread around (an engine, not a bare C-ABI caller) the owed invalidation
  //     is left to its next 100 ms tick (GpuContext::housekeeping) - the 0.3-0.4 ms KFD round trip leaves the
  //     caller's free() and, unless an alloc follows within that tick, reaches nobody's critical path
  //     (KVCACHED_ASYNC_SHOOTDOWN, on by default; one page id: free() 0.6 -> 0.2 ms).
  SegTimer sg;
  const int64_t trail_us = options().deferred_unmap_flush_us.load();
  if (trail_us > 0 && u.any_backfilled && !u.foreign && may_defer_shootdown && !u.own.empty()) {
    // compat, relaxed (KVCACHED_UNMAP_INVALIDATION_US): the invalidation trails the call by at most trail_us - performed by
    // the context's thread, or absorbed by the next map batch's own. The pages wait for it un-scrubbed and un-offered.
    auto own = std::make_shared<std::vector<Phys>>(std::move(u.own));
    const size_t rows = u.rows, ps = u.page_size;
    ctx->park(u.epoch, own->size() * pool->page_bytes(), [ctx, pool, own, rows, ps]() {
      pool->release_batch(own->data(), own->size(), scrub_on_the_way_back(ctx, pool, *own, rows, ps));
    });
    ctx->request_async_flush(trail_us);
    sg.mark(kSegUnmapInvalidation);
    stats().pages_unmapped += u.n;
    return;
  }
  const bool defer = options().defer_unmap_shootdown.load() || options().async_shootdown.load();
  if (u.any_backfilled || u.foreign || !may_defer_shootdown || !defer) {
    // (starting it on the context's thread and overlapping the scrub launch and the pool with it was tried: the thread
    // hand-off costs what the overlap gains)
    ctx->ensure_flushed();
  } else if (options().defer_unmap_shootdown.load())
    ctx->defer_tlb_shootdown(); // explicitly left to the next map batch / release to the driver
  else
    ctx->request_async_flush(); // this context's own thread does it now, off the caller's path
  for (auto h : u.imported) {
    if (!vmm_try_release(h)) KVC_LOG(LOG_ERROR, "releasing an imported handle failed");
  }
  sg.mark(kSegUnmapInvalidation);
  const int64_t tr0 = now_ns();
  const uint64_t ticket = scrub_on_the_way_back(ctx, pool, u.own, u.rows, u.page_size);
  sg.mark(kSegUnmapScrubLaunch);
  pool->release_batch(u.own.data(), u.own.size(), ticket);
  sg.mark(kSegUnmapPool);
  stats().t_release += now_ns() - tr0;
  stats().pages_unmapped += u.n;
}

} // namespace kvc
