// kv_lanes.cpp — page ids backed, released, exported and imported as units (see kv_allocator.hpp).
#include "kv_allocator_impl.hpp"

#include <unistd.h>

#include <algorithm>

#include "kernels.hpp"

namespace kvc {

// ------------------------------------------------------------------ lanes
// The geometry engines use on ROCm (the reference forces it there: kvcached/utils.py:150-171) is one region per layer with a
// K half and a V half, so ONE page id is `rows` = layers x 2 single slots in as many places of the address space
// (csrc/allocator.cpp:189-206: 64 for Llama-3-8B) and k consecutive page ids are `rows` runs of k slots. What the kernel
// charges for is the page-table RANGE, not the byte (tools/engine_ioctl_probe.cpp: 2.5 us per MAP, 4.1 per REPLACE over
// PRT, +0.23 us per further page of the range, 2.7 us per remainder of a PRT mapping that a REPLACE split), so a page id
// costs `rows` ioctls whatever user space does - and everything else should cost nothing. A page id is allocated and freed as a
// unit (PageAllocator), so it is BACKED as a unit: a LANE, the `rows` pages behind one page id, taken from and given back
// to the pool in one piece (1 pool operation per page id instead of 64; what is recycled has exactly the shape that is
// asked for, so the footprint is that of the page ids in use). A buffer holds k lanes ROW-MAJOR - page (row, lane) at
// (row x k + lane) - so that k consecutive page ids backed by one call are still ONE ioctl per row; lanes of such a buffer
// go back one by one (a free lane of a partly used buffer serves the next single page id at full speed: 64 ioctls
// either way) and the buffer leaves for the driver when the last one is home. ExtentPool does the bookkeeping with the
// lane as its unit; this file knows where a lane's pages are.
void KvAllocator::setup_lanes() {
  lanes_ = false;
  rows_.clear();
  lane_pool_ = nullptr;
  if (!dev_.is_gpu || contiguous_ || exportable_ || layers_.empty() || !ctx_) return;
  if (!env_option("KVCACHED_LANE_EXTENTS") || options().phys_chunk_pages.load() <= 1) return;
  if (options().async_unmap.load()) return; // queued unmaps work slot by slot (the reclaimer's chunks): the per-slot path keeps them
  const bool kv = !unified_pool_ && num_kv_buffers_ == 2;
  for (auto &r : layers_) {
    if (r->backfilled && !r->rest_direct()) return; // (zero aliases through ROCr: the fallback's fallback keeps the per-slot path)
    rows_.push_back(Row{r.get(), 0});
    if (kv) rows_.push_back(Row{r.get(), r->num_slots() / 2}); // get_v_base_offset, allocator.cpp:46-52
  }
  ids_per_row_ = kv ? layers_[0]->num_slots() / 2 : layers_[0]->num_slots();
  if (rows_.size() >= 2) lane_pool_ = ctx_->lane_extents(rows_.size(), layers_[0]->page_size);
  if (!lane_pool_) {
    rows_.clear();
    return;
  }
  lanes_ = true;
}

namespace {
// slots [first, first + n) of a region, cut where its rest state must be (zero extent: its pages repeat; PRT: groups)
template <class F> void for_rest_pieces(const KvRegion &r, size_t first, size_t n, F &&f) {
  const size_t g = r.rest_group();
  while (n) {
    const size_t take = g == (size_t)-1 ? n : std::min(n, g - first % g);
    f(first, take);
    first += take;
    n -= take;
  }
}
} // namespace

// The page id an offset names: a multiple of the page size inside one row. kNoPageId: it names none of this geometry.
size_t KvAllocator::page_id_of(offset_t off) const {
  const size_t ps = rows_[0].r->page_size;
  return off >= 0 && (size_t)off % ps == 0 && (size_t)off / ps < ids_per_row_ ? (size_t)off / ps : kNoPageId;
}

// f(region, slot of page id p in it) for every row: what a path writes per row - handle, seq, mapped, stale_epoch - over a
// run of page ids that starts at p
template <class F> void KvAllocator::for_rows(size_t p, F &&f) {
  for (const Row &row : rows_) f(*row.r, row.first + p);
}

// Backs page ids [p, p + cnt) of every row with lanes j0 .. j0 + cnt of buffer `bo`, which holds k lanes: one ioctl per row -
// pages (r, j0 .. j0 + cnt) are neighbours in the buffer. Returns 0, or what the driver said, with `rows_done` rows backed.
int KvAllocator::back_rows(void *bo, uint64_t j0, uint64_t k, size_t p, size_t cnt, RowsSplit &split, size_t &rows_done) {
  DrmVm &vm = DrmVm::instance();
  for (size_t r = 0; r < rows_.size(); ++r) {
    KvRegion &reg = *rows_[r].r;
    const size_t ps = reg.page_size;
    char *va = reg.base + (rows_[r].first + p) * ps;
    const uint64_t boff = ((uint64_t)r * k + j0) * ps;
    int rc;
    if (reg.rest_direct()) { // pages take the place of the rest mapping in the same ioctl
      tlb_stale().store(true);
      rc = vm.replace(bo, va, cnt * ps, boff);
      tlb_stale().store(true); // what was there may sit in a TLB (a zero alias; a PRT entry that was looked at: §4.2)
      split.replaced = true;
      if (reg.zx) split.zx_dirty = vm.find(reg.zx_handle);
      if (reg.prt) split.prt_dirty = true;
    } else {
      rc = vm.map(bo, va, cnt * ps, boff);
    }
    if (rc != 0) return rc;
    rows_done = r + 1;
  }
  return 0;
}

// Takes back_rows back: the first `rows_done` rows of page ids [p, p + cnt) go back to their rest state; a row that has none
// is unmapped by the path's own driver call, `unmap(region, first slot)`. `settled`: the slots said they were backed.
template <class Unmap> void KvAllocator::undo_rows(size_t p, size_t cnt, size_t rows_done, bool settled, Unmap &&unmap) {
  for (size_t r = 0; r < rows_done; ++r) {
    KvRegion &reg = *rows_[r].r;
    if (reg.rest_direct())
      for_rest_pieces(reg, rows_[r].first + p, cnt, [&](size_t first, size_t n) { (void)rest_replace(reg, first, n); });
    else
      unmap(reg, rows_[r].first + p);
  }
  if (settled)
    for_rows(p, [&](KvRegion &reg, size_t first) { std::fill(reg.mapped.begin() + first, reg.mapped.begin() + first + cnt, Unbacked); });
}

bool KvAllocator::try_map_lanes(const offset_t *offsets, size_t n) {
  if (!n) return true;
  const size_t R = rows_.size(), ps = rows_[0].r->page_size;
  SegTimer sg;
  // Every slot the call names must be unbacked. Anything else - a page id named twice, a slot that is mapped already, an
  // imported page, a queued unmap, an offset that is none - is the generic path's business (it logs and goes on, or
  // throws, as the reference does: ftensor.cpp:104-107).
  uint64_t need_epoch = 0;
  RunScan scan;
  for (size_t i = 0; i < n; ++i) {
    const size_t p = page_id_of(offsets[i]);
    if (p == kNoPageId) return false;
    for (const Row &row : rows_) {
      if (row.r->mapped[row.first + p] != Unbacked) return false;
      need_epoch = std::max(need_epoch, row.r->stale_epoch[row.first + p]);
    }
    if (!scan.add(rows_[0].r, rows_[0].first + p)) return false;
  }
  GpuContext *ctx = ctx_;
  ctx->bind();
  ExtentPool *pool = lane_pool_;
  if (!ctx->primary_pool()) ctx->set_primary_pool(pool);
  const bool fill = options().zero_fill.load() != 0;
  if (vmm_hip_registered()) // once per slot (a rest_direct region did it when it was made)
    for (size_t i = 0; i < n; ++i)
      for_rows(page_id_of(offsets[i]), [&](KvRegion &reg, size_t idx) {
        if (reg.registered[idx]) return;
        const int64_t t0 = now_ns();
        register_slot(reg, idx);
        stats().t_unmap_alias += now_ns() - t0;
      });
  sg.mark(kSegMapClassify);
  const std::vector<SlotRun> runs = scan.collect();
  stats().seg[kSegMapRunCount] += (int64_t)runs.size();
  sg.mark(kSegMapRuns);

  struct Chunk {
    size_t p, k, rows_done;
    bool settled; // the slots name the lanes
    Phys lane[kMaxLanesPerBuffer];
  };
  std::vector<Chunk> done;
  std::vector<void *> pending;
  uint64_t max_ticket = 0;
  size_t prescrubbed = 0, ids = 0;
  bool launched = false;
  RowsSplit split;
  try {
    for (const SlotRun &run : runs) {
      for (size_t at = run.first - rows_[0].first, end = at + run.count; at < end;) {
        done.emplace_back();
        Chunk &c = done.back();
        c.p = at;
        c.k = c.rows_done = 0;
        c.settled = false;
        const int64_t t1 = now_ns();
        c.k = acquire_pages(pool, end - at, c.lane, /*stolen=*/nullptr); // (a stolen page is not a lane)
        const int64_t t2 = now_ns();
        sg.mark(kSegMapPool);
        unsigned j0 = 0, ke = 1;
        void *bo = vmm_direct_bo(c.lane[0].h, &j0, &ke);
        if (!bo) throw GpuError("a lane's buffer is not a direct DRM buffer");
        if (const int rc = back_rows(bo, j0, ke, at, c.k, split, c.rows_done))
          throw GpuError(std::string("DRM_AMDGPU_GEM_VA (backing a page id) failed: ") + strerror(rc < 0 ? -rc : rc));
        stats().seg[kSegMapIoctlCount] += (int64_t)R;
        stats().t_acquire += t2 - t1;
        stats().t_map += now_ns() - t2;
        sg.mark(kSegMapIoctls);
        for (size_t j = 0; j < c.k; ++j) {
          max_ticket = std::max(max_ticket, c.lane[j].wait_ticket);
          const bool clean = fill && c.lane[j].scrub_ticket != 0;
          if (clean) {
            max_ticket = std::max(max_ticket, c.lane[j].scrub_ticket);
            prescrubbed += R;
          }
          for_rows(at + j, [&](KvRegion &reg, size_t idx) {
            reg.handle[idx] = c.lane[j].h;
            reg.seq[idx] = c.lane[j].seq;
            reg.mapped[idx] = Lane;
            if (fill && !clean) pending.push_back(reg.base + idx * ps);
          });
        }
        c.settled = true;
        ids += c.k;
        at += c.k;
        sg.mark(kSegMapBookkeeping);
      }
    }
    // (no flush happens between the REPLACEs of this path, so they are all noted here, once)
    settle_batch(ctx, ps, split.prt_dirty, split.zx_dirty, need_epoch, split.replaced || options().map_shootdown_always.load() != 0);
    sg.mark(kSegMapInvalidation);
    const int64_t ts = now_ns();
    for (size_t i = 0; i < pending.size(); i += kMaxPtrsPerLaunch) { // fresh memory, or pages that came back unscrubbed
      ctx->zero_fill(pending.data() + i, std::min<size_t>(kMaxPtrsPerLaunch, pending.size() - i), ps, nullptr);
      launched = true;
    }
    if (launched) ctx->sync(nullptr);
    sg.mark(kSegMapWaitFill);
    ctx->wait_scrub(max_ticket);
    stats().t_sync += now_ns() - ts;
    sg.mark(kSegMapWaitScrub);
  } catch (...) {
    roll_back(ctx, launched, [&]() {
      for (auto it = done.rbegin(); it != done.rend(); ++it) {
        undo_rows(it->p, it->k, it->rows_done, it->settled,
                  [&](KvRegion &reg, size_t first) { (void)vmm_try_unmap(reg.base + first * ps, it->k * ps, it->lane[0].h); });
        if (it->k) pool->release_batch(it->lane, it->k);
      }
    });
    throw;
  }
  stats().pages_mapped += (int64_t)(ids * R);
  if (prescrubbed) stats().pages_prescrubbed += (int64_t)prescrubbed;
  if (pool->creations() > 0) cold_start_reserve(pool);
  return true;
}

size_t KvAllocator::unmap_lanes(const offset_t *offsets, size_t n, std::vector<offset_t> *others) {
  const size_t R = rows_.size(), ps = rows_[0].r->page_size;
  SegTimer sg;
  RunScan scan;
  for (size_t i = 0; i < n; ++i) {
    const size_t p = page_id_of(offsets[i]);
    const uint8_t state = p != kNoPageId ? rows_[0].r->mapped[rows_[0].first + p] : Unbacked;
    if (state == Lane || state == PeerLane) {
      if (!scan.add(rows_[0].r, rows_[0].first + p)) KVC_LOG(LOG_ERROR, "Page %zu is not mapped.", p); // named twice
    } else {
      others->push_back(offsets[i]);
    }
  }
  if (!scan.size()) return 0;
  GpuContext *ctx = ctx_;
  ctx->bind();
  ExtentPool *pool = lane_pool_;
  const std::vector<SlotRun> runs = scan.collect();
  sg.mark(kSegUnmapRuns);
  Unmapped u; // own: the lanes that go home
  u.pool = pool;
  u.rows = R;
  u.page_size = ps;
  std::vector<phys_handle_t> peers_buffers; // page ids that were backed by a peer's lane: its buffer is released once, after the invalidation
  KeyGroups<uint32_t> touched(n); // buffer -> lanes of it that this call takes back
  for (const SlotRun &run : runs) {
    const size_t p0 = run.first - rows_[0].first;
    for (size_t r = 0; r < R; ++r) {
      KvRegion &reg = *rows_[r].r;
      const int64_t t0 = now_ns();
      if (reg.rest_direct()) { // back to the rest state, whatever is mapped there, in one ioctl per piece
        for_rest_pieces(reg, rows_[r].first + p0, run.count, [&](size_t first, size_t cnt) {
          const int rc = rest_replace(reg, first, cnt);
          if (rc != 0) throw GpuError(std::string("DRM_AMDGPU_GEM_VA replace (back to the rest state) failed: ") + strerror(rc < 0 ? -rc : rc));
          stats().seg[kSegUnmapIoctlCount]++;
        });
        u.any_backfilled = u.any_backfilled || reg.backfilled;
      } else {
        vmm_unmap_run(reg.base + (rows_[r].first + p0) * ps, run.count * ps);
        stats().seg[kSegUnmapIoctlCount]++;
      }
      stats().t_unmap += now_ns() - t0;
    }
    for (size_t p = p0; p < p0 + run.count; ++p) {
      const size_t idx0 = rows_[0].first + p;
      const phys_handle_t h = rows_[0].r->handle[idx0];
      if (rows_[0].r->mapped[idx0] == PeerLane) {
        peers_buffers.push_back(h);
        continue;
      }
      u.own.push_back(Phys{h, rows_[0].r->seq[idx0]});
      ++touched.at(chunk_of(h));
    }
  }
  sg.mark(kSegUnmapIoctls);
  for (const SlotRun &run : runs)
    for_rows(run.first - rows_[0].first, [&](KvRegion &reg, size_t first) { std::fill(reg.mapped.begin() + first, reg.mapped.begin() + first + run.count, Unbacked); });
  sg.mark(kSegUnmapBookkeeping);
  // Lanes that were backed together share one mapping per row; taking some of them out splits it, and what is left of it
  // must be written again before the invalidation (DrmVm::refresh_mappings_of, §4.8). A buffer that loses ALL its mapped
  // lanes here leaves nothing behind.
  if (!KVC_TEST_HOOK("SKIP_REMAINDER_REFRESH")) {
    bool any = false;
    for (auto &kv : touched.items())
      if (pool->pieces_out(kv.first) > kv.second)
        if (void *bo = DrmVm::instance().find(kv.first)) {
          if (!DrmVm::instance().refresh_mappings_of(bo, ps)) KVC_LOG(LOG_ERROR, "rewriting the remaining mappings of a buffer failed");
          any = true;
        }
    if (any) tlb_stale().store(true);
  }
  sg.mark(kSegUnmapRemainders);
  const uint64_t epoch = u.epoch = ctx->next_flush_epoch(); // every driver call that removed or rewrote a translation has returned
  for (const SlotRun &run : runs)
    for_rows(run.first - rows_[0].first, [&](KvRegion &reg, size_t first) { std::fill(reg.stale_epoch.begin() + first, reg.stale_epoch.begin() + first + run.count, epoch); });
  sg.mark(kSegUnmapEpochs);
  // a peer's memory: no translation of it may survive the call (one entry per page id: the buffer goes - behind the
  // invalidation - when the last page id it backs here has gone)
  u.foreign = !peers_buffers.empty();
  for (auto h : peers_buffers) {
    auto it = peer_refs_.find(h);
    if (it != peer_refs_.end() && --it->second > 0) continue;
    if (it != peer_refs_.end()) peer_refs_.erase(it);
    u.imported.push_back(h);
  }
  const size_t n_ids = u.own.size() + peers_buffers.size();
  u.n = (int64_t)(n_ids * R);
  unmap_finish(u, true); // the invalidation: inside the call where unbacked VA promises zeros (compat), behind it otherwise
  return n_ids;
}

int KvAllocator::export_page_ids(const offset_t *offsets, size_t n, int *out_fds, int64_t *out_meta, int64_t cap) {
  std::lock_guard<std::mutex> g(mu_);
  if (!dev_.is_gpu) throw NoGpuError("export_page_ids needs a GPU device");
  if (!lanes_) throw InvalidError("page ids are not backed as units here (kvc_get_option(129) == 0): export slot by slot");
  if ((int64_t)n > cap) return (int)n;
  const size_t ps = rows_[0].r->page_size;
  for (size_t i = 0; i < n; ++i) { // nothing is exported unless everything can be
    const size_t p = page_id_of(offsets[i]);
    if (p == kNoPageId || rows_[0].r->mapped[rows_[0].first + p] != Lane)
      throw InvalidError("export of a page id that is not backed by a lane of this process");
  }
  ctx_->bind();
  KeyGroups<int> bufs(n); // buffer -> its place among the exported fds (order of first appearance)
  int k = 0;
  try {
    for (size_t i = 0; i < n; ++i) {
      const phys_handle_t h = rows_[0].r->handle[rows_[0].first + (size_t)offsets[i] / ps];
      const size_t before = bufs.items().size();
      int &at = bufs.at(chunk_of(h));
      if (bufs.items().size() != before) { // first page id of this buffer: export it (AMDKFD_IOC_EXPORT_DMABUF)
        const int fd = DrmVm::instance().export_fd(chunk_of(h));
        if (fd < 0) throw GpuError("a lane's buffer cannot be exported");
        out_fds[k] = fd;
        at = k++;
      }
      out_meta[3 * i] = at;
      out_meta[3 * i + 1] = (int64_t)pages_of(h);
      out_meta[3 * i + 2] = (int64_t)piece_of(h);
    }
  } catch (...) {
    for (int i = 0; i < k; ++i) ::close(out_fds[i]);
    throw;
  }
  return k;
}

bool KvAllocator::map_imported_page_ids(const offset_t *offsets, size_t n, const int *fds, size_t n_fds, const int64_t *meta) {
  std::lock_guard<std::mutex> g(mu_);
  if (!dev_.is_gpu) throw NoGpuError("map_imported_page_ids needs a GPU device");
  if (num_layers_ == 0) return false;
  if (rows_.empty()) throw InvalidError("page ids cannot be imported as units here (single-row geometry or not the drm backend): import slot by slot");
  if (!n) return true;
  const size_t R = rows_.size(), ps = rows_[0].r->page_size;
  struct Id {
    size_t p;
    uint64_t buf, k, j;
  };
  std::vector<Id> ids(n);
  for (size_t i = 0; i < n; ++i) {
    const size_t p = page_id_of(offsets[i]);
    if (p == kNoPageId) throw InvalidError("offset " + std::to_string(offsets[i]) + " is not a page id of this geometry");
    const int64_t b = meta[3 * i], k = meta[3 * i + 1], j = meta[3 * i + 2];
    if (b < 0 || (size_t)b >= n_fds || k < 1 || k > (int64_t)kMaxLanesPerBuffer || j < 0 || j >= k)
      throw InvalidError("import of a page id: (fd " + std::to_string(b) + ", lane " + std::to_string(j) + " of " + std::to_string(k) + ") names no lane of the buffers that came along");
    ids[i] = Id{p, (uint64_t)b, (uint64_t)k, (uint64_t)j};
    for (const Row &row : rows_)
      if (row.r->mapped[row.first + ids[i].p] != Unbacked) throw InvalidError("import into a page id that is backed already");
  }
  std::sort(ids.begin(), ids.end(), [](const Id &a, const Id &b) { return a.p < b.p; });
  for (size_t i = 1; i < n; ++i)
    if (ids[i].p == ids[i - 1].p) throw InvalidError("import of a page id that is named twice");
  GpuContext *ctx = ctx_;
  ctx->bind();
  DrmVm &vm = DrmVm::instance();
  if (!vm.kfd_ready()) throw InvalidError("importing page ids as units needs the drm backend with pages straight from KFD");
  std::vector<phys_handle_t> bufs(n_fds, 0);
  struct Done {
    size_t p, cnt, rows_done;
    phys_handle_t h;
    bool settled;
  };
  std::vector<Done> done;
  RowsSplit split;
  uint64_t need_epoch = 0;
  try {
    for (size_t f = 0; f < n_fds; ++f) { // AMDKFD_IOC_IMPORT_DMABUF + DRM import, once per buffer
      bufs[f] = vm.import_fd(fds[f]);
      ++g_imports_direct;
    }
    for (size_t i = 0; i < n;) {
      size_t cnt = 1; // page ids that are neighbours here AND in one buffer: one ioctl per row
      while (i + cnt < n && ids[i + cnt].p == ids[i].p + cnt && ids[i + cnt].buf == ids[i].buf && ids[i + cnt].k == ids[i].k &&
             ids[i + cnt].j == ids[i].j + cnt)
        ++cnt;
      const Id &first = ids[i];
      done.push_back(Done{first.p, cnt, 0, bufs[first.buf], false});
      Done &d = done.back();
      void *bo = vm.find(d.h);
      if (!bo) throw GpuError("an imported buffer is not a direct DRM buffer");
      for_rows(first.p, [&](KvRegion &reg, size_t idx) { // (HIP hears of every slot of the run before any of its rows is backed)
        for (size_t c = 0; c < cnt; ++c) {
          if (vmm_hip_registered() && !reg.registered[idx + c]) register_slot(reg, idx + c);
          need_epoch = std::max(need_epoch, reg.stale_epoch[idx + c]);
        }
      });
      if (const int rc = back_rows(bo, first.j, first.k, first.p, cnt, split, d.rows_done))
        throw GpuError(std::string("DRM_AMDGPU_GEM_VA (mapping a peer's page ids) failed: ") + strerror(rc < 0 ? -rc : rc) +
                       " - does the buffer hold " + std::to_string(first.k) + " lanes of " + std::to_string(R) + " pages?");
      for_rows(first.p, [&](KvRegion &reg, size_t idx) {
        std::fill(reg.handle.begin() + idx, reg.handle.begin() + idx + cnt, d.h);
        std::fill(reg.seq.begin() + idx, reg.seq.begin() + idx + cnt, 0);
        std::fill(reg.mapped.begin() + idx, reg.mapped.begin() + idx + cnt, PeerLane);
      });
      d.settled = true;
      stats().seg[kSegMapIoctlCount] += (int64_t)R;
      i += cnt;
    }
    settle_batch(ctx, ps, split.prt_dirty, split.zx_dirty, need_epoch, split.replaced);
  } catch (...) {
    roll_back(ctx, /*launched=*/false, [&]() {
      for (auto it = done.rbegin(); it != done.rend(); ++it)
        undo_rows(it->p, it->cnt, it->rows_done, it->settled,
                  [&](KvRegion &reg, size_t first) { (void)vm.clear(reg.base + first * ps, it->cnt * ps); });
    });
    for (auto h : bufs)
      if (h) (void)vmm_try_release(h);
    throw;
  }
  for (const Id &id : ids) ++peer_refs_[bufs[id.buf]];
  for (auto h : bufs) // (an fd that came along but backs none of the page ids)
    if (h && !peer_refs_.count(h)) (void)vmm_try_release(h);
  stats().pages_mapped += (int64_t)(n * R);
  return true;
}

} // namespace kvc
