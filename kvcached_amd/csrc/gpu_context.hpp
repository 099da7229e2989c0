// gpu_context.hpp — process-wide statistics (the options: options.hpp), and the per-device state of the allocator (implemented in
// gpu_context.cpp): streams, kernel launches, the physical pools, the alias arena and the scrub queue, the zero extent,
// the TLB invalidation with its epochs.
#pragma once

#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "hip_vmm.hpp"
#include "options.hpp"

namespace kvc {

static_assert(kMaxChunkPages == kMaxExtentPages, "the option table's bound is the extent pool's");

struct Stats {
  std::atomic<int64_t> pages_mapped{0}, pages_unmapped{0};
  std::atomic<int64_t> map_calls{0}, unmap_calls{0}, map_ns{0}, unmap_ns{0};
  std::atomic<int64_t> fill_launches{0}, fill_bytes{0};
  std::atomic<int64_t> compact_launches{0}, compact_bytes{0};
  std::atomic<int64_t> tlb_shootdowns{0}, shootdown_ns{0};
  std::atomic<int64_t> index_launches{0};
  std::atomic<int64_t> pages_scrubbed{0}, pages_prescrubbed{0}; // zeroed on their way back / handed out without a fill of their own (options 125, 126)
  std::atomic<int64_t> unmaps_queued{0}, unmaps_cancelled{0}; // async unmap: slots queued / re-backed before the reclaimer got to them
  // host time inside each driver call of the map/unmap paths (diagnostics; kvc_get_driver_breakdown)
  std::atomic<int64_t> t_unmap_alias{0}, t_acquire{0}, t_map{0}, t_access{0}, t_unmap{0}, t_release{0}, t_realias{0}, t_sync{0};
  // host time of the map / unmap calls by segment (diagnostics, read-only options KVC_OPT_HOST_SEGMENT_0 + i; enum Seg)
  std::atomic<int64_t> seg[kSegCount] = {};
  std::mutex mu;
  double fill_ms = 0, compact_ms = 0;
  VmmCounters vmm;
  void reset();
};
Stats &stats();
struct SegTimer { // accumulates the time since the previous mark into stats().seg[i]
  int64_t t = now_ns();
  void mark(Seg i) {
    const int64_t n = now_ns();
    stats().seg[i] += n - t;
    t = n;
  }
};
std::atomic<int64_t> &background_shootdowns(); // TLB invalidations performed off the callers' threads (option 111)

// Per-device state: stream for our kernels, event pool for per-launch timing, handle pools.
class GpuContext {
public:
  explicit GpuContext(int dev);
  ~GpuContext();
  int dev() const { return dev_; }
  void bind() const; // hipSetDevice for the calling thread (HIP's current device is per thread)
  hipStream_t stream() const { return stream_; }
  // What map/unmap take pages from (extent_pool.hpp): run-sized extents of up to KVCACHED_PHYS_CHUNK_PAGES pages with
  // the drm backend and pages straight from KFD (non-exportable pools), single pages everywhere else.
  ExtentPool *extents(size_t page_bytes, bool exportable);
  // The pool of an allocator whose page ids are `rows` slots in `rows` places of the address space (one per layer and K/V
  // half: the non-contiguous layout engines use on ROCm): its unit is a LANE - the `rows` pages behind one page id - and an
  // extent is one buffer of up to KVCACHED_LANE_EXTENT_MB holding k lanes row-major (page (row, lane) at (row * k + lane)),
  // so that k consecutive page ids are ONE map ioctl per row and a page id is acquired, scrubbed and released as a unit
  // (DESIGN.md §4.11). drm backend with pages straight from KFD only (nullptr otherwise).
  ExtentPool *lane_extents(size_t rows, size_t page_bytes);
  // the pool the engine's own pages come from (the reserve and the footprint diagnostics belong to it)
  void set_primary_pool(ExtentPool *p) { primary_pool_.store(p); }
  ExtentPool *primary_pool() const { return primary_pool_.load(); }
  void drain_pools();
  size_t idle_pool_bytes(); // physical memory parked in the handle pools: ours to reuse, invisible to hipMemGetInfo
  // 10 Hz from the allocator's watcher thread: drain idle handles if the device is short of free memory, and
  // let handles that sat idle for KVCACHED_POOL_IDLE_MS go back to the driver (ExtentPool::decay), keep the reserve filled
  void housekeeping();
  // a thread that calls housekeeping() periodically exists / is gone (PageAllocator's watcher): while one does,
  // pools hand over-cap handles to it instead of releasing them on the caller's free() path
  void add_housekeeper(int delta);
  bool has_housekeeper() const { return housekeepers_.load() > 0; }

  // kernel launches on `s` (NULL = own stream), timed with events when profiling is on
  void zero_fill(void *const *pages, size_t n, size_t page_bytes, hipStream_t s);
  void compact(void *const *bases, size_t n_regions, const int64_t *src, const int64_t *dst, size_t n_moves,
               size_t block_bytes, hipStream_t s);
  // blocks <-> a block-major host image (copy_blocks_to_host / _from_host, or encode_ / decode_ with a codec: HostCodec of
  // kernels.hpp); `host` is a device address of pinned memory. With `slots`, block i's row of the image is row slots[i] of
  // the arena at `host` (launch_copy_blocks_host_slots) instead of row i.
  void copy_blocks_host(bool to_host, void *const *bases, size_t n_regions, const int64_t *ids, size_t n, size_t block_bytes,
                        void *host, hipStream_t s, int codec = 0, const int64_t *slots = nullptr);
  void sync(hipStream_t s); // hipStreamSynchronize + harvest event timings
  // ---- zeroing pages on their way BACK (drm backend, extents with an alias mapping).
  // A page handed out by map_slots must read zero. Filling it there puts 0.3 us per page of GPU time between the
  // driver calls and the caller; filling it when it is given back - through a second, permanent mapping of its buffer
  // that only the library knows, on a stream of its own - lets that run while the host does whatever comes next.
  // scrub(): launches the fill on the given alias addresses (0 = skip) and returns its ticket; wait_scrub(t): returns
  // once scrub t has finished (no-op if it has). Tickets are issued in launch order on one stream.
  uint64_t scrub(const uint64_t *alias_addrs, size_t n, size_t page_bytes);
  void wait_scrub(uint64_t ticket);
  void wait_all_scrubs() { wait_scrub(scrub_issued_.load()); }
  uint64_t scrubs_issued() const { return scrub_issued_.load(); }
  // VA for alias mappings (never handed to anybody): carved from arenas reserved 64 GiB at a time
  uint64_t alias_alloc(size_t bytes);
  void alias_free(uint64_t va, size_t bytes);
  // The buffer of zeros behind the unbacked slots of compat-mode regions (drm backend): created and filled on first use,
  // `*pages` pages of `page_bytes`; 0 if it cannot be had (the caller aliases sharded zero pages through ROCr instead).
  phys_handle_t zero_extent(size_t page_bytes, size_t *pages);
  size_t zero_extent_pages(size_t page_bytes); // of the one that exists (0: none was needed)
  // block id <-> token index glue (index_kernels.hip); ids are HOST arrays, everything else device memory
  void expand_block_ids(const int64_t *ids, size_t n, int64_t tpb, int64_t *out, hipStream_t s);
  void alloc_extend_indices(const int64_t *pre_lens, const int64_t *seq_lens, const int64_t *last_loc, size_t bs,
                            const int64_t *ids, size_t n_ids, int64_t tpb, int64_t *out, size_t out_len, hipStream_t s);
  void alloc_decode_indices(const int64_t *seq_lens, const int64_t *last_loc, size_t bs, const int64_t *ids, size_t n_ids,
                            int64_t tpb, int64_t *out, hipStream_t s);
  // blocking: distinct blocks of `n` device token indices, ascending, into out_host; returns the count
  int64_t unique_block_ids(const int64_t *idx, size_t n, int64_t tpb, int64_t n_blocks, int64_t *out_host, size_t cap,
                           hipStream_t s);
  // Make the driver invalidate this GPU's TLBs. hipMemMap/hipMemUnmap/hipMemSetAccess do not do it
  // on ROCm 7.2 (stale translations survive a remap: kvcached_amd/csrc/tools/remap_diag.cpp); KFD's unmap ioctl does:
  // issued directly on a buffer of our own (KfdTlbFlush, drm_vm.hpp), or - where /dev/kfd cannot be used that way -
  // through an ordinary >= 2 MiB hipMalloc + hipFree. KvAllocator::init proves on a scratch slot that whichever is
  // in effect really invalidates, and refuses to start otherwise.
  void tlb_shootdown();
  bool kfd_flush_active() const { return kfd_flush_.ready(); }
  // unmap path: the invalidation is owed but nothing needs it yet (see KvAllocator::unmap_slots)
  void defer_tlb_shootdown() { tlb_stale().store(true); }
  bool tlb_owed() const { return tlb_stale().load(); } // some unmap since the last invalidation (hip_vmm.hpp)
  // Invalidate if (and only if) an unmap has happened since the last invalidation; a caller that arrives while
  // another thread's invalidation is in flight waits for it instead of issuing a second one.
  void ensure_flushed();
  void flush_deferred_shootdown() { ensure_flushed(); }
  // Invalidations are numbered. A translation removed NOW is covered by the first invalidation that starts from now on:
  // next_flush_epoch() (read after the driver's unmap call has returned) is its number, and flushed_through(e) says
  // whether that one has finished. A map batch only has to wait for the invalidations that cover ITS slots
  // (KvRegion::stale_epoch) - a stale translation of some other address cannot shadow a mapping made here.
  uint64_t next_flush_epoch() const { return flush_started_.load() + 1; }
  bool flushed_through(uint64_t epoch) const { return flush_done_.load() >= epoch; }
  void ensure_flushed_through(uint64_t epoch);
  // Have this context's own thread do ensure_flushed() right away (started on first use): the unmap path's 0.3-0.5 ms
  // KFD round trip leaves the caller's free(); whoever needs the invalidation earlier (the next map batch before
  // its first fill, a handle leaving for the driver) calls ensure_flushed() and waits for it or performs it.
  void request_async_flush(int64_t within_us = 0); // within_us > 0: at the latest that many microseconds from now, foreground calls or not
  // ---- pages in limbo: unmapped, their invalidation still owed (KVCACHED_UNMAP_INVALIDATION_US). `finish` scrubs them and
  // gives them back to their pool; it runs - on whatever thread completed an invalidation numbered >= epoch - strictly after
  // that invalidation: a page is never zeroed nor on offer while a stale translation of it can exist.
  void park(uint64_t epoch, size_t bytes, std::function<void()> finish);
  void drain_limbo();                       // runs the finishers whose invalidation is over
  void flush_limbo();                       // invalidates if anything is parked, then drains
  size_t limbo_bytes() const { return limbo_bytes_.load(); }
  // The idle memory the primary pool is kept at: KVCACHED_PHYS_RESERVE_MB (never above the pool's cap) plus - where unmaps park
  // their pages - the most that was parked at once during the last second (at most the base again): parked pages are in transit,
  // and a reserve of exactly one batch next to a parked batch leaves the next map call on the edge of having to invalidate for
  // them itself.
  size_t reserve_target_bytes() const;
  // a map / unmap call of an allocator is in progress (or was a moment ago): the background invalidation waits its turn
  struct Foreground {
    GpuContext *c;
    explicit Foreground(GpuContext *ctx) : c(ctx) {
      if (c) c->fg_active_.fetch_add(1);
    }
    ~Foreground() {
      if (c) {
        c->fg_last_ns_.store(now_ns());
        c->fg_active_.fetch_sub(1);
      }
    }
  };
  bool foreground_busy() const { return fg_active_.load() > 0 || now_ns() - fg_last_ns_.load() < 150000; }

private:
  struct Timed {
    hipEvent_t a, b;
    int kind; // 0 fill, 1 compact
  };
  void begin_timed(hipStream_t s, int kind);
  void end_timed(hipStream_t s);
  void harvest();
  void flusher_loop();
  void do_shootdown(); // needs flush_mu_
  int dev_;
  hipStream_t stream_ = nullptr;
  std::mutex flush_mu_; // serialises TLB invalidations
  std::atomic<uint64_t> flush_started_{0}, flush_done_{0};
  std::atomic<int> fg_active_{0};
  std::atomic<int64_t> fg_last_ns_{0};
  std::thread flusher_;
  std::mutex fl_mu_;
  std::condition_variable fl_cv_;
  bool fl_stop_ = false, fl_kick_ = false;
  int64_t fl_deadline_ns_ = 0; // (under fl_mu_) the async flush must have started by then (0: when the foreground is quiet)
  struct Parked {
    uint64_t epoch;
    size_t bytes;
    std::function<void()> finish;
  };
  std::mutex limbo_mu_;
  std::deque<Parked> limbo_;
  std::atomic<size_t> limbo_bytes_{0};
  static constexpr int kLimboTicks = 10;
  std::atomic<size_t> limbo_peak_[kLimboTicks] = {}; // per housekeeping tick (one slot for ever where no thread ticks)
  std::atomic<unsigned> limbo_tick_{0};
  std::atomic<int> housekeepers_{0};
  std::mutex mu_;
  std::unordered_map<size_t, std::unique_ptr<ExtentPool>> extent_pools_[2]; // [exportable], key: page bytes
  std::map<std::pair<size_t, size_t>, std::unique_ptr<ExtentPool>> lane_pools_; // key: (rows, page bytes)
  std::atomic<ExtentPool *> primary_pool_{nullptr};
  // the reserve follows demand (housekeeping(), one thread): units created on callers' paths per tick over the last second
  std::mutex hk_mu_;
  static constexpr size_t kDemandTicks = 10;
  ExtentPool *demand_pool_ = nullptr;
  size_t demand_seen_ = 0, demand_window_[kDemandTicks] = {}, demand_tick_ = 0, demand_quiet_ticks_ = 0, reserve_boost_units_ = 0;
  ExtentDriver make_driver(size_t unit_bytes, bool exportable, bool aliases);
  std::vector<ExtentPool *> all_pools();
  KfdTlbFlush kfd_flush_;
  void *fallback_block_ = nullptr; // the 2 MiB allocation whose hipFree is the next invalidation of the hipMalloc/hipFree fallback
  hipStream_t scrub_stream_ = nullptr;
  std::mutex scrub_mu_; // launch order = ticket order
  std::atomic<uint64_t> scrub_issued_{0}, scrub_done_{0};
  std::deque<std::pair<uint64_t, hipEvent_t>> scrub_events_; // (ticket, recorded behind its launch), ascending; under scrub_mu_
  std::vector<hipEvent_t> scrub_free_events_;
  void retire_scrubs_locked(uint64_t through); // entries <= through are over
  struct Arena {
    char *base;
    size_t size, used;
  };
  std::mutex arena_mu_;
  std::vector<Arena> arenas_;
  std::map<size_t, std::vector<uint64_t>> alias_free_; // by size: extents come in a handful of sizes
  std::vector<std::pair<uint64_t, size_t>> alias_limbo_; // alias addresses whose mapping is gone but not yet invalidated (arena_mu_)
  struct ZeroExtent {
    phys_handle_t h;
    size_t pages;
    uint64_t alias;
  };
  std::mutex zero_mu_;
  std::map<size_t, ZeroExtent> zero_extents_; // by page size
  std::vector<Timed> inflight_;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> free_events_;
  // unique_block_ids scratch (grow-only; bitmap all-zero and header reset between calls)
  std::mutex uniq_mu_;
  unsigned *uniq_bitmap_ = nullptr;
  size_t uniq_words_ = 0;
  void *uniq_header_ = nullptr;
  int64_t *uniq_result_ = nullptr; // pinned host memory the sweep kernel writes into
  size_t uniq_result_cap_ = 0;     // entries, including the count
  void reset_unique_scratch();
};

} // namespace kvc
