// kv_allocator.cpp — see kv_allocator.hpp. The registry and the lifetime of allocators, the reclaimer thread and quiesce,
// the KV tensors and the map/unmap entry points. The paths behind them: kv_regions.cpp, kv_map_paths.cpp, kv_lanes.cpp,
// kv_share.cpp; the self tests of init(): kv_selftest.cpp.
#include "kv_allocator_impl.hpp"

#include <algorithm>

namespace kvc {

namespace {
std::mutex g_mu; // guards the registry below
// Never destroyed: a process that ends without kvc_shutdown() must not tear GPU state down from static destructors -
// the HIP runtime, ROCr and libdrm are going away in an unspecified order at that point (that crashed at exit); the
// kernel reclaims mappings and memory with the process. The Python module shuts down in an atexit hook, in good time.
auto &g_allocators = *new std::unordered_map<int64_t, std::unique_ptr<KvAllocator>>;
auto &g_contexts = *new std::unordered_map<int, std::unique_ptr<GpuContext>>;
DeviceSpec g_device;
bool g_contiguous = false;
bool g_initialized = false;
size_t g_page_size = kBasePage;
std::atomic<size_t> g_override_free{0}, g_override_total{0};

int resolve_dev_index(const DeviceSpec &d) {
  if (d.index >= 0) return d.index;
  int cur = 0;
  HIP_CHECK(hipGetDevice(&cur));
  return cur;
}

GpuContext *context_for(int dev) {
  auto it = g_contexts.find(dev);
  if (it == g_contexts.end()) it = g_contexts.emplace(dev, std::make_unique<GpuContext>(dev)).first;
  return it->second.get();
}
} // namespace
std::atomic<size_t> g_vaddr_offset{0}; // running offset behind kStartAddr (reference: ftensor.cpp:17)
std::atomic<size_t> g_pending_unmap_bytes{0}; // async unmap: released by the caller, not yet by the driver

// ------------------------------------------------------------------ registry
void KvAllocator::init(const std::string &dev_str, size_t page_size, bool contiguous_layout) {
  std::unordered_map<int64_t, std::unique_ptr<KvAllocator>> old; // destroyed after g_mu is released
  std::unique_lock<std::mutex> g(g_mu);
  const DeviceSpec want_dev = parse_device(dev_str);
  if (!g_allocators.empty()) {
    // One device per process (as in the reference: one FTensorAllocator multiton, allocator.cpp:18-22). Re-initialising
    // for the SAME device re-creates the allocators like the reference does (allocator.cpp:75-78); asking for another
    // device while KV tensors of the first one exist would pull the driver state (DrmVm, pooled pages) from under them.
    const bool other_device = want_dev.is_gpu != g_device.is_gpu ||
                              (want_dev.is_gpu && want_dev.index >= 0 && want_dev.index != g_device.index);
    if (other_device) {
      bool live = false;
      for (auto &kv : g_allocators) live = live || kv.second->kv_tensors_created();
      if (live)
        throw InvalidError("init_kvcached(\"" + dev_str + "\") while KV tensors of " +
                           (g_device.is_gpu ? "cuda:" + std::to_string(g_device.index) : std::string("cpu")) +
                           " exist: one device per process - call shutdown_kvcached() first");
    }
    KVC_LOG(LOG_ERROR, "KvAllocator has been initialized. Re-initializing...");
    old.swap(g_allocators);
    g_initialized = false; // until this init has succeeded
    g.unlock();
    old.clear();
    g.lock();
    if (other_device) { // nothing of the old device may linger in pools that DrmVm::open() is about to invalidate
      std::unordered_map<int, std::unique_ptr<GpuContext>> ctxs;
      ctxs.swap(g_contexts);
      g.unlock();
      for (auto &kv : ctxs) kv.second->drain_pools();
      ctxs.clear();
      g.lock();
    }
  }
  if (page_size > 0) {
    if (page_size % kBasePage != 0) // reference aborts here (allocator.cpp:84-90); we report it
      throw InvalidError("Invalid page size: " + std::to_string(page_size) +
                         ", must be a multiple of 2MB (2097152 bytes)");
    g_page_size = page_size;
  }
  // environment knobs, read once per init: one row each in options.cpp.
  // KVCACHED_ZERO_BACKFILL is ON by default since round 2, as in the reference (csrc/ftensor.cpp:160-176: unbacked VA reads as
  // zeros instead of faulting). Round 1 had it off: with per-slot aliases through ROCr every creation cost O(mappings in the
  // process) and the cycle ran at 160 GB/s; with the drm backend's zero extent (backfill_all) it is 1.5 TB/s and start-up is
  // 2 304 ioctls for a 288 GiB reservation. =false ("lazy": unbacked VA stays unmapped, a stray access FAULTS) is the opt-in
  // for engines that never touch a block they do not own: 4.3 TB/s, no invalidation on the allocation path.
  load_options_from_env();
  {
    const std::string b = env_word("KVCACHED_VMM_BACKEND");
    if (b != "hip" && b != "hybrid" && b != "drm")
      throw InvalidError("KVCACHED_VMM_BACKEND must be 'drm', 'hybrid' or 'hip'");
    const int want = b == "hybrid" ? kVmmHybrid : (b == "drm" ? kVmmDrm : kVmmHip);
    // Pooled handles belong to the backend that made them; init's self tests may yet change the backend, and the
    // extent size may differ too: start every init with empty pools.
    for (auto &kv : g_contexts) kv.second->drain_pools();
    vmm_backend() = want;
  }
  g_device = want_dev;
  g_contiguous = contiguous_layout;
  if (g_device.is_gpu) {
    HIP_CHECK(hipInit(0));
    g_device.index = resolve_dev_index(g_device);
    GpuContext *ctx = context_for(g_device.index); // validates VMM support + granularity (reference: allocator.cpp:324-343)
    if (vmm_hip_registered() && !hybrid_self_test(g_device.index)) {
      KVC_LOG(LOG_WARNING, "hybrid VMM backend failed its self test on this HIP runtime: using the plain HIP backend "
                           "(KVCACHED_VMM_BACKEND=hip), map/unmap will be ~2x slower");
      vmm_backend() = kVmmHip;
    }
    if (vmm_backend() == kVmmDrm && !drm_self_test(g_device.index)) {
      KVC_LOG(LOG_WARNING, "direct DRM mapping failed its self test: using the hybrid backend (KVCACHED_VMM_BACKEND=hybrid)");
      DrmVm::instance().close();
      vmm_backend() = kVmmHybrid;
    }
    // Whatever backend is left standing: pages are only private if unmapping them really invalidates the GPU's TLBs.
    // No fallback for that - init fails.
    if (options().tlb_shootdown.load()) tlb_self_test(ctx);
  }
  g_allocators[0] = std::make_unique<KvAllocator>(g_device, contiguous_layout,
                                                  g_device.is_gpu ? context_for(g_device.index) : nullptr);
  g_initialized = true;
}

void KvAllocator::shutdown() {
  // Allocators unmap/release through their GpuContext and must not be destroyed under g_mu
  // (region teardown is slow, and nothing below may re-enter the registry); contexts go last.
  std::unordered_map<int64_t, std::unique_ptr<KvAllocator>> victims;
  {
    std::lock_guard<std::mutex> g(g_mu);
    victims.swap(g_allocators);
    g_initialized = false;
  }
  victims.clear();
  std::unordered_map<int, std::unique_ptr<GpuContext>> ctxs;
  {
    std::lock_guard<std::mutex> g(g_mu);
    if (g_allocators.empty()) ctxs.swap(g_contexts);
  }
  for (auto &kv : ctxs) kv.second->drain_pools();
  ctxs.clear();
}

KvAllocator *KvAllocator::global(int64_t group_id) {
  std::lock_guard<std::mutex> g(g_mu);
  auto it = g_allocators.find(group_id);
  if (it != g_allocators.end()) return it->second.get();
  if (g_allocators.empty()) throw InvalidError("KvAllocator::init() must be called first (init_kvcached)");
  // lazily created for an unseen group, with the device/layout of init() (allocator.cpp:101-114)
  auto &slot = g_allocators[group_id];
  slot = std::make_unique<KvAllocator>(g_device, g_contiguous, g_device.is_gpu ? context_for(g_device.index) : nullptr);
  return slot.get();
}

bool KvAllocator::initialized() {
  std::lock_guard<std::mutex> g(g_mu);
  return g_initialized;
}
DeviceSpec KvAllocator::device() { return g_device; }
size_t KvAllocator::page_size() { return g_page_size; }
GpuContext *KvAllocator::gpu() {
  std::lock_guard<std::mutex> g(g_mu);
  if (!g_initialized || !g_device.is_gpu) return nullptr;
  return context_for(g_device.index);
}

void mem_get_info(size_t *free_b, size_t *total_b) {
  size_t of = g_override_free.load(), ot = g_override_total.load();
  if (ot != 0) {
    *free_b = of;
    *total_b = ot;
    return;
  }
  GpuContext *ctx = KvAllocator::gpu();
  if (!ctx) throw NoGpuError("hipMemGetInfo needs a GPU device (init_kvcached with \"cuda:N\"), or a mem-info override");
  ctx->bind();
  HIP_CHECK(hipMemGetInfo(free_b, total_b));
  // What sits idle in our own handle pool is as good as free for this allocator (the reference would have
  // released it, csrc/page.cpp:17): without this, alloc() right after a large free() could be refused.
  *free_b = std::min(*total_b, *free_b + ctx->idle_pool_bytes() + g_pending_unmap_bytes.load());
}
void set_mem_info_override(size_t free_b, size_t total_b) {
  g_override_free = free_b;
  g_override_total = total_b;
}
void device_synchronize() {
  GpuContext *ctx = KvAllocator::gpu();
  if (!ctx) return;
  ctx->bind();
  HIP_CHECK(hipDeviceSynchronize());
}

// ------------------------------------------------------------------ KvAllocator
KvAllocator::KvAllocator(DeviceSpec dev, bool contiguous_layout, GpuContext *ctx)
    : dev_(dev), contiguous_(contiguous_layout), ctx_(ctx) {
  exportable_ = env_option("KVCACHED_EXPORTABLE_HANDLES") != 0;
}

KvAllocator::~KvAllocator() {
  if (reclaimer_.joinable()) {
    {
      std::lock_guard<std::mutex> g(mu_);
      reclaimer_stop_ = true;
    }
    pending_cv_.notify_all();
    reclaimer_.join();
  }
  std::lock_guard<std::mutex> g(mu_);
  size_t still_queued = 0;
  std::vector<Phys> lanes; // page ids still backed by lanes: their pages go home once every row is unmapped
  std::vector<phys_handle_t> peers_buffers; // ... and buffers of a peer that back page ids here: released once each
  if (!rows_.empty())
    for (size_t p = 0; p < ids_per_row_; ++p) {
      const size_t idx = rows_[0].first + p;
      if (rows_[0].r->mapped[idx] == Lane) lanes.push_back(Phys{rows_[0].r->handle[idx], rows_[0].r->seq[idx]});
      if (rows_[0].r->mapped[idx] == PeerLane) peers_buffers.push_back(rows_[0].r->handle[idx]);
    }
  for (auto &r : layers_) {
    for (auto m : r->mapped) still_queued += (m == UnmapQueued) ? r->page_size : 0;
    destroy_region(*r); // also unmaps what was still queued (UnmapQueued counts as mapped there)
  }
  g_pending_unmap_bytes -= std::min(still_queued, g_pending_unmap_bytes.load());
  layers_.clear();
  if (lane_pool_ && ctx_) {
    try {
      ctx_->ensure_flushed(); // (destroy_region has invalidated; a region that had nothing mapped owes nothing)
    } catch (...) {
      (void)hipGetLastError();
    }
    if (!lanes.empty()) lane_pool_->release_batch(lanes.data(), lanes.size());
    lane_pool_->drain(0); // an allocator that goes away gives its memory back (the reference releases in ~FTensor, ftensor.cpp:78-98)
  }
  std::sort(peers_buffers.begin(), peers_buffers.end());
  peers_buffers.erase(std::unique(peers_buffers.begin(), peers_buffers.end()), peers_buffers.end());
  for (auto h : peers_buffers) (void)vmm_try_release(h);
  peer_refs_.clear();
}

// ------------------------------------------------------------------ async unmap
// With KVC_OPT_ASYNC_UNMAP the caller's free() path only marks slots and queues them; this thread carries out the
// driver calls (hipMemUnmap is 15 us per slot, 1 ms for one page id of the Llama-3-8B geometry - time the
// scheduler thread of an engine would otherwise spend blocked). Bookkeeping stays synchronous, so page ids and
// block tables are unaffected. A slot that is backed again before its turn is simply kept (no driver call at
// all, just the zero fill). The driver serialises page-table updates per process, so this buys latency, not
// throughput: the reclaimer works in small chunks and yields to foreground map calls.
void KvAllocator::lock_foreground(std::unique_lock<std::mutex> &lk) {
  foreground_waiting_.fetch_add(1);
  lk.lock();
  foreground_waiting_.fetch_sub(1);
}

void KvAllocator::reclaimer_loop() {
  constexpr size_t kChunk = 128; // slots per critical section: <= 2 ms of driver calls between two chances to yield
  if (ctx_) {
    try {
      ctx_->bind();
    } catch (...) {
    }
  }
  std::unique_lock<std::mutex> lk(mu_);
  for (;;) {
    pending_cv_.wait(lk, [&] { return reclaimer_stop_ || !pending_.empty(); });
    if (reclaimer_stop_) return;
    std::vector<Slot> chunk;
    while (!pending_.empty() && chunk.size() < kChunk) {
      Slot s = pending_.front();
      pending_.pop_front();
      if (s.region->mapped[s.index] == UnmapQueued) { // still released (not re-backed, not already handled via a duplicate entry)
        s.region->mapped[s.index] = Own;
        chunk.push_back(s);
      }
    }
    if (chunk.empty()) {
      if (pending_.empty()) drained_cv_.notify_all();
      continue;
    }
    reclaimer_busy_ = true;
    Unmapped u;
    try {
      if (dev_.is_gpu) {
        unmap_collect(chunk, u);
      } else {
        for (auto &c : chunk) c.region->mapped[c.index] = Unbacked;
        stats().pages_unmapped += (int64_t)chunk.size();
      }
    } catch (const std::exception &e) {
      KVC_LOG(LOG_ERROR, "async unmap failed: %s", e.what());
    }
    g_pending_unmap_bytes -= std::min(chunk.size() * chunk[0].region->page_size, g_pending_unmap_bytes.load());
    lk.unlock();
    try {
      if (dev_.is_gpu) unmap_finish(u, false); // TLB invalidation + handles back to the pool: no allocator state involved
    } catch (const std::exception &e) {
      KVC_LOG(LOG_ERROR, "async unmap (finish) failed: %s", e.what());
    }
    while (foreground_waiting_.load() > 0) std::this_thread::yield(); // map calls go first
    lk.lock();
    reclaimer_busy_ = false;
    if (pending_.empty()) drained_cv_.notify_all();
  }
}

void KvAllocator::flush_unmaps() {
  std::unique_lock<std::mutex> lk(mu_);
  if (!reclaimer_.joinable()) return;
  drained_cv_.wait(lk, [&] { return pending_.empty() && !reclaimer_busy_; });
}

void KvAllocator::flush_all_unmaps() {
  std::vector<KvAllocator *> all;
  {
    std::lock_guard<std::mutex> g(g_mu);
    for (auto &kv : g_allocators) all.push_back(kv.second.get());
  }
  for (auto *a : all) a->flush_unmaps();
  if (GpuContext *ctx = gpu()) { // ... and no invalidation is left owed or in flight, no page still being zeroed
    ctx->bind();
    ctx->ensure_flushed();
    ctx->flush_limbo();
    ctx->wait_all_scrubs();
  }
}

void KvAllocator::quiesce_all(bool on) {
  static std::mutex q_mu;                                   // one holder at a time
  static std::vector<std::unique_lock<std::mutex>> held;    // (owned by the holder's thread between begin and end)
  static std::unique_lock<std::mutex> holder;
  if (on) {
    std::unique_lock<std::mutex> me(q_mu);
    std::vector<KvAllocator *> all;
    {
      std::lock_guard<std::mutex> g(g_mu);
      for (auto &kv : g_allocators) all.push_back(kv.second.get());
    }
    std::sort(all.begin(), all.end()); // a fixed order: two holders cannot exist, but map calls of several groups do
    for (auto *a : all) {
      std::unique_lock<std::mutex> lk(a->mu_, std::defer_lock);
      a->lock_foreground(lk); // (ahead of the reclaimer)
      held.push_back(std::move(lk));
    }
    holder = std::move(me);
  } else {
    if (!holder.owns_lock()) throw InvalidError("kvc_quiesce_end without kvc_quiesce_begin");
    held.clear();
    holder.unlock();
    holder = std::unique_lock<std::mutex>();
  }
}

size_t KvAllocator::pending_unmap_bytes() { return g_pending_unmap_bytes.load(); }

std::vector<KvAllocator::TensorDesc> KvAllocator::create_kv_tensors(size_t size, size_t dtype_size,
                                                                    const std::string &dev_str, int64_t num_layers,
                                                                    int64_t num_kv_buffers, bool unified_pool) {
  if (dtype_size != 1 && dtype_size != 2 && dtype_size != 4 && dtype_size != 8)
    throw std::runtime_error("Unsupported dtype size: " + std::to_string(dtype_size));
  if (num_layers <= 0 || num_kv_buffers <= 0) throw InvalidError("num_layers and num_kv_buffers must be positive");
  (void)dev_str; // the reference only asserts it equals the init device (allocator.cpp:298-301)
  std::lock_guard<std::mutex> g(mu_);
  if (num_layers_ != 0 && num_layers_ != num_layers)
    throw InvalidError("create_kv_tensors called again with a different num_layers");
  const size_t ps = g_page_size;
  size_t aligned = size;
  if (size % ps != 0) {
    aligned = ((size + ps - 1) / ps) * ps;
    KVC_LOG(LOG_WARNING, "Size %zu is not aligned to page size %zu, aligning to %zu", size, ps, aligned);
  }
  GpuContext *ctx = ctx_;
  if (ctx) ctx->bind();
  const bool backfill = dev_.is_gpu && options().zero_backfill.load();
  const size_t region_page = contiguous_ ? ps * (size_t)num_layers * (size_t)num_kv_buffers : ps;

  std::vector<TensorDesc> out;
  if (contiguous_) {
    // one region for all layers; slot = compound page (page x layers x kv buffers), allocator.cpp:139-147
    for (auto &r : layers_) destroy_region(*r);
    layers_.clear();
    auto r = make_region("kv_contiguous", aligned * (size_t)num_layers, region_page);
    if (backfill)
      backfill_all(*r);
    else
      (void)prt_all(*r, false); // lazy mode: unmapped VA unless KVCACHED_PRT=true asks for PRT
    out.push_back({r->base, r->size});
    layers_.push_back(std::move(r));
  } else {
    if (!layers_.empty() && (layers_.size() != (size_t)num_layers || layers_[0]->size != aligned))
      throw InvalidError("create_kv_tensors called again with a different size");
    if (layers_.empty()) {
      if (num_kv_buffers == 2 && !unified_pool && aligned % (2 * ps) != 0)
        throw InvalidError("Invalid tensor size: " + std::to_string(aligned) + ", must be a multiple of 2 * page size " +
                           std::to_string(2 * ps));
      for (int64_t i = 0; i < num_layers; ++i) {
        auto r = make_region("kv_" + std::to_string(i), aligned, ps);
        if (backfill)
          backfill_all(*r);
        else
          (void)prt_all(*r, false);
        layers_.push_back(std::move(r));
      }
    }
    for (auto &r : layers_) out.push_back({r->base, r->size});
  }
  const bool first_time = num_layers_ == 0;
  num_layers_ = num_layers;
  num_kv_buffers_ = num_kv_buffers;
  unified_pool_ = unified_pool;
  tensor_bytes_per_layer_ = aligned;
  if (first_time || contiguous_) setup_lanes();
  return out;
}

bool KvAllocator::kv_tensors_created() {
  std::lock_guard<std::mutex> g(mu_);
  return num_layers_ > 0;
}

bool KvAllocator::uses_prt() {
  std::lock_guard<std::mutex> g(mu_);
  return !layers_.empty() && layers_[0]->prt;
}

size_t KvAllocator::lanes_per_extent() {
  std::lock_guard<std::mutex> g(mu_);
  return lanes_ && lane_pool_ ? lane_pool_->max_extent_pages() : 0;
}

std::vector<void *> KvAllocator::region_bases() {
  std::lock_guard<std::mutex> g(mu_);
  std::vector<void *> b;
  for (auto &r : layers_) {
    b.push_back(r->base);
    if (!contiguous_ && !unified_pool_ && num_kv_buffers_ == 2) b.push_back(r->base + r->size / 2);
  }
  return b;
}

void KvAllocator::copy_blocks_host(bool to_host, const int64_t *ids, size_t n, size_t block_bytes, void *host, hipStream_t s,
                                   int codec, const int64_t *slots) {
  if (!ctx_) throw NoGpuError("copying blocks to or from host memory needs init_kvcached on a GPU device");
  std::unique_lock<std::mutex> g(mu_, std::defer_lock);
  lock_foreground(g);
  if (layers_.empty()) throw InvalidError("KV tensors are not created");
  // the regions in region_bases() order: (region, offset of the base inside it, bytes from the base to the end of its half)
  struct Span {
    KvRegion *r;
    size_t off, bytes;
  };
  std::vector<Span> spans;
  std::vector<void *> bases;
  const bool halves = !contiguous_ && !unified_pool_ && num_kv_buffers_ == 2;
  for (auto &r : layers_) {
    spans.push_back({r.get(), 0, halves ? r->size / 2 : r->size});
    if (halves) spans.push_back({r.get(), r->size / 2, r->size / 2});
  }
  for (auto &sp : spans) bases.push_back(sp.r->base + sp.off);
  // Every slot that a (block, region) byte range touches must be backed by a page - a block may straddle two slots. An
  // unbacked slot is unmapped VA in the lazy mode (a GPU fault) and a PRT entry in the default one, which the TLBs would
  // cache. The page-table entries of a backed slot stay valid whatever is mapped or unmapped around it
  // (DESIGN.md §4.14), so the launch needs no fence beyond this lock.
  for (auto &sp : spans) {
    const size_t ps = sp.r->page_size;
    for (size_t i = 0; i < n; ++i) {
      if (ids[i] < 0 || (size_t)ids[i] >= sp.bytes / block_bytes)
        throw InvalidError("block id " + std::to_string(ids[i]) + " is outside the KV tensors");
      const size_t first = sp.off + (size_t)ids[i] * block_bytes, last = first + block_bytes - 1;
      for (size_t slot = first / ps; slot <= last / ps; ++slot) {
        const uint8_t st = sp.r->mapped[slot];
        if (st != Own && st != Imported && st != Lane && st != PeerLane)
          throw InvalidError("block id " + std::to_string(ids[i]) + " lies on a slot of " + sp.r->name + " that is not backed");
      }
    }
  }
  ctx_->bind();
  ctx_->copy_blocks_host(to_host, bases.data(), bases.size(), ids, n, block_bytes, host, s, codec, slots);
}

// Offsets -> (region, slot) in the reference's order: layer-major, then offset, K before V
// (allocator.cpp:168-207). Contiguous: one compound slot per offset. Unified pool: one slot per layer.
std::vector<KvAllocator::Slot> KvAllocator::slots_for(const offset_t *offsets, size_t n) {
  std::vector<Slot> s;
  auto add = [&](KvRegion *r, offset_t off) {
    if (off < 0 || (size_t)off % r->page_size != 0 || (size_t)off >= r->size)
      throw InvalidError("offset " + std::to_string(off) + " is not a valid page offset of " + r->name);
    s.push_back({r, (size_t)off / r->page_size});
  };
  if (contiguous_) {
    for (size_t i = 0; i < n; ++i) add(layers_[0].get(), offsets[i]);
  } else if (unified_pool_ || num_kv_buffers_ == 1) {
    // One slot per layer per offset. NB for a single KV buffer (MLA) the reference's per-layer branch
    // still maps `offset + size/2` as well (allocator.cpp:189-206), i.e. two pages where its own
    // accounting (page_allocator.cpp:688-695) counts one, and out of range for the upper half of the
    // page ids; we back exactly what is accounted (DESIGN.md "reference quirks").
    s.reserve(layers_.size() * n);
    for (auto &r : layers_)
      for (size_t i = 0; i < n; ++i) add(r.get(), offsets[i]);
  } else {
    s.reserve(layers_.size() * n * 2);
    for (auto &r : layers_) {
      const offset_t v_base = (offset_t)(r->size / 2); // get_v_base_offset, allocator.cpp:46-52
      for (size_t i = 0; i < n; ++i) {
        add(r.get(), offsets[i]);
        add(r.get(), offsets[i] + v_base);
      }
    }
  }
  return s;
}

bool KvAllocator::map_to_kv_tensors(const offset_t *offsets, size_t n) {
  const int64_t t0 = now_ns();
  GpuContext::Foreground fg(ctx_);
  std::unique_lock<std::mutex> g(mu_, std::defer_lock);
  lock_foreground(g);
  if (num_layers_ == 0) {
    KVC_LOG(LOG_ERROR, "try to map to KV tensors when KV tensors are not created");
    return false;
  }
  SegTimer sg;
  if (lanes_ && try_map_lanes(offsets, n)) { // page ids of a multi-row geometry: backed as units (lanes)
    stats().map_calls++;
    stats().map_ns += now_ns() - t0;
    return true;
  }
  const auto slots = slots_for(offsets, n);
  sg.mark(kSegMapOffsets);
  map_slots(slots, nullptr);
  stats().map_calls++;
  stats().map_ns += now_ns() - t0;
  return true;
}

bool KvAllocator::unmap_from_kv_tensors(const offset_t *offsets, size_t n) {
  const int64_t t0 = now_ns();
  GpuContext::Foreground fg(ctx_);
  std::unique_lock<std::mutex> g(mu_, std::defer_lock);
  lock_foreground(g);
  if (num_layers_ == 0) {
    KVC_LOG(LOG_ERROR, "try to unmap from KV tensors when KV tensors are not created");
    return false;
  }
  SegTimer sg;
  std::vector<offset_t> others;
  if (lanes_) { // page ids backed by lanes go back as units; whatever else the call names takes the generic path
    (void)unmap_lanes(offsets, n, &others);
    if (others.empty()) {
      stats().unmap_calls++;
      stats().unmap_ns += now_ns() - t0;
      return true;
    }
    offsets = others.data();
    n = others.size();
    sg.t = now_ns();
  }
  auto slots = slots_for(offsets, n);
  sg.mark(kSegUnmapOffsets);
  bool async = options().async_unmap.load() != 0; // also on the cpu device: same queue and thread, no driver calls
  for (auto &r : layers_) async = async && !r->backfilled; // compat mode promises zeros behind an unmap: stay synchronous
  if (async) {
    std::vector<Slot> now; // imported pages are a peer's memory: dropped at once
    size_t queued = 0;
    for (auto &s : slots) {
      uint8_t &m = s.region->mapped[s.index];
      if (m == Own) {
        m = UnmapQueued;
        pending_.push_back(s);
        ++queued;
      } else if (m == Imported) {
        now.push_back(s);
      } else { // reference: log + skip (ftensor.cpp:124-127)
        KVC_LOG(LOG_ERROR, "Page %zu is not mapped.", s.index);
      }
    }
    if (queued) {
      g_pending_unmap_bytes += queued * slots[0].region->page_size;
      stats().unmaps_queued += (int64_t)queued;
      if (!reclaimer_.joinable()) reclaimer_ = std::thread(&KvAllocator::reclaimer_loop, this);
      pending_cv_.notify_one();
    }
    if (!now.empty()) unmap_slots(now);
  } else {
    unmap_slots(slots);
  }
  stats().unmap_calls++;
  stats().unmap_ns += now_ns() - t0;
  return true;
}

} // namespace kvc
