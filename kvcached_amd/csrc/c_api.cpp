// c_api.cpp — the extern "C" surface declared in include/kvcached_amd.h.
#include "../../include/kvcached_amd.h"

#include <algorithm>
#include <cstring>
#include <vector>

#include "kernels.hpp"
#include "kv_allocator.hpp"
#include "page_allocator.hpp"

using namespace kvc;

namespace {
thread_local std::string g_last_error;

int fail(int code, const char *what) {
  g_last_error = what ? what : "";
  return code;
}

// Maps the exception zoo onto KVC_E_* and records the message.
template <class F> auto guarded(F &&f) -> decltype(f()) {
  using R = decltype(f());
  try {
    return f();
  } catch (const NoPagesError &e) {
    return (R)fail(KVC_E_NO_PAGES, e.what());
  } catch (const GpuError &e) {
    return (R)fail(KVC_E_GPU, e.what());
  } catch (const NoGpuError &e) {
    return (R)fail(KVC_E_NO_GPU, e.what());
  } catch (const InvalidError &e) {
    return (R)fail(KVC_E_INVALID, e.what());
  } catch (const CallbackError &e) {
    return (R)fail(KVC_E_CALLBACK, e.what());
  } catch (const std::exception &e) {
    return (R)fail(KVC_E_RUNTIME, e.what());
  } catch (...) {
    return (R)fail(KVC_E_RUNTIME, "unknown error");
  }
}

template <class C> int64_t copy_out(const C &v, int64_t *out, int64_t cap) {
  const int64_t n = (int64_t)v.size();
  if (out && cap >= n) std::copy(v.begin(), v.end(), out);
  return n;
}

inline InternalPage *P(kvc_page_t *p) { return reinterpret_cast<InternalPage *>(p); }
inline const InternalPage *P(const kvc_page_t *p) { return reinterpret_cast<const InternalPage *>(p); }
inline PageAllocator *A(kvc_page_allocator_t *p) { return reinterpret_cast<PageAllocator *>(p); }
inline const PageAllocator *A(const kvc_page_allocator_t *p) { return reinterpret_cast<const PageAllocator *>(p); }
} // namespace

extern "C" {

const char *kvc_last_error(void) { return g_last_error.c_str(); }
int kvc_abi_version(void) { return KVC_ABI_VERSION; }

// ---------------------------------------------------------------- allocator lifecycle
int kvc_init(const char *dev_str, size_t page_size, int contiguous_layout) {
  return guarded([&]() -> int {
    if (!dev_str) throw InvalidError("dev_str is NULL");
    KvAllocator::init(dev_str, page_size, contiguous_layout != 0);
    return KVC_OK;
  });
}
int kvc_shutdown(void) {
  return guarded([&]() -> int {
    KvAllocator::shutdown();
    return KVC_OK;
  });
}
int kvc_create_kv_tensors(size_t size, size_t dtype_size, const char *dev_str, int64_t num_layers,
                          int64_t num_kv_buffers, int64_t group_id, int unified_pool, void **out_ptrs,
                          size_t *out_nbytes, int64_t *inout_count) {
  return guarded([&]() -> int {
    if (!out_ptrs || !out_nbytes || !inout_count) throw InvalidError("output arrays are NULL");
    auto descs = KvAllocator::global(group_id)->create_kv_tensors(size, dtype_size, dev_str ? dev_str : "", num_layers,
                                                                  num_kv_buffers, unified_pool != 0);
    if ((int64_t)descs.size() > *inout_count) throw InvalidError("output arrays too small for the tensor list");
    for (size_t i = 0; i < descs.size(); ++i) {
      out_ptrs[i] = descs[i].ptr;
      out_nbytes[i] = descs[i].nbytes;
    }
    *inout_count = (int64_t)descs.size();
    return KVC_OK;
  });
}
int kvc_kv_tensors_created(int64_t group_id) {
  return guarded([&]() -> int { return KvAllocator::global(group_id)->kv_tensors_created() ? 1 : 0; });
}
int kvc_get_device(int *is_gpu, int *index) {
  if (!KvAllocator::initialized()) return fail(KVC_E_INVALID, "init_kvcached has not been called");
  DeviceSpec d = KvAllocator::device();
  if (is_gpu) *is_gpu = d.is_gpu ? 1 : 0;
  if (index) *index = d.index;
  return KVC_OK;
}
int kvc_map_to_kv_tensors(const int64_t *offsets, size_t n, int64_t group_id) {
  return guarded([&]() -> int {
    return KvAllocator::global(group_id)->map_to_kv_tensors(offsets, n) ? KVC_OK
                                                                         : fail(KVC_E_NOT_CREATED, "KV tensors are not created");
  });
}
int kvc_unmap_from_kv_tensors(const int64_t *offsets, size_t n, int64_t group_id) {
  return guarded([&]() -> int {
    return KvAllocator::global(group_id)->unmap_from_kv_tensors(offsets, n)
               ? KVC_OK
               : fail(KVC_E_NOT_CREATED, "KV tensors are not created");
  });
}

// The stored options are rows of the table in options.cpp; the names of all numbers: include/kvcached_amd.h.
int kvc_set_option(int opt, int64_t value) {
  if (opt == KVC_OPT_ASYNC_UNMAP && !value) KvAllocator::flush_all_unmaps(); // switching off: nothing may stay queued
  if (opt == KVC_OPT_UNMAP_INVALIDATION_US && value <= 0) // ... nor parked behind an invalidation nobody is in a hurry for
    if (GpuContext *ctx = KvAllocator::gpu()) ctx->flush_limbo();
  if (opt == KVC_OPT_FAIL_AFTER_CREATES) fail_after_creates() = value;
  else if (!set_stored_option(opt, value)) return fail(KVC_E_INVALID, "unknown option");
  return KVC_OK;
}
int64_t kvc_get_option(int opt) {
  int64_t stored;
  if (get_stored_option(opt, &stored)) return stored;
  if (opt >= KVC_OPT_HOST_SEGMENT_0 && opt < KVC_OPT_SEG_END) return stats().seg[opt - KVC_OPT_HOST_SEGMENT_0];
  GpuContext *ctx = nullptr; // (computed diagnostics, all read-only)
  switch (opt) {
  case KVC_OPT_FAIL_AFTER_CREATES: return fail_after_creates();
  case KVC_OPT_EFFECTIVE_BACKEND: return vmm_backend().load();
  case KVC_OPT_BACKGROUND_SHOOTDOWNS: return background_shootdowns().load();
  case KVC_OPT_KFD_CREATE_ACTIVE: return vmm_backend().load() == kVmmDrm && DrmVm::instance().kfd_ready() ? 1 : 0;
  case KVC_OPT_KFD_ALLOC_NS: return DrmVm::instance().create_times().alloc_ns.load();
  case KVC_OPT_KFD_EXPORT_NS: return DrmVm::instance().create_times().export_ns.load();
  case KVC_OPT_DRM_IMPORT_NS: return DrmVm::instance().create_times().import_ns.load();
  case KVC_OPT_KFD_CREATES: return DrmVm::instance().create_times().count.load();
  case KVC_OPT_KFD_FREE_NS: return DrmVm::instance().create_times().free_ns.load();
  case KVC_OPT_KFD_FREES: return DrmVm::instance().create_times().frees.load();
  case KVC_OPT_KFD_TLB_FLUSH_ACTIVE: return (ctx = KvAllocator::gpu()) && ctx->kfd_flush_active() ? 1 : 0;
  case KVC_OPT_POOL_HELD_PAGES: case KVC_OPT_POOL_OUT_PAGES: case KVC_OPT_POOL_FREE_PIECES: case KVC_OPT_POOL_EXTENT_PAGES_NOW: {
    if (!(ctx = KvAllocator::gpu())) return 0;
    ExtentPool *p = ctx->primary_pool();
    // (nothing mapped yet: no pool is made for a diagnostic)
    if (!p) return opt == KVC_OPT_POOL_EXTENT_PAGES_NOW ? (int64_t)options().phys_chunk_pages.load() : 0;
    const auto f = p->footprint();
    const int64_t scale = (int64_t)p->counter_scale();
    return scale * (int64_t)(opt == KVC_OPT_POOL_HELD_PAGES    ? f.held_pages
                             : opt == KVC_OPT_POOL_OUT_PAGES   ? f.out_pages
                             : opt == KVC_OPT_POOL_FREE_PIECES ? f.free_pieces
                                                               : f.extent_pages_now);
  }
  case KVC_OPT_POOL_BAD_RELEASES: {
    ExtentPool *p = (ctx = KvAllocator::gpu()) ? ctx->primary_pool() : nullptr;
    return p ? (int64_t)p->footprint().bad_releases : 0;
  }
  case KVC_OPT_PAGES_SCRUBBED: return stats().pages_scrubbed;
  case KVC_OPT_PAGES_PRESCRUBBED: return stats().pages_prescrubbed;
  case KVC_OPT_ZERO_EXTENT_PAGES: return (ctx = KvAllocator::gpu()) ? (int64_t)ctx->zero_extent_pages(KvAllocator::page_size()) : 0;
  case KVC_OPT_PRT:
  case KVC_OPT_LANES_PER_BUFFER:
    try {
      if (!KvAllocator::initialized()) return 0;
      KvAllocator *a = KvAllocator::global(0);
      return opt == KVC_OPT_PRT ? (a->uses_prt() ? 1 : 0) : (int64_t)a->lanes_per_extent();
    } catch (...) {
      return 0;
    }
  case KVC_OPT_IMPORTS_DIRECT: return import_count(true);
  case KVC_OPT_IMPORTS_RUNTIME: return import_count(false);
  default: return fail(KVC_E_INVALID, "unknown option");
  }
}

int kvc_get_stats(kvc_stats_t *o) {
  if (!o) return fail(KVC_E_INVALID, "NULL stats");
  Stats &s = stats();
  o->pages_mapped = s.pages_mapped;
  o->pages_unmapped = s.pages_unmapped;
  o->handles_created = s.vmm.created;
  o->handles_released = s.vmm.released;
  o->handles_reused = s.vmm.reused;
  o->map_calls = s.map_calls;
  o->unmap_calls = s.unmap_calls;
  o->map_ns = s.map_ns;
  o->unmap_ns = s.unmap_ns;
  o->fill_launches = s.fill_launches;
  o->fill_bytes = s.fill_bytes;
  o->compact_launches = s.compact_launches;
  o->compact_bytes = s.compact_bytes;
  o->tlb_shootdowns = s.tlb_shootdowns;
  o->shootdown_ns = s.shootdown_ns;
  o->index_launches = s.index_launches;
  o->unmaps_queued = s.unmaps_queued;
  o->unmaps_cancelled = s.unmaps_cancelled;
  std::lock_guard<std::mutex> g(s.mu);
  o->fill_ms = s.fill_ms;
  o->compact_ms = s.compact_ms;
  return KVC_OK;
}
int kvc_quiesce_begin(void) {
  return guarded([&]() -> int {
    KvAllocator::quiesce_all(true);
    return KVC_OK;
  });
}
int kvc_quiesce_end(void) {
  return guarded([&]() -> int {
    KvAllocator::quiesce_all(false);
    return KVC_OK;
  });
}
int kvc_flush_unmaps(void) {
  return guarded([&]() -> int {
    KvAllocator::flush_all_unmaps();
    return KVC_OK;
  });
}
int kvc_get_driver_breakdown(int64_t *o) {
  if (!o) return fail(KVC_E_INVALID, "NULL output");
  Stats &s = stats();
  o[0] = s.t_unmap_alias; o[1] = s.t_acquire; o[2] = s.t_map; o[3] = s.t_access;
  o[4] = s.t_unmap; o[5] = s.t_release; o[6] = s.t_realias; o[7] = s.t_sync;
  return KVC_OK;
}
int kvc_reset_stats(void) {
  stats().reset();
  return KVC_OK;
}

int kvc_mem_get_info(size_t *free_bytes, size_t *total_bytes) {
  return guarded([&]() -> int {
    mem_get_info(free_bytes, total_bytes);
    return KVC_OK;
  });
}
int kvc_set_mem_info_override(size_t free_bytes, size_t total_bytes) {
  set_mem_info_override(free_bytes, total_bytes);
  return KVC_OK;
}

// ---------------------------------------------------------------- InternalPage
kvc_page_t *kvc_page_new(int64_t page_id, int64_t page_size) {
  return reinterpret_cast<kvc_page_t *>(new InternalPage(page_id, page_size));
}
void kvc_page_delete(kvc_page_t *p) { delete P(p); }
int64_t kvc_page_id(const kvc_page_t *p) { return P(p)->page_id; }
int64_t kvc_page_size(const kvc_page_t *p) { return P(p)->page_size; }
void kvc_page_init(kvc_page_t *p, int64_t block_mem_size) { P(p)->init(block_mem_size); }
int64_t kvc_page_alloc(kvc_page_t *p, int64_t num_blocks, int64_t *out) {
  return guarded([&]() -> int64_t {
    auto v = P(p)->alloc(num_blocks);
    return copy_out(v, out, num_blocks);
  });
}
void kvc_page_free(kvc_page_t *p, int64_t block_id) { P(p)->free(block_id); }
void kvc_page_free_batch(kvc_page_t *p, const int64_t *ids, size_t n) { P(p)->free_batch(ids, n); }
int kvc_page_empty(const kvc_page_t *p) { return P(p)->empty(); }
int kvc_page_full(const kvc_page_t *p) { return P(p)->full(); }
int64_t kvc_page_num_free_blocks(const kvc_page_t *p) { return P(p)->num_free_blocks(); }
int64_t kvc_page_get_free_blocks(const kvc_page_t *p, int64_t *out, int64_t cap) {
  return copy_out(P(p)->free_blocks(), out, cap);
}
void kvc_page_get_block_range(int64_t page_id, int64_t page_size, int64_t block_mem_size, int64_t *start, int64_t *end) {
  auto r = InternalPage::get_block_range(page_id, page_size, block_mem_size);
  *start = r.first;
  *end = r.second;
}
int64_t kvc_page_get_num_blocks(int64_t page_size, int64_t block_mem_size) {
  return InternalPage::get_num_blocks(page_size, block_mem_size);
}

// ---------------------------------------------------------------- PageAllocator
kvc_page_allocator_t *kvc_pa_new(int64_t num_layers, int64_t mem_size_per_layer, int64_t page_size, int64_t world_size,
                                 int64_t pp_rank, int async_sched, int contiguous_layout, int enable_page_prealloc,
                                 int64_t num_kv_buffers, int64_t group_id, const char *ipc_name) {
  try {
    return reinterpret_cast<kvc_page_allocator_t *>(
        new PageAllocator(num_layers, mem_size_per_layer, page_size, world_size, pp_rank, async_sched != 0,
                          contiguous_layout != 0, enable_page_prealloc != 0, num_kv_buffers, group_id,
                          ipc_name ? ipc_name : ""));
  } catch (const std::exception &e) {
    g_last_error = e.what();
    return nullptr;
  }
}
void kvc_pa_delete(kvc_page_allocator_t *pa) { delete A(pa); }
int kvc_pa_start_prealloc_thread(kvc_page_allocator_t *pa) {
  return guarded([&]() -> int {
    A(pa)->start_prealloc_thread();
    return KVC_OK;
  });
}
int kvc_pa_stop_prealloc_thread(kvc_page_allocator_t *pa) {
  return guarded([&]() -> int {
    A(pa)->stop_prealloc_thread();
    return KVC_OK;
  });
}
int64_t kvc_pa_alloc_page(kvc_page_allocator_t *pa) {
  return guarded([&]() -> int64_t { return A(pa)->alloc_page(); });
}
int64_t kvc_pa_alloc_pages(kvc_page_allocator_t *pa, int64_t n, int64_t *out_ids) {
  return guarded([&]() -> int64_t {
    if (n > 0 && !out_ids) throw InvalidError("out_ids is NULL");
    auto ids = A(pa)->alloc_pages(n);
    std::copy(ids.begin(), ids.end(), out_ids);
    return (int64_t)ids.size();
  });
}
int kvc_pa_free_page(kvc_page_allocator_t *pa, int64_t page_id) {
  return guarded([&]() -> int {
    A(pa)->free_page(page_id);
    return KVC_OK;
  });
}
int kvc_pa_free_pages(kvc_page_allocator_t *pa, const int64_t *page_ids, size_t n) {
  return guarded([&]() -> int {
    A(pa)->free_pages(page_ids, n);
    return KVC_OK;
  });
}
int kvc_pa_resize(kvc_page_allocator_t *pa, int64_t new_mem_size) {
  return guarded([&]() -> int { return A(pa)->resize(new_mem_size) ? 1 : 0; });
}
int kvc_pa_trim(kvc_page_allocator_t *pa) {
  return guarded([&]() -> int {
    A(pa)->trim();
    return KVC_OK;
  });
}
int kvc_pa_reset_free_page_order(kvc_page_allocator_t *pa) {
  return guarded([&]() -> int {
    A(pa)->reset_free_page_order();
    return KVC_OK;
  });
}
int64_t kvc_pa_get_num_free_pages(const kvc_page_allocator_t *pa) { return A(pa)->get_num_free_pages(); }
int64_t kvc_pa_get_num_inuse_pages(const kvc_page_allocator_t *pa) { return A(pa)->get_num_inuse_pages(); }
int64_t kvc_pa_get_num_total_pages(const kvc_page_allocator_t *pa) { return A(pa)->get_num_total_pages(); }
int64_t kvc_pa_get_num_reserved_pages(const kvc_page_allocator_t *pa) { return A(pa)->get_num_reserved_pages(); }
int64_t kvc_pa_get_avail_physical_pages(const kvc_page_allocator_t *pa) {
  return guarded([&]() -> int64_t { return A(pa)->get_avail_physical_pages(); });
}
int64_t kvc_pa_check_and_get_resize_target(const kvc_page_allocator_t *pa, int64_t current_mem_size) {
  return A(pa)->check_and_get_resize_target(current_mem_size);
}
int64_t kvc_pa_get_resize_target(const kvc_page_allocator_t *pa) { return A(pa)->get_resize_target(); }
int64_t kvc_pa_get_page_id(const kvc_page_allocator_t *pa, int64_t block_id, int64_t block_mem_size) {
  return A(pa)->get_page_id(block_id, block_mem_size);
}
int64_t kvc_pa_group_indices_by_page(const kvc_page_allocator_t *pa, const int64_t *indices, size_t n,
                                     int64_t block_mem_size, int64_t *keys, int64_t *counts, int64_t *values) {
  return guarded([&]() -> int64_t {
    auto groups = A(pa)->group_indices_by_page(indices, n, block_mem_size);
    int64_t k = 0, w = 0;
    for (auto &kv : groups) { // iteration order is the contract
      keys[k] = kv.first;
      counts[k] = (int64_t)kv.second.size();
      std::memcpy(values + w, kv.second.data(), kv.second.size() * sizeof(int64_t));
      w += (int64_t)kv.second.size();
      ++k;
    }
    return k;
  });
}
int kvc_pa_set_broadcast_map_callback(kvc_page_allocator_t *pa, kvc_broadcast_cb cb, void *user) {
  A(pa)->set_broadcast_map_callback(
      cb ? BroadcastFn([cb, user](int64_t ws, const offset_t *o, size_t n) { return cb(user, ws, o, n); }) : BroadcastFn());
  return KVC_OK;
}
int kvc_pa_set_broadcast_unmap_callback(kvc_page_allocator_t *pa, kvc_broadcast_cb cb, void *user) {
  A(pa)->set_broadcast_unmap_callback(
      cb ? BroadcastFn([cb, user](int64_t ws, const offset_t *o, size_t n) { return cb(user, ws, o, n); }) : BroadcastFn());
  return KVC_OK;
}
int kvc_pa_set_should_use_worker_ipc_callback(kvc_page_allocator_t *pa, kvc_bool_cb cb, void *user) {
  A(pa)->set_should_use_worker_ipc_callback(cb ? BoolFn([cb, user]() { return cb(user) != 0; }) : BoolFn());
  return KVC_OK;
}
int64_t kvc_pa_get_page_list(const kvc_page_allocator_t *pa, int which, int64_t *out, int64_t cap) {
  return copy_out(A(pa)->page_list(which), out, cap);
}
const char *kvc_pa_ipc_name(const kvc_page_allocator_t *pa) { return A(pa)->ipc_name().c_str(); }

// ---------------------------------------------------------------- kernels
int kvc_zero_fill_pages(void *const *page_ptrs, size_t n, size_t page_bytes, void *stream, int sync) {
  return guarded([&]() -> int {
    GpuContext *ctx = KvAllocator::gpu();
    if (!ctx) throw NoGpuError("zero_fill_pages needs init_kvcached on a GPU device");
    if (n && !page_ptrs) throw InvalidError("page_ptrs is NULL");
    if (page_bytes == 0 || page_bytes % kFillSlabBytes != 0) throw InvalidError("page_bytes must be a multiple of 64 KiB");
    for (size_t i = 0; i < n; ++i)
      if (reinterpret_cast<uintptr_t>(page_ptrs[i]) % 16 != 0) throw InvalidError("page pointer is not 16-byte aligned");
    ctx->bind();
    ctx->zero_fill(page_ptrs, n, page_bytes, static_cast<hipStream_t>(stream));
    if (sync) ctx->sync(static_cast<hipStream_t>(stream));
    return KVC_OK;
  });
}

int kvc_compact_blocks(void *const *region_bases, size_t n_regions, const int64_t *src_blocks, const int64_t *dst_blocks,
                       size_t n_moves, size_t block_bytes, void *stream, int sync) {
  return guarded([&]() -> int {
    GpuContext *ctx = KvAllocator::gpu();
    if (!ctx) throw NoGpuError("compact_blocks needs init_kvcached on a GPU device");
    if ((n_regions && !region_bases) || (n_moves && (!src_blocks || !dst_blocks))) throw InvalidError("NULL argument");
    if (block_bytes == 0 || block_bytes % 16 != 0) throw InvalidError("block_bytes must be a positive multiple of 16");
    for (size_t i = 0; i < n_moves; ++i)
      if (src_blocks[i] < 0 || dst_blocks[i] < 0) throw InvalidError("negative block id");
    ctx->bind();
    ctx->compact(region_bases, n_regions, src_blocks, dst_blocks, n_moves, block_bytes, static_cast<hipStream_t>(stream));
    if (sync) ctx->sync(static_cast<hipStream_t>(stream));
    return KVC_OK;
  });
}

namespace {
// Host side of kvc_copy_blocks_{to,from}_host and, with a codec, of kvc_encode_blocks_to_host / kvc_decode_blocks_from_host:
// arguments, the host buffer (pinned, 16-byte aligned, resolved to the address the GPU reaches it at), then the allocator's
// own checks and the launch. With `slots` (kvc_copy_blocks_{to,from}_host_slots), block i's row of the image is row slots[i] of
// an arena of n_slots rows.
int copy_blocks_host(bool to_host, int64_t group_id, const int64_t *block_ids, size_t n, size_t block_bytes, const void *host,
                     void *stream, int sync, int codec = kCodecRaw, const int64_t *slots = nullptr, size_t n_slots = 0,
                     bool with_slots = false) {
  return guarded([&]() -> int {
    GpuContext *ctx = KvAllocator::gpu();
    if (!ctx) throw NoGpuError("copying blocks to or from host memory needs init_kvcached on a GPU device");
    if (n && (!block_ids || !host || (with_slots && !slots))) throw InvalidError("NULL argument");
    if (block_bytes == 0 || block_bytes % 16 != 0) throw InvalidError("block_bytes must be a positive multiple of 16");
    if (codec != kCodecRaw && codec != KVC_CODEC_MXFP8_BF16 && codec != KVC_CODEC_MXFP8_F16) throw InvalidError("unknown codec");
    if (host_record_bytes(codec, block_bytes) == 0) throw InvalidError("block_bytes must be a multiple of 1024 for this codec");
    for (size_t i = 0; i < n; ++i)
      if (block_ids[i] < 0) throw InvalidError("negative block id");
    if (!to_host && n > 1) { // two copies into one block would race
      std::vector<int64_t> sorted(block_ids, block_ids + n);
      std::sort(sorted.begin(), sorted.end());
      if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) throw InvalidError("duplicate block id");
    }
    if (with_slots) {
      if (n_slots > 0x100000000ull) throw InvalidError("an arena holds at most 2^32 slots");
      for (size_t i = 0; i < n; ++i)
        if (slots[i] < 0 || (uint64_t)slots[i] >= n_slots)
          throw InvalidError("slot " + std::to_string(slots[i]) + " is outside the arena of " + std::to_string(n_slots) + " slots");
      if (to_host && n > 1) { // two copies into one slot would race
        std::vector<int64_t> sorted(slots, slots + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) throw InvalidError("duplicate slot");
      }
    }
    if (n == 0) return KVC_OK;
    if (reinterpret_cast<uintptr_t>(host) % 16 != 0) throw InvalidError("host buffer is not 16-byte aligned");
    ctx->bind();
    hipPointerAttribute_t attr;
    std::memset(&attr, 0, sizeof(attr));
    if (hipPointerGetAttributes(&attr, host) != hipSuccess || attr.type != hipMemoryTypeHost || !attr.devicePointer) {
      (void)hipGetLastError();
      throw InvalidError("host buffer is not pinned host memory");
    }
    char *dev = static_cast<char *>(attr.devicePointer);
    if (attr.hostPointer) dev += static_cast<const char *>(host) - static_cast<const char *>(attr.hostPointer);
    if (reinterpret_cast<uintptr_t>(dev) % 16 != 0) throw InvalidError("host buffer is not 16-byte aligned on the device side");
    KvAllocator::global(group_id)->copy_blocks_host(to_host, block_ids, n, block_bytes, dev, static_cast<hipStream_t>(stream),
                                                    codec, with_slots ? slots : nullptr);
    if (sync) ctx->sync(static_cast<hipStream_t>(stream));
    return KVC_OK;
  });
}
} // namespace

int kvc_copy_blocks_to_host(int64_t group_id, const int64_t *block_ids, size_t n, size_t block_bytes, void *host, void *stream,
                            int sync) {
  return copy_blocks_host(true, group_id, block_ids, n, block_bytes, host, stream, sync);
}

int kvc_copy_blocks_from_host(int64_t group_id, const int64_t *block_ids, size_t n, size_t block_bytes, const void *host,
                              void *stream, int sync) {
  return copy_blocks_host(false, group_id, block_ids, n, block_bytes, host, stream, sync);
}

static_assert(KVC_CODEC_MXFP8_BF16 == kCodecMxfp8Bf16 && KVC_CODEC_MXFP8_F16 == kCodecMxfp8F16, "the header's numbers are the kernels'");

size_t kvc_codec_record_bytes(int codec, size_t block_bytes) {
  return codec == kCodecRaw ? 0 : host_record_bytes(codec, block_bytes);
}

// (a codec number of 0 is not an encoding: these two refuse it instead of copying bytes)
int kvc_encode_blocks_to_host(int64_t group_id, const int64_t *block_ids, size_t n, size_t block_bytes, int codec, void *host,
                              void *stream, int sync) {
  return copy_blocks_host(true, group_id, block_ids, n, block_bytes, host, stream, sync, codec == kCodecRaw ? -1 : codec);
}

int kvc_decode_blocks_from_host(int64_t group_id, const int64_t *block_ids, size_t n, size_t block_bytes, int codec,
                                const void *host, void *stream, int sync) {
  return copy_blocks_host(false, group_id, block_ids, n, block_bytes, host, stream, sync, codec == kCodecRaw ? -1 : codec);
}

// (here codec 0 is the raw copy: one pair of entries for the three images)
int kvc_copy_blocks_to_host_slots(int64_t group_id, const int64_t *block_ids, const int64_t *slots, size_t n, size_t block_bytes,
                                  int codec, void *host, size_t n_slots, void *stream, int sync) {
  return copy_blocks_host(true, group_id, block_ids, n, block_bytes, host, stream, sync, codec, slots, n_slots, true);
}

int kvc_copy_blocks_from_host_slots(int64_t group_id, const int64_t *block_ids, const int64_t *slots, size_t n,
                                    size_t block_bytes, int codec, const void *host, size_t n_slots, void *stream, int sync) {
  return copy_blocks_host(false, group_id, block_ids, n, block_bytes, host, stream, sync, codec, slots, n_slots, true);
}

int64_t kvc_get_region_bases(int64_t group_id, void **out, int64_t cap) {
  return guarded([&]() -> int64_t {
    auto b = KvAllocator::global(group_id)->region_bases();
    if (out && cap >= (int64_t)b.size()) std::copy(b.begin(), b.end(), out);
    return (int64_t)b.size();
  });
}

// ---------------------------------------------------------------- block ids <-> token indices
namespace {
GpuContext *index_ctx(const char *what) {
  GpuContext *ctx = KvAllocator::gpu();
  if (!ctx) throw NoGpuError(std::string(what) + " needs init_kvcached on a GPU device");
  ctx->bind();
  return ctx;
}
} // namespace

int kvc_expand_block_ids(const int64_t *block_ids, size_t n, int64_t tpb, int64_t *out_dev, void *stream) {
  return guarded([&]() -> int {
    GpuContext *ctx = index_ctx("expand_block_ids");
    if (tpb <= 0 || tpb > 0x7fffffff) throw InvalidError("tokens_per_block must be in [1, 2^31)");
    if (n && (!block_ids || !out_dev)) throw InvalidError("NULL argument");
    ctx->expand_block_ids(block_ids, n, tpb, out_dev, static_cast<hipStream_t>(stream));
    return KVC_OK;
  });
}

int kvc_alloc_extend_indices(const int64_t *prefix_lens_dev, const int64_t *seq_lens_dev, const int64_t *last_loc_dev,
                             size_t bs, const int64_t *new_block_ids, size_t n_new, int64_t tpb, int64_t *out_dev,
                             size_t extend_num_tokens, void *stream) {
  return guarded([&]() -> int {
    GpuContext *ctx = index_ctx("alloc_extend_indices");
    if (tpb <= 0 || tpb > 0x7fffffff) throw InvalidError("tokens_per_block must be in [1, 2^31)");
    if (bs && (!prefix_lens_dev || !seq_lens_dev || !last_loc_dev)) throw InvalidError("NULL argument");
    if ((n_new && !new_block_ids) || (extend_num_tokens && !out_dev)) throw InvalidError("NULL argument");
    if (extend_num_tokens > (size_t)65535 * 4096) throw InvalidError("extend_num_tokens too large for one call");
    ctx->alloc_extend_indices(prefix_lens_dev, seq_lens_dev, last_loc_dev, bs, new_block_ids, n_new, tpb, out_dev,
                              extend_num_tokens, static_cast<hipStream_t>(stream));
    return KVC_OK;
  });
}

int kvc_alloc_decode_indices(const int64_t *seq_lens_dev, const int64_t *last_loc_dev, size_t bs,
                             const int64_t *new_block_ids, size_t n_new, int64_t tpb, int64_t *out_dev, void *stream) {
  return guarded([&]() -> int {
    GpuContext *ctx = index_ctx("alloc_decode_indices");
    if (tpb <= 0 || tpb > 0x7fffffff) throw InvalidError("tokens_per_block must be in [1, 2^31)");
    if (bs && (!seq_lens_dev || !last_loc_dev || !out_dev)) throw InvalidError("NULL argument");
    if (n_new && !new_block_ids) throw InvalidError("NULL argument");
    ctx->alloc_decode_indices(seq_lens_dev, last_loc_dev, bs, new_block_ids, n_new, tpb, out_dev,
                              static_cast<hipStream_t>(stream));
    return KVC_OK;
  });
}

int64_t kvc_unique_block_ids(const int64_t *token_indices_dev, size_t n, int64_t tpb, int64_t num_blocks, int64_t *out_host,
                             size_t cap, void *stream) {
  return guarded([&]() -> int64_t {
    GpuContext *ctx = index_ctx("unique_block_ids");
    if (n && !token_indices_dev) throw InvalidError("NULL argument");
    return ctx->unique_block_ids(token_indices_dev, n, tpb, num_blocks, out_host, cap, static_cast<hipStream_t>(stream));
  });
}

// ---------------------------------------------------------------- TP shared pool
int kvc_export_mapped_slots(const int64_t *offsets, size_t n, int64_t group_id, int *out_fds, int64_t cap) {
  return guarded([&]() -> int { return KvAllocator::global(group_id)->export_mapped_slots(offsets, n, out_fds, cap); });
}
int kvc_map_imported_slots(const int64_t *offsets, size_t n, int64_t group_id, const int *fds, size_t n_fds) {
  return guarded([&]() -> int {
    return KvAllocator::global(group_id)->map_imported_slots(offsets, n, fds, n_fds) ? KVC_OK
                                                                                      : fail(KVC_E_NOT_CREATED, "KV tensors are not created");
  });
}
int kvc_export_page_ids(const int64_t *offsets, size_t n, int64_t group_id, int *out_fds, int64_t *out_meta, int64_t cap) {
  return guarded([&]() -> int { return KvAllocator::global(group_id)->export_page_ids(offsets, n, out_fds, out_meta, cap); });
}
int kvc_map_imported_page_ids(const int64_t *offsets, size_t n, int64_t group_id, const int *fds, size_t n_fds, const int64_t *meta) {
  return guarded([&]() -> int {
    return KvAllocator::global(group_id)->map_imported_page_ids(offsets, n, fds, n_fds, meta) ? KVC_OK
                                                                                          : fail(KVC_E_NOT_CREATED, "KV tensors are not created");
  });
}

} // extern "C"
