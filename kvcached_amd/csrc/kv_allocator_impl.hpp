// kv_allocator_impl.hpp — what the translation units of KvAllocator share with each other and with nobody else:
// kv_allocator.cpp (registry, lifetime, reclaimer, the entry points), kv_selftest.cpp, kv_regions.cpp, kv_map_paths.cpp,
// kv_lanes.cpp, kv_share.cpp. Declarations only, plus one template.
#pragma once

#include "kv_allocator.hpp"
#include "run_scan.hpp"

namespace kvc {

using SlotRun = SlotRunOf<KvRegion>;
using RunScan = RunScanOf<KvRegion>;

// kv_allocator.cpp
extern std::atomic<size_t> g_vaddr_offset;        // running offset behind kStartAddr (reference: ftensor.cpp:17)
extern std::atomic<size_t> g_pending_unmap_bytes; // async unmap: released by the caller, not yet by the driver

// kv_selftest.cpp: KvAllocator::init() runs them once per init
bool hybrid_self_test(int dev);
bool drm_self_test(int dev);
void tlb_self_test(GpuContext *ctx);

// kv_share.cpp: pages imported straight into KFD + DRM / through ROCr or HIP (import_count)
extern std::atomic<int64_t> g_imports_direct, g_imports_runtime;

// kv_map_paths.cpp
void settle_batch(GpuContext *ctx, size_t ps, bool &prt_dirty, void *&zx_dirty, uint64_t &need_epoch, bool replaced);

// A map batch failed: `undo` takes its mappings back - once no fill can still be running on the pages that go - and no
// translation of them is left behind, nor the error HIP remembers.
template <class Undo> void roll_back(GpuContext *ctx, bool launched, Undo &&undo) {
  if (launched) (void)hipStreamSynchronize(ctx->stream());
  undo();
  (void)hipGetLastError();
  try {
    ctx->tlb_shootdown();
  } catch (...) {
  }
}

} // namespace kvc
