// kv_regions.cpp — making and destroying regions, their rest state, HIP registration (see kv_allocator.hpp).
#include "kv_allocator_impl.hpp"

#include <sys/mman.h>

#include <algorithm>

namespace kvc {

std::unique_ptr<KvRegion> KvAllocator::make_region(const std::string &name, size_t size, size_t page_size) {
  if (size % kBasePage != 0) throw InvalidError("alloc size not aligned.");
  auto r = std::make_unique<KvRegion>();
  r->name = name;
  r->size = size;
  r->page_size = page_size;
  r->on_gpu = dev_.is_gpu;
  if (size % page_size != 0) throw InvalidError("region size is not a multiple of its page size");
  size_t off = g_vaddr_offset.fetch_add(size);
  void *hint = reinterpret_cast<void *>(kStartAddr + off);
  if (dev_.is_gpu) {
    r->base = static_cast<char *>(vmm_reserve(size, kBasePage, hint));
  } else {
    void *p = mmap(hint, size, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (p == MAP_FAILED) throw InvalidError("mmap failed.");
    r->base = static_cast<char *>(p);
  }
  r->handle.assign(r->num_slots(), phys_handle_t{});
  r->seq.assign(r->num_slots(), 0);
  r->stale_epoch.assign(r->num_slots(), 0);
  r->mapped.assign(r->num_slots(), Unbacked);
  r->mark.assign((r->num_slots() + 63) / 64, 0);
  r->registered.assign(r->num_slots(), 0);
  r->reg_group = std::max<size_t>(1, (size_t)std::max<int64_t>(0, options().hip_reg_group_mb.load()) * (1u << 20) / r->page_size);
  return r;
}

// reference: FTensor::init_with_zero_ (ftensor.cpp:160-176) — every unbacked slot aliases a physical
// page of zeros so that stray reads do not fault. The reference uses ONE such page for the whole
// reservation; on ROCm hipMemUnmap of an alias costs O(aliases of that handle) (~6 ns each: 37 us
// per slot at 6k aliases, 220-260 us at 32k, ~1 ms at the 147k slots of a 288 GiB reservation), so
// the zero page is sharded: one handle per `fanout` slots (default 256 => 0.4 % of the VA size).
// The rest state of unbacked slots on the drm backend where reads of them must not fault: PRT (DrmVm::map_prt), one
// mapping per group of 64 slots. Default in compat mode. NOT in lazy mode: a PRT translation IS cached by the TLBs once something
// has looked at the address (tools/prt_tlb_probe.cpp: every read stale and 0.8 % of the writes lost after backing such
// slots without an invalidation), so backing a PRT slot owes an invalidation before the page is used - and lazy mode's
// contract (nothing touches unbacked VA) is what makes its map path free of one: plain unmapped VA, where a violation
// faults instead of poisoning the next mapping. KVCACHED_PRT=true|false overrides either default.
bool KvAllocator::prt_all(KvRegion &r, bool by_default) {
  if (!dev_.is_gpu || vmm_backend() != kVmmDrm || !DrmVm::instance().can_clear() || !env_flag("KVCACHED_PRT", by_default)) return false;
  hipDeviceProp_t prop{};
  if (hipGetDeviceProperties(&prop, ctx_->dev()) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    (void)hipGetLastError();
    return false; // what a PRT page does to a load is a property of the GPU: checked on gfx950 (tools/prt_probe.cpp), nowhere else
  }
  // HIP must have been introduced to every slot BEFORE the range is occupied (its placeholder mapping cannot overlap ours)
  for (size_t i = 0; i < r.num_slots(); ++i)
    if (vmm_hip_registered()) register_slot(r, i);
  // One mapping per group of 64 slots (2 304 ioctls for the 147 k slots of a 288 GiB reservation), not one for the region:
  // a page-table entry carries a fragment size that may be as large as its MAPPING, and when a mapping is split what is
  // left of it has to be written again (DrmVm::refresh_prt_remainders). Runs that go back to PRT later are one mapping of
  // up to KvRegion::kPrtRunSlots (1024) slots; rewriting what a split leaves of one costs 17 us against 11 us for a
  // 64-slot group (profiles/r04_prt_run_probe.log): it grows with the length, slowly.
  const size_t group = KvRegion::kPrtGroupSlots * r.page_size;
  for (size_t off = 0; off < r.size; off += group) {
    const int rc = DrmVm::instance().map_prt(r.base + off, std::min(group, r.size - off));
    if (rc != 0) {
      KVC_LOG(LOG_WARNING, "PRT mapping refused (%s): unbacked slots fall back to %s", strerror(rc < 0 ? -rc : rc),
              options().zero_backfill.load() ? "zero aliases" : "unmapped VA");
      if (off) {
        StaleAfter mark;
        (void)DrmVm::instance().clear(r.base, off);
      }
      return false;
    }
  }
  r.prt = true;
  return true;
}

int KvAllocator::rest_replace(KvRegion &r, size_t first, size_t n) {
  StaleAfter mark; // whatever was mapped there was a live translation
  char *va = r.base + first * r.page_size;
  if (r.prt) return DrmVm::instance().map_prt(va, n * r.page_size, /*replace=*/true);
  return DrmVm::instance().replace(DrmVm::instance().find(r.zx_handle), va, n * r.page_size, (first % r.zx_pages) * r.page_size);
}

int KvAllocator::rest_map(KvRegion &r, size_t first, size_t n) {
  char *va = r.base + first * r.page_size;
  if (r.prt) return DrmVm::instance().map_prt(va, n * r.page_size);
  return DrmVm::instance().map(DrmVm::instance().find(r.zx_handle), va, n * r.page_size, (first % r.zx_pages) * r.page_size);
}

void KvAllocator::backfill_all(KvRegion &r) {
  if (prt_all(r, true)) { // "reads as zeros" from the page tables themselves: no zero page to keep and to alias
    r.backfilled = true;
    return;
  }
  // drm backend: one buffer of zeros, a whole group of slots aliased per ioctl, no per-slot object anywhere (§4.2):
  // 2 304 ioctls for the 147 k slots of a 288 GiB reservation instead of 147 k map + set_access pairs.
  if (env_option("KVCACHED_ZERO_EXTENT")) {
    size_t zp = 0;
    if (const phys_handle_t zh = ctx_->zero_extent(r.page_size, &zp)) {
      void *zbo = DrmVm::instance().find(zh);
      size_t done = 0;
      try {
        for (size_t i = 0; i < r.num_slots(); ++i)
          if (vmm_hip_registered()) register_slot(r, i); // compat promises zeros to ANY access, hipMemcpy included
        for (; done < r.num_slots(); done += zp) {
          const size_t k = std::min(zp, r.num_slots() - done);
          if (DrmVm::instance().map(zbo, r.base + done * r.page_size, k * r.page_size, 0) != 0)
            throw GpuError("aliasing the zero extent failed");
        }
      } catch (...) {
        if (done) {
          StaleAfter mark;
          (void)DrmVm::instance().clear(r.base, std::min(done, r.num_slots()) * r.page_size);
        }
        throw;
      }
      r.zx = true;
      r.zx_handle = zh;
      r.zx_pages = zp;
      r.backfilled = true;
      return; // invalid -> valid: nothing to invalidate; the extent was filled when it was made
    }
  }
  r.fanout = (size_t)std::max<int64_t>(1, options().zero_alias_fanout.load());
  const size_t n_zero = (r.num_slots() + r.fanout - 1) / r.fanout;
  r.zero.assign(n_zero, phys_handle_t{});
  size_t made = 0;
  try {
    for (; made < n_zero; ++made) r.zero[made] = vmm_create(ctx_->dev(), r.page_size, false, /*direct=*/false);
    const size_t run = (size_t)std::max<int64_t>(1, options().access_run_slots.load());
    for (size_t i = 0; i < r.num_slots(); ++i) {
      if (vmm_hip_registered()) register_slot(r, i); // compat promises zeros to ANY access, hipMemcpy included
      vmm_map(r.base + i * r.page_size, r.page_size, r.zero_of(i));
    }
    for (size_t i = 0; i < r.num_slots(); i += run) {
      size_t k = std::min(run, r.num_slots() - i);
      vmm_set_access(r.base + i * r.page_size, k * r.page_size, ctx_->dev());
    }
  } catch (...) {
    (void)vmm_try_unmap(r.base, r.size);
    try {
      ctx_->tlb_shootdown(); // the aliases were live translations
    } catch (...) {
    }
    for (size_t j = 0; j < made; ++j) (void)vmm_try_release(r.zero[j]);
    r.zero.clear();
    (void)hipGetLastError();
    throw;
  }
  r.backfilled = true;
  // the driver hands out zeroed memory today, but that is not a documented guarantee: fill each
  // zero page once, through its first alias
  ctx_->tlb_shootdown();
  std::vector<void *> firsts;
  for (size_t z = 0; z < n_zero; ++z) firsts.push_back(r.base + z * r.fanout * r.page_size);
  ctx_->zero_fill(firsts.data(), firsts.size(), r.page_size, nullptr);
  ctx_->sync(nullptr);
}

// Hybrid backend. HIP resolves a device pointer through its own table of allocations and mappings; a VA that only
// ROCr knows is "pageable host memory" to hipMemcpy. So each slot is introduced to HIP once: hipMemMap of a placeholder
// handle at the slot's VA (HIP records VA -> memory object), then hsa_amd_vmem_unmap of that very mapping (ROCr's
// state: nothing mapped; HIP never looks again). Every later backing of the slot goes through ROCr only. HIP's copy
// engines address memory by VA and the hardware walks the page tables ROCr maintains, so all hipMemcpy flavours keep
// working, at full speed (tools/hsa_vmm_probe.cpp op 8: D2H 32-50 GB/s, 0 wrong words over re-backing rounds).
// One placeholder per `fanout` slots (as for the zero pages) keeps the number of mappings HIP hangs off one handle
// small. Cost: hipMemMap 3 us + unmap 3 us, once per slot per region lifetime.
void KvAllocator::register_slot(KvRegion &r, size_t slot) {
  if (r.registered[slot]) return;
  constexpr size_t kShellFanout = 4096; // mappings per placeholder handle
  auto prop = make_alloc_prop(ctx_->dev(), false);
  // One hipMemMap introduces a whole group of slots (64 MiB of VA): a slot is registered the first time ANY slot of
  // its group is backed, so nothing can be mapped inside the group at this point. The registration costs the same
  // ~3 us per call whatever its size, i.e. 0.1 us per slot instead of 3.3.
  const bool group = r.in_full_group(slot);
  const size_t first = group ? slot / r.reg_group * r.reg_group : slot, count = group ? r.reg_group : 1;
  auto &shells = group ? r.shell_group : r.shell;
  const size_t tail_base = r.reg_group > 1 ? r.num_slots() / r.reg_group * r.reg_group : 0; // slots behind the last full group
  const size_t shard = (group ? slot / r.reg_group : slot - tail_base) / kShellFanout;
  if (shells.size() <= shard) shells.resize(shard + 1, nullptr);
  if (!shells[shard]) HIP_CHECK(hipMemCreate(&shells[shard], count * r.page_size, &prop, 0));
  char *va = r.base + first * r.page_size;
  HIP_CHECK(hipMemMap(va, count * r.page_size, 0, shells[shard], 0));
  HSA_CHECK(hsa_amd_vmem_unmap(va, count * r.page_size));
  for (size_t i = first; i < first + count; ++i) r.registered[i] = 1;
}

// Teardown of the above: HIP believes its placeholder mappings are still there and must be allowed to unmap them
// (hipMemAddressFree and hipMemRelease expect that). Everything of ours inside a registered unit - pages, zero aliases -
// is unmapped first; then a stand-in of the unit's size is mapped through ROCr for HIP's unmap to remove.
void KvAllocator::unregister_slots(KvRegion &r) {
  if (r.rest_direct()) { // pages and the rest state (PRT, zero aliases) alike are DRM mappings of ours: one ranged CLEAR drops them all
    StaleAfter mark;
    if (DrmVm::instance().clear(r.base, r.size) != 0) KVC_LOG(LOG_ERROR, "dropping the mappings of %s failed", r.name.c_str());
  }
  hsa_amd_vmem_alloc_handle_t standin[2] = {{}, {}}; // [0] one slot, [1] one group
  bool have_standin[2] = {false, false};
  size_t failures = 0;
  for (size_t first = 0; first < r.num_slots();) {
    const bool group = r.in_full_group(first);
    const size_t count = group ? r.reg_group : 1;
    if (!r.registered[first]) {
      first += count;
      continue;
    }
    char *va = r.base + first * r.page_size;
    for (size_t i = first; i < first + count; ++i) {
      char *sva = r.base + i * r.page_size;
      if (r.rest_direct()) continue; // (cleared above)
      if (r.mapped[i]) {
        if (!vmm_try_unmap(sva, r.page_size, r.handle[i])) KVC_LOG(LOG_ERROR, "unmap during cleanup failed (slot %zu)", i);
      } else if (r.backfilled) {
        (void)vmm_try_unmap(sva, r.page_size); // a zero alias
      }
    }
    const int k = group ? 1 : 0;
    if (!have_standin[k])
      have_standin[k] = hsa_amd_vmem_handle_create(hsa_device(ctx_->dev()).pool, count * r.page_size, MEMORY_TYPE_PINNED, 0,
                                                   &standin[k]) == HSA_STATUS_SUCCESS;
    if (!have_standin[k] || hsa_amd_vmem_map(va, count * r.page_size, 0, standin[k], 0) != HSA_STATUS_SUCCESS) {
      failures += count;
    } else if (hipMemUnmap(va, count * r.page_size) != hipSuccess) {
      (void)hipGetLastError();
      (void)hsa_amd_vmem_unmap(va, count * r.page_size);
      failures += count;
    }
    for (size_t i = first; i < first + count; ++i) r.registered[i] = 0;
    first += count;
  }
  for (int k = 0; k < 2; ++k)
    if (have_standin[k]) (void)hsa_amd_vmem_handle_release(standin[k]);
  for (auto *shells : {&r.shell, &r.shell_group}) {
    for (auto h : *shells)
      if (h && hipMemRelease(h) != hipSuccess) (void)hipGetLastError();
    shells->clear();
  }
  if (failures) KVC_LOG(LOG_ERROR, "%zu slots of %s could not be unregistered from HIP", failures, r.name.c_str());
}

void KvAllocator::destroy_region(KvRegion &r) {
  if (!r.base) return;
  if (!r.on_gpu) {
    munmap(r.base, r.size);
    r.base = nullptr;
    return;
  }
  GpuContext *ctx = ctx_;
  if (ctx) (void)hipSetDevice(ctx->dev());
  // Tolerate stale mappings during teardown: log, do not throw (ftensor.cpp:78-98).
  bool whole = false;
  if (vmm_hip_registered()) {
    // HIP unmaps every slot it was told about (that removes our pages' and aliases' mappings too); what was never
    // registered cannot be mapped either
    unregister_slots(r);
    whole = true;
  } else if (r.backfilled) {
    whole = vmm_try_unmap(r.base, r.size);
    if (!whole) KVC_LOG(LOG_ERROR, "unmapping the whole region %s in one call failed", r.name.c_str());
  }
  std::vector<Phys> dead, pieces; // dead: a peer's pages (imports); pieces: our own, which go home through their pool
  ExtentPool *pp = ctx ? ctx->extents(r.page_size, exportable_) : nullptr;
  for (size_t i = 0; i < r.num_slots(); ++i) {
    if (!r.mapped[i]) continue;
    if (!whole) {
      if (!vmm_try_unmap(r.base + i * r.page_size, r.page_size, r.handle[i])) KVC_LOG(LOG_ERROR, "unmap during cleanup failed (slot %zu)", i);
    }
    if (r.mapped[i] != Lane && r.mapped[i] != PeerLane) // (a page of a lane / of a peer's lane is released once, from ~KvAllocator, not once per row)
      (r.mapped[i] != Imported ? pieces : dead).push_back(Phys{r.handle[i], r.seq[i]});
    r.mapped[i] = Unbacked;
  }
  std::sort(dead.begin(), dead.end(), [](const Phys &a, const Phys &b) { return a.seq < b.seq; }); // oldest first
  if (r.backfilled && !whole) // aliases that could not be dropped in one call
    for (size_t i = 0; i < r.num_slots(); ++i) (void)vmm_try_unmap(r.base + i * r.page_size, r.page_size);
  // Pages and zero pages leave the process and the VA range may be handed out again: no translation of either may
  // survive (any unmap above has set tlb_stale(); a region that never had anything mapped owes nothing).
  if (ctx && tlb_stale().load() && !KVC_TEST_HOOK("SKIP_TEARDOWN_FLUSH")) { // hook: prove the test has teeth
    try {
      ctx->tlb_shootdown();
    } catch (...) {
      (void)hipGetLastError();
    }
  }
  for (auto &p : dead) {
    if (!vmm_try_release(p.h)) KVC_LOG(LOG_ERROR, "releasing a physical handle during cleanup failed");
    stats().vmm.released++;
  }
  if (!pieces.empty()) {
    pp->release_batch(pieces.data(), pieces.size());
    pp->drain(0); // a region that goes away gives its memory back (the reference releases in ~FTensor, ftensor.cpp:78-98)
  }
  for (auto z : r.zero) (void)vmm_try_release(z);
  r.zero.clear();
  if (!vmm_try_address_free(r.base, r.size)) KVC_LOG(LOG_ERROR, "freeing the VA range of %s failed", r.name.c_str());
  (void)hipGetLastError();
  r.base = nullptr;
}

} // namespace kvc
