// kv_selftest.cpp — the start-up self tests of KvAllocator::init() (see kv_allocator.hpp).
#include "kv_allocator_impl.hpp"

#include "kernels.hpp"

namespace kvc {

// The hybrid backend rests on one property of the HIP runtime: once it has recorded a mapping for a VA it keeps
// addressing that VA in copies and memsets, whatever ROCr has mapped there since. Checked once per init on a
// scratch page (a few hundred microseconds): placeholder mapped through HIP and removed through ROCr, a real page
// mapped through ROCr, written with hipMemset and read back with hipMemcpy. Any surprise -> the plain HIP backend.
bool hybrid_self_test(int dev) {
  if (KVC_TEST_HOOK("FAIL_HYBRID_SELFTEST")) return false; // tests: exercise the fallback
  const size_t ps = kBasePage;
  void *va = nullptr;
  hipMemGenericAllocationHandle_t shell = nullptr;
  hsa_amd_vmem_alloc_handle_t real{};
  bool have_real = false, hip_mapped = false, rocr_mapped = false, ok = false;
  try {
    const HsaDevice &hd = hsa_device(dev);
    auto prop = make_alloc_prop(dev, false);
    if (hipMemAddressReserve(&va, ps, ps, nullptr, 0) != hipSuccess) throw 1;
    if (hipMemCreate(&shell, ps, &prop, 0) != hipSuccess) throw 2;
    if (hipMemMap(va, ps, 0, shell, 0) != hipSuccess) throw 3;
    hip_mapped = true;
    if (hsa_amd_vmem_unmap(va, ps) != HSA_STATUS_SUCCESS) throw 4;
    if (hsa_amd_vmem_handle_create(hd.pool, ps, MEMORY_TYPE_PINNED, 0, &real) != HSA_STATUS_SUCCESS) throw 5;
    have_real = true;
    if (hsa_amd_vmem_map(va, ps, 0, real, 0) != HSA_STATUS_SUCCESS) throw 6;
    rocr_mapped = true;
    hsa_amd_memory_access_desc_t d{HSA_ACCESS_PERMISSION_RW, hd.agent};
    if (hsa_amd_vmem_set_access(va, ps, &d, 1) != HSA_STATUS_SUCCESS) throw 7;
    unsigned char host[256];
    memset(host, 0, sizeof host);
    if (hipMemset(va, 0x5a, sizeof host) != hipSuccess) throw 8;
    if (hipMemcpy(host, va, sizeof host, hipMemcpyDeviceToHost) != hipSuccess) throw 9;
    for (unsigned char c : host)
      if (c != 0x5a) throw 10;
    memset(host, 0xc3, sizeof host);
    if (hipMemcpy(static_cast<char *>(va) + 4096, host, sizeof host, hipMemcpyHostToDevice) != hipSuccess) throw 11;
    unsigned char back[256];
    if (hipMemcpy(back, static_cast<char *>(va) + 4096, sizeof back, hipMemcpyDeviceToHost) != hipSuccess) throw 12;
    if (memcmp(back, host, sizeof back) != 0) throw 13;
    ok = true;
  } catch (int step) {
    KVC_LOG(LOG_WARNING, "hybrid VMM self test stopped at step %d", step);
  } catch (const std::exception &e) {
    KVC_LOG(LOG_WARNING, "hybrid VMM self test: %s", e.what());
  }
  (void)hipGetLastError();
  // teardown in the order HIP expects: something mapped at the VA, HIP unmaps it
  if (hip_mapped) {
    if (!rocr_mapped && have_real) rocr_mapped = hsa_amd_vmem_map(va, ps, 0, real, 0) == HSA_STATUS_SUCCESS;
    if (hipMemUnmap(va, ps) != hipSuccess) {
      (void)hipGetLastError();
      if (rocr_mapped) (void)hsa_amd_vmem_unmap(va, ps);
    }
  }
  { // the page was written through this VA: its translation must not outlive it (the page goes back below, and the
    // VA may be handed out again for a region whose first map no longer invalidates by itself)
    void *p = nullptr;
    if (!KVC_TEST_HOOK("SKIP_TEARDOWN_FLUSH") && hipMalloc(&p, kBasePage) == hipSuccess) (void)hipFree(p);
    (void)hipGetLastError();
  }
  if (have_real) (void)hsa_amd_vmem_handle_release(real);
  if (shell) (void)hipMemRelease(shell);
  if (va) (void)hipMemAddressFree(va, ps);
  (void)hipGetLastError();
  return ok;
}

// The drm backend edits the process's GPU page tables through libdrm_amdgpu, next to ROCr (DrmVm, hip_vmm.hpp).
// Before any page is served that way, prove on one slot that (1) the amdgpu_device libdrm handed us drives the SAME
// address space as ROCr - a GEM_VA map over a VA that ROCr has mapped must be refused, and accepted once ROCr has
// unmapped it; this step touches no memory, so a wrong VM cannot fault - and (2) data follows the handle: two pages
// swapped under one VA keep their own contents, seen through HIP's memset/copy on a HIP-registered slot.
bool drm_self_test(int dev) {
  if (KVC_TEST_HOOK("FAIL_DRM_SELFTEST")) return false; // tests: exercise the fallback
  std::string why;
  DrmVm &vm = DrmVm::instance();
  if (!vm.open(dev, &why)) {
    KVC_LOG(LOG_WARNING, "direct DRM mapping unavailable: %s", why.c_str());
    return false;
  }
  const size_t ps = kBasePage;
  void *va = nullptr;
  hipMemGenericAllocationHandle_t shell = nullptr;
  hsa_amd_vmem_alloc_handle_t a{}, b{};
  bool have_a = false, have_b = false, hip_mapped = false, rocr_mapped = false, ok = false;
  void *drm_mapped = nullptr; // the bo currently mapped at va through DRM
  auto shootdown = [&]() {
    void *p = nullptr;
    if (hipMalloc(&p, kBasePage) == hipSuccess) (void)hipFree(p);
  };
  try {
    const HsaDevice &hd = hsa_device(dev);
    auto prop = make_alloc_prop(dev, false);
    if (hipMemAddressReserve(&va, ps, ps, nullptr, 0) != hipSuccess) throw 1;
    if (hipMemCreate(&shell, ps, &prop, 0) != hipSuccess) throw 2;
    if (hipMemMap(va, ps, 0, shell, 0) != hipSuccess) throw 3;
    hip_mapped = true;
    if (hsa_amd_vmem_unmap(va, ps) != HSA_STATUS_SUCCESS) throw 4;
    if (hsa_amd_vmem_handle_create(hd.pool, ps, MEMORY_TYPE_PINNED, 0, &a) != HSA_STATUS_SUCCESS) throw 5;
    have_a = true;
    if (hsa_amd_vmem_handle_create(hd.pool, ps, MEMORY_TYPE_PINNED, 0, &b) != HSA_STATUS_SUCCESS) throw 6;
    have_b = true;
    if (!vm.adopt(a.handle) || !vm.adopt(b.handle)) throw 7;
    void *bo_a = vm.find(a.handle), *bo_b = vm.find(b.handle);
    // (1) same address space?
    if (hsa_amd_vmem_map(va, ps, 0, a, 0) != HSA_STATUS_SUCCESS) throw 8;
    rocr_mapped = true;
    hsa_amd_memory_access_desc_t d{HSA_ACCESS_PERMISSION_RW, hd.agent};
    if (hsa_amd_vmem_set_access(va, ps, &d, 1) != HSA_STATUS_SUCCESS) throw 9;
    if (vm.map(bo_b, va, ps) == 0) { // accepted: libdrm gave us some other VM
      (void)vm.unmap(bo_b, va, ps);
      throw 10;
    }
    if (hsa_amd_vmem_unmap(va, ps) != HSA_STATUS_SUCCESS) throw 11;
    rocr_mapped = false;
    if (vm.map(bo_b, va, ps) != 0) throw 12;
    drm_mapped = bo_b;
    // (2) data follows the handle
    shootdown();
    unsigned char host[256];
    if (hipMemset(va, 0x5a, sizeof host) != hipSuccess || hipDeviceSynchronize() != hipSuccess) throw 13;
    if (vm.unmap(bo_b, va, ps) != 0) throw 14;
    drm_mapped = nullptr;
    if (vm.map(bo_a, va, ps) != 0) throw 15;
    drm_mapped = bo_a;
    shootdown();
    if (hipMemset(va, 0xc3, sizeof host) != hipSuccess || hipDeviceSynchronize() != hipSuccess) throw 16;
    memset(host, 0, sizeof host);
    if (hipMemcpy(host, va, sizeof host, hipMemcpyDeviceToHost) != hipSuccess) throw 17;
    for (unsigned char c : host)
      if (c != 0xc3) throw 18;
    if (vm.unmap(bo_a, va, ps) != 0) throw 19;
    drm_mapped = nullptr;
    if (vm.map(bo_b, va, ps) != 0) throw 20;
    drm_mapped = bo_b;
    shootdown();
    if (hipMemcpy(host, va, sizeof host, hipMemcpyDeviceToHost) != hipSuccess) throw 21;
    for (unsigned char c : host)
      if (c != 0x5a) throw 22;
    ok = true;
    // (3) optional on top: physical memory straight from KFD (flat creation cost). Its failure only means that
    // handles keep coming from ROCr.
    if (vm.unmap(bo_b, va, ps) != 0) throw 23;
    drm_mapped = nullptr;
    bool kfd_ok = false;
    if (env_option("KVCACHED_DRM_KFD_CREATE") && !KVC_TEST_HOOK("FAIL_KFD_SELFTEST")) {
      std::string why_kfd;
      phys_handle_t k = 0;
      int step = 0;
      try {
        if (!vm.open_kfd(&why_kfd)) throw 1;
        k = vm.create(ps);
        void *bo_k = vm.find(k);
        if (!bo_k || vm.map(bo_k, va, ps) != 0) throw 2;
        drm_mapped = bo_k;
        shootdown();
        if (hipMemset(va, 0x77, sizeof host) != hipSuccess || hipDeviceSynchronize() != hipSuccess) throw 3;
        if (hipMemcpy(host, va, sizeof host, hipMemcpyDeviceToHost) != hipSuccess) throw 4;
        for (unsigned char c : host)
          if (c != 0x77) throw 5;
        if (vm.unmap(bo_k, va, ps) != 0) throw 6;
        drm_mapped = nullptr;
        shootdown();
        kfd_ok = true;
      } catch (int st) {
        step = st;
      } catch (const std::exception &e) {
        why_kfd = e.what();
        step = -1;
      }
      (void)hipGetLastError();
      if (drm_mapped) {
        (void)vm.unmap(drm_mapped, va, ps);
        drm_mapped = nullptr;
      }
      if (k) (void)vm.forget(k);
      if (!kfd_ok)
        KVC_LOG(LOG_WARNING, "physical pages straight from KFD unavailable (step %d%s%s): creating them through ROCr", step,
                why_kfd.empty() ? "" : ": ", why_kfd.c_str());
    }
    if (!kfd_ok) vm.disable_kfd();
  } catch (int step) {
    KVC_LOG(LOG_WARNING, "direct DRM mapping self test stopped at step %d", step);
  } catch (const std::exception &e) {
    KVC_LOG(LOG_WARNING, "direct DRM mapping self test: %s", e.what());
  }
  (void)hipGetLastError();
  if (drm_mapped) (void)vm.unmap(drm_mapped, va, ps);
  if (hip_mapped) { // HIP must find something to unmap
    if (!rocr_mapped && have_a) rocr_mapped = hsa_amd_vmem_map(va, ps, 0, a, 0) == HSA_STATUS_SUCCESS;
    if (hipMemUnmap(va, ps) != hipSuccess) {
      (void)hipGetLastError();
      if (rocr_mapped) (void)hsa_amd_vmem_unmap(va, ps);
    }
  }
  shootdown();
  if (have_a) {
    vm.forget(a.handle);
    (void)hsa_amd_vmem_handle_release(a);
  }
  if (have_b) {
    vm.forget(b.handle);
    (void)hsa_amd_vmem_handle_release(b);
  }
  if (shell) (void)hipMemRelease(shell);
  if (va) (void)hipMemAddressFree(va, ps);
  (void)hipGetLastError();
  return ok;
}

// Does the TLB invalidation in effect (GpuContext::tlb_shootdown: the KFD ioctl pair, or its hipMalloc fallback)
// really invalidate, with the backend in effect? Two pages swapped under one VA, looked at through the GPU's own
// address translation (a one-lane kernel): after A has been used through the VA and B mapped in its place, a write
// through the VA must land in B - if it lands in A (found when A is mapped back), the translation survived the
// invalidation, and pages recycled between requests or engines would leak into each other. No fallback makes that
// acceptable: init fails (tests/test_gpu_vmm.py::test_init_refuses_to_start_when_tlb_invalidation_is_ineffective
// breaks the flush with a hook and expects exactly that).
void tlb_self_test(GpuContext *ctx) {
  const size_t ps = kBasePage;
  const int dev = ctx->dev();
  void *va = nullptr;
  unsigned *out = nullptr;
  phys_handle_t a = 0, b = 0, mapped = 0;
  std::string failure;
  auto look = [&](unsigned value, bool write) -> unsigned {
    unsigned host = 0;
    HIP_CHECK(launch_peek_poke(va, out, value, write, ctx->stream()));
    HIP_CHECK(hipStreamSynchronize(ctx->stream()));
    HIP_CHECK(hipMemcpy(&host, out, sizeof host, hipMemcpyDeviceToHost));
    return host;
  };
  auto put = [&](phys_handle_t h) {
    if (vmm_map(va, ps, h)) vmm_set_access(va, ps, dev);
    mapped = h;
  };
  auto take = [&]() {
    vmm_unmap(va, ps, mapped);
    mapped = 0;
  };
  try {
    va = vmm_reserve(ps, ps, nullptr);
    HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&out), 64));
    a = vmm_create(dev, ps, false);
    b = vmm_create(dev, ps, false);
    put(a);
    if (look(0x5a5a5a5au, true) != 0x5a5a5a5au) throw GpuError("a freshly mapped page does not read back what was written");
    take();
    put(b);               // the VA's translation to A may still be cached ...
    ctx->tlb_shootdown(); // ... until now (the path every unmap batch takes)
    if (look(0xc3c3c3c3u, true) != 0xc3c3c3c3u) throw GpuError("the second page does not read back what was written");
    take();
    put(a);
    ctx->tlb_shootdown();
    const unsigned seen = look(0, false);
    if (seen != 0x5a5a5a5au) {
      char buf[200];
      snprintf(buf, sizeof buf, "a write through a re-mapped VA landed in the page that had been unmapped (0x%08x where 0x5a5a5a5a "
               "was expected): the GPU kept a stale translation across the invalidation", seen);
      failure = buf;
    }
  } catch (const std::exception &e) {
    failure = e.what();
  }
  (void)hipGetLastError();
  if (mapped) (void)vmm_try_unmap(va, ps, mapped);
  try {
    ctx->tlb_shootdown(); // the scratch pages were touched through this VA: nothing of it may survive them
  } catch (...) {
  }
  if (a) (void)vmm_try_release(a);
  if (b) (void)vmm_try_release(b);
  if (out) (void)hipFree(out);
  if (va) (void)vmm_try_address_free(va, ps);
  (void)hipGetLastError();
  if (!failure.empty())
    throw GpuError("kvcached_amd: TLB invalidation is ineffective on this system (" + failure +
                   "). Pages could leak between requests and co-located engines: refusing to start.");
}

} // namespace kvc
