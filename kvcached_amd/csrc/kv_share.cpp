// kv_share.cpp — TP shared pool, slot by slot: import of a peer's pages, export of ours (see kv_allocator.hpp).
#include "kv_allocator_impl.hpp"

#include <fcntl.h>
#include <unistd.h>

namespace kvc {

// ------------------------------------------------------------------ TP shared pool
// hipMemImportFromShareableHandle's `osHandle` convention differs between HIP runtimes: the one
// bundled with PyTorch 2.10+rocm7.0 dereferences it as `int *` (passing the fd by value
// segfaults inside amd::roc::Device::ImportShareableHSAHandle), ROCm 7.2's takes the fd by value
// like CUDA. The pointer form is tried first: a by-value runtime reads the pointer's bits as a
// (huge, invalid) fd number and fails cleanly, after which the by-value form is used.
namespace {
std::atomic<int> g_import_convention{0}; // 0 unknown, 1 pointer to fd, 2 fd by value
}
std::atomic<int64_t> g_imports_direct{0}, g_imports_runtime{0}; // pages imported straight into KFD + DRM / through ROCr or HIP
int64_t import_count(bool direct) { return direct ? g_imports_direct.load() : g_imports_runtime.load(); }
static phys_handle_t import_posix_fd(int fd) {
  if (fd < 0 || fcntl(fd, F_GETFD) == -1) throw InvalidError("import of an invalid file descriptor");
  if (vmm_backend() == kVmmDrm && DrmVm::instance().kfd_ready() && env_option("KVCACHED_DRM_KFD_IMPORT")) {
    // straight into KFD + DRM: mapped with one ioctl like our own pages. A buffer that lives on ANOTHER GPU (rank 0's
    // pages seen from a peer over xGMI) may be refused by this shortcut - ROCr's import, which sets up peer access for
    // the local agent, is the fallback (hsa_amd_vmem_import_shareable_handle + map + set_access below).
    try {
      if (KVC_TEST_HOOK("FAIL_KFD_IMPORT")) throw GpuError("AMDKFD_IOC_IMPORT_DMABUF failed [injected]");
      const phys_handle_t h = DrmVm::instance().import_fd(fd);
      ++g_imports_direct;
      return h;
    } catch (const GpuError &e) {
      static std::atomic<bool> warned{false};
      if (!warned.exchange(true))
        KVC_LOG(LOG_WARNING, "direct import of a shared page failed (%s): importing through ROCr from now on", e.what());
    }
  }
  ++g_imports_runtime;
  if (vmm_uses_rocr()) { // ROCr takes the dmabuf fd by value
    hsa_amd_vmem_alloc_handle_t hh{};
    HSA_CHECK(hsa_amd_vmem_import_shareable_handle(fd, &hh));
    return hh.handle;
  }
  hipMemGenericAllocationHandle_t h{};
  int conv = g_import_convention.load();
  if (conv != 2) {
    alignas(8) static thread_local int slot;
    slot = fd;
    hipError_t st = hipMemImportFromShareableHandle(&h, static_cast<void *>(&slot), hipMemHandleTypePosixFileDescriptor);
    if (st == hipSuccess) {
      g_import_convention = 1;
      return reinterpret_cast<phys_handle_t>(h);
    }
    (void)hipGetLastError();
    int rt = 0;
    (void)hipRuntimeGetVersion(&rt);
    // runtimes before 7.1 are known to dereference: never hand them a small integer as a pointer
    if (conv == 1 || rt < 70100000) hip_check(st, "hipMemImportFromShareableHandle(&h, &fd, posix_fd)", __FILE__, __LINE__);
  }
  HIP_CHECK(hipMemImportFromShareableHandle(&h, reinterpret_cast<void *>(static_cast<uintptr_t>(fd)),
                                            hipMemHandleTypePosixFileDescriptor));
  g_import_convention = 2;
  return reinterpret_cast<phys_handle_t>(h);
}

int KvAllocator::export_mapped_slots(const offset_t *offsets, size_t n, int *out_fds, int64_t cap) {
  std::lock_guard<std::mutex> g(mu_);
  if (!dev_.is_gpu) throw NoGpuError("export_mapped_slots needs a GPU device");
  if (!exportable_) throw InvalidError("handles are not exportable: set KVCACHED_EXPORTABLE_HANDLES=1 before init");
  auto slots = slots_for(offsets, n);
  if ((int64_t)slots.size() > cap) return (int)slots.size();
  ctx_->bind();
  for (auto &s : slots) // nothing is exported unless everything can be
    if (s.region->mapped[s.index] != Own) throw InvalidError("export of a slot that is not backed by a local page");
  int k = 0;
  try {
    for (auto &s : slots) {
      int fd = -1;
      if (vmm_uses_rocr()) {
        if (vmm_backend() == kVmmDrm) fd = DrmVm::instance().export_fd(s.region->handle[s.index]); // -1: a ROCr handle
        if (fd < 0) HSA_CHECK(hsa_amd_vmem_export_shareable_handle(&fd, as_hsa(s.region->handle[s.index]), 0));
      } else {
        HIP_CHECK(hipMemExportToShareableHandle(&fd, as_hip(s.region->handle[s.index]), hipMemHandleTypePosixFileDescriptor, 0));
      }
      out_fds[k++] = fd;
    }
  } catch (...) { // the caller never learns how many were written: close them here
    for (int i = 0; i < k; ++i) ::close(out_fds[i]);
    throw;
  }
  return k;
}

bool KvAllocator::map_imported_slots(const offset_t *offsets, size_t n, const int *fds, size_t n_fds) {
  std::lock_guard<std::mutex> g(mu_);
  if (!dev_.is_gpu) throw NoGpuError("map_imported_slots needs a GPU device");
  if (num_layers_ == 0) return false;
  auto slots = slots_for(offsets, n);
  if (slots.size() != n_fds) throw InvalidError("fd count does not match the slot count of the offsets");
  ctx_->bind();
  std::vector<phys_handle_t> hs(n_fds);
  size_t i = 0;
  try {
    for (; i < n_fds; ++i) hs[i] = import_posix_fd(fds[i]);
  } catch (...) {
    for (size_t j = 0; j < i; ++j) (void)vmm_try_release(hs[j]);
    throw;
  }
  // map_slots consumes the handles of the slots it backs (they are released again by its own rollback if the batch
  // fails); what it skips - a slot that is already mapped - or never reaches must not stay imported: every such
  // handle pins a page of the peer's pool for the life of this process.
  std::vector<uint8_t> consumed(n_fds, 0);
  try {
    map_slots(slots, &hs, &consumed);
  } catch (...) {
    for (size_t j = 0; j < n_fds; ++j)
      if (!consumed[j]) (void)vmm_try_release(hs[j]);
    throw;
  }
  for (size_t j = 0; j < n_fds; ++j)
    if (!consumed[j]) (void)vmm_try_release(hs[j]);
  return true;
}

} // namespace kvc
