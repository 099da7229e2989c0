// kv_allocator.hpp — VA regions + the batched map/unmap hot path.
//
// Counterpart of the reference's FTensor (csrc/ftensor.cpp), GPUPage/CPUPage (csrc/page.cpp)
// and FTensorAllocator (csrc/allocator.cpp), re-designed around what the MI355X driver
// charges for (hip_vmm.hpp): slots are tracked in flat vectors instead of one heap object
// + hash-map node per page, a whole map_to_kv_tensors() call is one batch (pooled handles,
// ranged hipMemSetAccess, one zero_fill_pages launch per <=256 pages overlapped with the
// remaining driver calls, a single stream sync at the end), and failures roll the batch back
// instead of aborting the process.
#pragma once

#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <unordered_map>
#include <vector>

#include "gpu_context.hpp"

namespace kvc {


// What backs a slot (KvRegion::mapped).
enum SlotState : uint8_t {
  Unbacked = 0, // nothing but the region's rest state
  Own,          // backed by its own page
  Imported,     // by an imported page
  UnmapQueued,  // released by the caller, physical unmap still queued (async unmap)
  Lane,         // backed by a page of a LANE (handle = the lane's: one per page id, shared by all its rows)
  PeerLane,     // by a page of a peer's lane (handle = the imported buffer's, shared by all rows of the page id)
};

// One contiguous VA reservation cut into fixed-size slots (the reference's FTensor).
struct KvRegion {
  std::string name;
  char *base = nullptr;
  size_t size = 0;
  size_t page_size = 0;
  bool on_gpu = false;
  bool backfilled = false;             // every unbacked slot currently aliases a zero page
  std::vector<phys_handle_t> zero;     // zero pages of this region; slot i aliases zero[i / fanout]
  size_t fanout = 1;
  phys_handle_t zero_of(size_t slot) const { return zero[slot / fanout]; }
  // drm backend ("zero extent"): unbacked slots alias the pages of ONE multi-page buffer of zeros that the GPU context
  // owns - slot i shows its page i % zx_pages - mapped through DRM a whole group of zx_pages slots per ioctl; a run of
  // slots goes alias -> pages and pages -> alias with one REPLACE each
  bool zx = false;
  phys_handle_t zx_handle = 0;
  size_t zx_pages = 0;
  // drm backend, the rest state of unbacked slots of a compat region (a lazy one only with KVCACHED_PRT=true): a PRT
  // mapping with no buffer (DrmVm::map_prt) - reads return 0, writes are dropped, nothing faults. The TLBs cache such
  // an entry once it has been looked at, so a map batch that replaces one invalidates before its pages are used (§4.2).
  // `backfilled` says whether an unmap invalidates inside the call (compat) or behind it (lazy).
  bool prt = false;
  bool rest_direct() const { return zx || prt; }                       // unbacked slots carry a DRM mapping of ours
  // a REPLACE back to the rest state must not cross a multiple of this: the zero extent's pages repeat with that period.
  // PRT: the reservation lays its mappings out in groups of kPrtGroupSlots (prt_all); a run that goes back to PRT later is
  // ONE mapping of up to kPrtRunSlots - one batch of run-sized extents (§4.8) - so that an unmap costs one REPLACE per run
  // and not one per group. What a later split leaves of such a mapping is rewritten by one PRT operation: 17 us after a
  // split of 1024 slots against 11 us after one of 64 (DrmVm::refresh_prt_remainders, profiles/r04_prt_run_probe.log).
  static constexpr size_t kPrtGroupSlots = 64, kPrtRunSlots = 1024;
  size_t rest_group() const { return zx ? zx_pages : (prt ? kPrtRunSlots : (size_t)-1); }
  std::vector<phys_handle_t> handle;   // per slot, valid when mapped[slot]
  std::vector<uint64_t> seq;           // per slot: creation order of that handle (release oldest first)
  std::vector<uint64_t> stale_epoch;   // per slot: the TLB invalidation (GpuContext::next_flush_epoch) that covers its last unmap
  // hybrid/drm backends: slots HIP has been told about (placeholder mapping made and removed again). Registration
  // happens in units of `reg_group` consecutive slots (64 MiB of VA per hipMemMap; the slots behind the last full
  // group one by one), and the placeholder handles are HIP handles of the unit's size, one per 4096 units so that
  // HIP's per-handle bookkeeping stays small.
  std::vector<uint8_t> registered;
  size_t reg_group = 1;
  std::vector<hipMemGenericAllocationHandle_t> shell, shell_group;
  bool in_full_group(size_t slot) const { return reg_group > 1 && slot / reg_group < num_slots() / reg_group; }
  std::vector<uint64_t> mark;          // one bit per slot, all clear at rest: scratch of RunScan (run_scan.hpp), under the allocator's lock
  std::vector<uint8_t> mapped;         // per slot: its SlotState
  size_t num_slots() const { return size / page_size; }
};

class KvAllocator {
public:
  // process-wide registry keyed by group id (reference: FTensorAllocator multiton, allocator.cpp:18-22,72-119)
  static void init(const std::string &dev_str, size_t page_size, bool contiguous_layout);
  static void shutdown();
  static KvAllocator *global(int64_t group_id);
  static bool initialized();
  static DeviceSpec device();
  static GpuContext *gpu(); // context of the init device (nullptr on "cpu")
  static size_t page_size();

  KvAllocator(DeviceSpec dev, bool contiguous_layout, GpuContext *ctx);
  ~KvAllocator();

  struct TensorDesc {
    void *ptr;
    size_t nbytes;
  };
  std::vector<TensorDesc> create_kv_tensors(size_t size, size_t dtype_size, const std::string &dev_str,
                                            int64_t num_layers, int64_t num_kv_buffers, bool unified_pool);
  bool kv_tensors_created();
  bool map_to_kv_tensors(const offset_t *offsets, size_t n);
  bool unmap_from_kv_tensors(const offset_t *offsets, size_t n);
  std::vector<void *> region_bases(); // layer-major, K then V (compact_blocks' region table)
  // Offload / restore: copy blocks `ids` of every region (region_bases() order) to / from the block-major image at `host`
  // (device address of pinned host memory). Under the lock, every slot a (block, region) byte range touches must be backed
  // (Own, Imported, Lane, PeerLane), else InvalidError and nothing is launched; the launch is issued under the lock too.
  // codec: 0 = the bytes themselves, else the KVC_CODEC_* number of the image's encoding (the caller has checked it).
  // slots (optional): block i goes to / comes from row slots[i] of the arena at `host` (the caller has checked the slots).
  void copy_blocks_host(bool to_host, const int64_t *ids, size_t n, size_t block_bytes, void *host, hipStream_t s, int codec = 0,
                        const int64_t *slots = nullptr);
  bool uses_prt();                    // unbacked slots of this group's regions are PRT mappings
  size_t lanes_per_extent();          // page ids are backed by lanes: lanes a buffer holds at most (0: per-slot pages)

  // async unmap (KVC_OPT_ASYNC_UNMAP): wait until every queued unmap of this allocator / of all allocators has
  // been carried out; bytes still queued (they count as free for this process)
  void flush_unmaps();
  static void flush_all_unmaps();
  // every allocator's lock, taken (true) / released (false) by the calling thread: no page-table update in between
  static void quiesce_all(bool on);
  static size_t pending_unmap_bytes();

  // TP shared pool
  int export_mapped_slots(const offset_t *offsets, size_t n, int *out_fds, int64_t cap);
  bool map_imported_slots(const offset_t *offsets, size_t n, const int *fds, size_t n_fds);
  // ... with page ids as units (lanes): one fd per page id + (lanes in the buffer, lane index) per page id
  int export_page_ids(const offset_t *offsets, size_t n, int *out_fds, int64_t *out_meta, int64_t cap);
  bool map_imported_page_ids(const offset_t *offsets, size_t n, const int *fds, size_t n_fds, const int64_t *meta);

private:
  struct Slot {
    KvRegion *region;
    size_t index;
  };
  std::vector<Slot> slots_for(const offset_t *offsets, size_t n);
  std::unique_ptr<KvRegion> make_region(const std::string &name, size_t size, size_t page_size);
  void destroy_region(KvRegion &r);
  void backfill_all(KvRegion &r);
  bool prt_all(KvRegion &r, bool by_default);      // PRT behind every slot of the region (false: not available / not wanted)
  int rest_replace(KvRegion &r, size_t first, size_t n); // slots [first, first+n) back to their rest state in one ioctl, whatever is mapped there
  int rest_map(KvRegion &r, size_t first, size_t n);     // the same over slots that hold nothing
  void register_slot(KvRegion &r, size_t slot);   // hybrid backend: make HIP aware of the slot's VA (once per slot)
  void unregister_slots(KvRegion &r);             // ... and take that back before the VA range is freed
  // `imported`: a peer's pages, one per slot, instead of pages from the pool; imported_consumed[i] is set for every
  // handle a slot took ownership of (the caller releases the others)
  void map_slots(const std::vector<Slot> &slots, const std::vector<phys_handle_t> *imported,
                 std::vector<uint8_t> *imported_consumed = nullptr);
  void unmap_slots(const std::vector<Slot> &slots);
  // the two halves of unmap_slots: driver unmaps under mu_ (handles collected), then invalidate + give handles back
  struct Unmapped {
    ExtentPool *pool = nullptr;  // where `own` goes back to
    size_t rows = 0;             // 0: `own` are single pages; else lanes of that many pages each (scrubbed row by row)
    std::vector<Phys> own;
    std::vector<phys_handle_t> imported; // released to the driver, behind the invalidation
    bool foreign = false;        // a peer's memory was among what was unmapped: no translation of it may survive the call
    bool any_backfilled = false;
    uint64_t epoch = 0; // the invalidation that covers these unmaps (GpuContext::next_flush_epoch after the driver calls)
    int64_t n = 0;
    size_t page_size = 0;
  };
  void unmap_collect(const std::vector<Slot> &slots, Unmapped &out);
  void unmap_finish(Unmapped &u, bool may_defer_shootdown);
  void reclaimer_loop();
  // ---- lanes (kv_lanes.cpp): page ids of a multi-row geometry backed, scrubbed and released as units
  struct Row {
    KvRegion *r;
    size_t first; // slot of page id p in this row = first + p
  };
  void setup_lanes();                                      // after the regions exist: decide, build the row table
  bool try_map_lanes(const offset_t *offsets, size_t n);   // false: nothing done, the generic path takes the call
  size_t unmap_lanes(const offset_t *offsets, size_t n, std::vector<offset_t> *others); // lanes unmapped; offsets that are not lane-backed -> others
  // the steps the lane paths share - own lanes and a peer's, map, unmap, export and import
  static constexpr size_t kNoPageId = (size_t)-1;
  size_t page_id_of(offset_t off) const;                   // the page id an offset names, or kNoPageId
  template <class F> void for_rows(size_t p, F &&f);       // f(region, slot of page id p) row by row: the per-row writes of a run
  struct RowsSplit {                                       // what back_rows leaves for settle_batch to rewrite and invalidate
    bool prt_dirty = false, replaced = false;
    void *zx_dirty = nullptr;
  };
  int back_rows(void *bo, uint64_t j0, uint64_t k, size_t p, size_t cnt, RowsSplit &split, size_t &rows_done);
  template <class Unmap> void undo_rows(size_t p, size_t cnt, size_t rows_done, bool settled, Unmap &&unmap);
  void cold_start_reserve(ExtentPool *pool);
  bool steal_pending(size_t page_size, Phys *out);
  size_t acquire_pages(ExtentPool *pool, size_t want, Phys *out, bool *stolen); // stolen == nullptr: may not steal_pending()
  struct MapBatch; // the state of one map_slots() batch (kv_map_paths.cpp)
  void lock_foreground(std::unique_lock<std::mutex> &lk); // mu_ with priority over the reclaimer

  DeviceSpec dev_;
  bool contiguous_;
  GpuContext *ctx_; // owned by the registry, outlives every allocator; nullptr on "cpu"
  bool unified_pool_ = false;
  bool exportable_ = false;
  int64_t num_layers_ = 0;
  int64_t num_kv_buffers_ = 2;
  size_t tensor_bytes_per_layer_ = 0;
  std::mutex mu_;
  std::vector<std::unique_ptr<KvRegion>> layers_; // per-layer regions, or ONE region in contiguous layout
  bool lanes_ = false;           // page ids are backed by lanes
  std::vector<Row> rows_;        // layer-major, K then V: the order slots_for() lists the slots of one offset in
  size_t ids_per_row_ = 0;       // page ids a row has room for
  ExtentPool *lane_pool_ = nullptr;
  std::unordered_map<phys_handle_t, uint32_t> peer_refs_; // imported buffers -> page ids of ours they back (released at 0)
  bool reserve_built_ = false;   // the cold-start instalments of the reserve are over (cold_start_reserve)
  // async unmap state (guarded by mu_)
  std::deque<Slot> pending_;
  std::condition_variable pending_cv_, drained_cv_;
  std::thread reclaimer_;
  bool reclaimer_stop_ = false, reclaimer_busy_ = false;
  std::atomic<int> foreground_waiting_{0};
};

// hipMemGetInfo of the init device, or the test override.
void mem_get_info(size_t *free_b, size_t *total_b);
void set_mem_info_override(size_t free_b, size_t total_b);
void device_synchronize();
int64_t import_count(bool direct); // shared pool: a peer's pages imported straight into KFD + DRM / through the runtime (ROCr, HIP)

} // namespace kvc
