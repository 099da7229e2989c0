// options.hpp — every switch of the library in one table (options.cpp): option number, KVCACHED_* variable, kind, default
// and bounds, one row each. Free of HIP: common.hpp and the public header only (tests/native/options_check.cpp compiles it
// with g++ alone). Hot paths read options().x; nothing on a map / unmap path looks a row up.
#pragma once

#include <atomic>
#include <limits>

#include "../../include/kvcached_amd.h"
#include "common.hpp"

namespace kvc {

constexpr int64_t kMaxChunkPages = 1024; // KVCACHED_PHYS_CHUNK_PAGES at most (= kMaxExtentPages, extent_pool.hpp)
constexpr unsigned kMaxLanesPerBuffer = 64; // KVCACHED_LANES_PER_BUFFER at most (a lane buffer is rows x lanes pages)

// The stored options. The initialisers are the table's defaults (options_check.cpp holds them to it).
struct Options {
  std::atomic<int64_t> zero_backfill{1};
  std::atomic<int64_t> zero_fill{1};
  std::atomic<int64_t> pool_bytes{16384ll << 20};
  std::atomic<int64_t> profile{0};
  std::atomic<int64_t> tlb_shootdown{1};
  std::atomic<int64_t> pool_idle_ms{1000};       // idle handles older than this are released (0 = keep until pressure)
  std::atomic<int64_t> async_unmap{0};           // unmap_from_kv_tensors only queues; a reclaimer thread does the driver calls
  std::atomic<int64_t> async_shootdown{1};       // with a housekeeping thread around, unmap leaves its TLB invalidation to it
  std::atomic<int64_t> hip_reg_group_mb{64};     // hybrid/drm: VA introduced to HIP per hipMemMap (0 = slot by slot)
  std::atomic<int64_t> clear_run_slots{16};      // drm backend: unmap runs of adjacent slots with one CLEAR ioctl (0 = off)
  std::atomic<int64_t> phys_chunk_pages{kMaxChunkPages}; // drm backend: a run of adjacent slots is backed by ONE buffer of up to this many pages (1 = off)
  std::atomic<int64_t> extent_waste_pct{5};      // ... and new extents shrink while free pieces of partly used ones exceed this share of the pages in use
  std::atomic<int64_t> phys_reserve_bytes{2048ll << 20}; // idle physical memory the housekeeping thread keeps ready (pre-created, never below it)
  std::atomic<int64_t> map_waits_for_all_flushes{0}; // 1 = a map batch waits for every invalidation owed, not only those of its own slots
  std::atomic<int64_t> scrub_on_release{1};      // drm backend: pages are zeroed (through an alias mapping) when they come back, not when they go out
  std::atomic<int64_t> map_shootdown_always{0};  // 1 = invalidate after every map batch even when no stale translation can exist
  std::atomic<int64_t> defer_unmap_shootdown{0}; // unmap's invalidation may wait for the next map batch / driver release
  // compat regions: the invalidation an unmap owes may trail the call by at most `deferred_unmap_flush_us` (0 = inside the call,
  // the default): the pages wait un-scrubbed and un-offered until it has happened, and the next map batch's own invalidation
  // absorbs it if it comes first (KVCACHED_UNMAP_INVALIDATION_US)
  std::atomic<int64_t> deferred_unmap_flush_us{0};
  std::atomic<int64_t> access_run_slots{1}; // max mappings one hipMemSetAccess call may span
  std::atomic<int64_t> zero_alias_fanout{256}; // unbacked slots that share one physical zero page
  std::atomic<int64_t> fill_chunk_slots{1024}; // slots made usable (one TLB shootdown + fill launches) at a time
  std::atomic<int64_t> fill_variant{0};
  std::atomic<int64_t> compact_variant{0};
};
Options &options(); // one object per process: defined in options.cpp, which goes into libkvcached_amd.so only

enum class OptKind { Bool, Int, Keyword };
enum class OptAccess { ReadWrite, ReadOnly, EnvOnly }; // through kvc_set_option / kvc_get_option
constexpr int64_t kNoMin = std::numeric_limits<int64_t>::min(), kNoMax = std::numeric_limits<int64_t>::max();
constexpr int64_t kByMode = -1; // a Bool row whose default depends on the caller's mode (env_flag's second argument)

struct OptionRow {
  int id;          // kvc_set_option / kvc_get_option number (0 = none)
  const char *env; // KVCACHED_* variable (nullptr = none)
  OptKind kind;
  int64_t dflt, min, max; // in the variable's units
  int shift;              // stored value = variable's value << shift (the _MB switches are stored in bytes)
  std::atomic<int64_t> Options::*member; // where load_options_from_env() stores it (nullptr: read where it is used)
  OptAccess access;
  const char *text; // Keyword rows: the default word; with a member, the word that stores 1 (anything else stores 0)
};
const OptionRow *option_rows(size_t *count);

void load_options_from_env();                       // every row with a variable and a member: parse, clamp, store
bool set_stored_option(int id, int64_t value);      // ReadWrite rows: clamps by the row; false: no such row
bool get_stored_option(int id, int64_t *value);     // ReadWrite and ReadOnly rows
// The switches that are read where (and when) they are used, parsed by their row: default and bounds stand there.
int64_t env_option(const char *env);                // Int (clamped, shifted) and Bool rows
bool env_flag(const char *env, bool by_mode);       // a Bool row with kByMode: the caller's default where the variable is unset
const char *env_word(const char *env);              // Keyword rows: the variable's text, the row's where it is unset
double env_gpu_utilization();                       // KVCACHED_GPU_UTILIZATION, read once per process

// Host-time segments of the map / unmap calls: Stats::seg is indexed by these, option KVC_OPT_HOST_SEGMENT_0 + i reads them.
#define KVC_SEG(name) (KVC_OPT_SEG_##name - KVC_OPT_HOST_SEGMENT_0)
enum Seg : int {
  kSegMapOffsets = KVC_SEG(MAP_OFFSETS), kSegMapClassify = KVC_SEG(MAP_CLASSIFY), kSegMapRuns = KVC_SEG(MAP_RUNS),
  kSegMapPool = KVC_SEG(MAP_POOL), kSegMapIoctls = KVC_SEG(MAP_IOCTLS), kSegMapBookkeeping = KVC_SEG(MAP_BOOKKEEPING),
  kSegMapInvalidation = KVC_SEG(MAP_INVALIDATION), kSegMapWaitFill = KVC_SEG(MAP_WAIT_FILL),
  kSegMapWaitScrub = KVC_SEG(MAP_WAIT_SCRUB), kSegMapScrubsBehind = KVC_SEG(MAP_SCRUBS_BEHIND),
  kSegUnmapOffsets = KVC_SEG(UNMAP_OFFSETS), kSegUnmapRuns = KVC_SEG(UNMAP_RUNS), kSegUnmapIoctls = KVC_SEG(UNMAP_IOCTLS),
  kSegUnmapBookkeeping = KVC_SEG(UNMAP_BOOKKEEPING), kSegUnmapRemainders = KVC_SEG(UNMAP_REMAINDERS),
  kSegUnmapEpochs = KVC_SEG(UNMAP_EPOCHS), kSegUnmapInvalidation = KVC_SEG(UNMAP_INVALIDATION),
  kSegUnmapScrubLaunch = KVC_SEG(UNMAP_SCRUB_LAUNCH), kSegUnmapPool = KVC_SEG(UNMAP_POOL),
  kSegKfdRemapHalf = KVC_SEG(KFD_REMAP_HALF), kSegMapRemainderRewrite = KVC_SEG(MAP_REMAINDER_REWRITE),
  kSegMapIoctlCount = KVC_SEG(MAP_IOCTL_COUNT), kSegUnmapIoctlCount = KVC_SEG(UNMAP_IOCTL_COUNT),
  kSegMapRunCount = KVC_SEG(MAP_RUN_COUNT),
  kSegCount = KVC_SEG(END),
};
#undef KVC_SEG

} // namespace kvc
