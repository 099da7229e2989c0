// options.cpp — see options.hpp. The table, and the three functions that walk it.
#include "options.hpp"

namespace kvc {

Options &options() {
  static Options o;
  return o;
}

namespace {
using O = Options;
constexpr OptKind Bo = OptKind::Bool, In = OptKind::Int, Kw = OptKind::Keyword;
constexpr OptAccess RW = OptAccess::ReadWrite, RO = OptAccess::ReadOnly, ENV = OptAccess::EnvOnly;

// What each switch does: INTEGRATION.md §5 (one line each), include/kvcached_amd.h and DESIGN.md §4 (at length).
const OptionRow kRows[] = {
    // id, variable, kind, default, min, max, shift, member, access, word
    {KVC_OPT_ZERO_BACKFILL, "KVCACHED_ZERO_BACKFILL", Bo, 1, 0, 1, 0, &O::zero_backfill, RW, nullptr},
    {KVC_OPT_ZERO_FILL, "KVCACHED_ZERO_FILL", Bo, 1, 0, 1, 0, &O::zero_fill, RW, nullptr},
    {KVC_OPT_POOL_BYTES, "KVCACHED_PHYS_POOL_MB", In, 16384, kNoMin, kNoMax, 20, &O::pool_bytes, RW, nullptr}, // (set / get: bytes)
    {KVC_OPT_PROFILE, nullptr, In, 0, kNoMin, kNoMax, 0, &O::profile, RW, nullptr},
    {KVC_OPT_TLB_SHOOTDOWN, "KVCACHED_TLB_SHOOTDOWN", Bo, 1, 0, 1, 0, &O::tlb_shootdown, RW, nullptr},
    {KVC_OPT_DEFER_UNMAP_SHOOTDOWN, "KVCACHED_DEFER_UNMAP_SHOOTDOWN", Bo, 0, 0, 1, 0, &O::defer_unmap_shootdown, RW, nullptr},
    {KVC_OPT_ASYNC_UNMAP, "KVCACHED_ASYNC_UNMAP", Bo, 0, 0, 1, 0, &O::async_unmap, RW, nullptr},
    {KVC_OPT_UNMAP_INVALIDATION_US, "KVCACHED_UNMAP_INVALIDATION_US", In, 0, 0, kNoMax, 0, &O::deferred_unmap_flush_us, RW, nullptr},
    {KVC_OPT_FILL_VARIANT, nullptr, In, 0, kNoMin, kNoMax, 0, &O::fill_variant, RW, nullptr},
    {KVC_OPT_COMPACT_VARIANT, nullptr, In, 0, kNoMin, kNoMax, 0, &O::compact_variant, RW, nullptr},
    {KVC_OPT_ACCESS_RUN_SLOTS, "KVCACHED_ACCESS_RUN_SLOTS", In, 1, 1, kNoMax, 0, &O::access_run_slots, RW, nullptr},
    {KVC_OPT_ZERO_ALIAS_FANOUT, "KVCACHED_ZERO_ALIAS_FANOUT", In, 256, 1, kNoMax, 0, &O::zero_alias_fanout, RW, nullptr},
    {KVC_OPT_FILL_CHUNK_SLOTS, "KVCACHED_FILL_CHUNK_SLOTS", In, 1024, 1, kNoMax, 0, &O::fill_chunk_slots, RW, nullptr},
    {KVC_OPT_POOL_IDLE_MS, "KVCACHED_POOL_IDLE_MS", In, 1000, 0, kNoMax, 0, &O::pool_idle_ms, RW, nullptr},
    {KVC_OPT_ASYNC_SHOOTDOWN, "KVCACHED_ASYNC_SHOOTDOWN", Bo, 1, 0, 1, 0, &O::async_shootdown, RW, nullptr},
    {KVC_OPT_MAX_EXTENT_PAGES, "KVCACHED_PHYS_CHUNK_PAGES", In, kMaxChunkPages, 1, kMaxChunkPages, 0, &O::phys_chunk_pages, RO, nullptr},
    {0, "KVCACHED_HIP_REG_GROUP_MB", In, 64, 0, kNoMax, 0, &O::hip_reg_group_mb, ENV, nullptr}, // (stored in MB)
    {0, "KVCACHED_DRM_CLEAR_RUN", In, 16, 0, kNoMax, 0, &O::clear_run_slots, ENV, nullptr},
    {0, "KVCACHED_EXTENT_WASTE_PCT", In, 5, 0, 100, 0, &O::extent_waste_pct, ENV, nullptr},
    {0, "KVCACHED_PHYS_RESERVE_MB", In, 2048, 0, kNoMax, 20, &O::phys_reserve_bytes, ENV, nullptr},
    {0, "KVCACHED_SCRUB_ON_RELEASE", Bo, 1, 0, 1, 0, &O::scrub_on_release, ENV, nullptr},
    {0, "KVCACHED_MAP_WAITS_FOR_ALL_FLUSHES", Bo, 0, 0, 1, 0, &O::map_waits_for_all_flushes, ENV, nullptr},
    {0, "KVCACHED_MAP_SHOOTDOWN", Kw, 0, 0, 1, 0, &O::map_shootdown_always, ENV, "always"},
    // read where they are used, at the moment they are used
    {0, "KVCACHED_VMM_BACKEND", Kw, 0, 0, 0, 0, nullptr, ENV, "drm"}, // KvAllocator::init: validated there, with its fallback chain
    {0, "KVCACHED_LOG_LEVEL", Kw, 0, 0, 0, 0, nullptr, ENV, "WARNING"}, // common.hpp: log_threshold(), once per process
    {0, "KVCACHED_IPC_NAME", Kw, 0, 0, 0, 0, nullptr, ENV, "kvcached_engine_<pgid>"}, // mem_info.hpp
    {0, "KVCACHED_GPU_UTILIZATION", Kw, 0, 0, 0, 0, nullptr, ENV, "0.95"}, // env_gpu_utilization(): a fraction, once per process
    {0, "KVCACHED_MIN_RESERVED_PAGES", In, 5, kNoMin, kNoMax, 0, nullptr, ENV, nullptr}, // page_allocator.cpp, once per process
    {0, "KVCACHED_MAX_RESERVED_PAGES", In, 10, kNoMin, kNoMax, 0, nullptr, ENV, nullptr},
    {0, "KVCACHED_LANE_EXTENTS", Bo, 1, 0, 1, 0, nullptr, ENV, nullptr},
    {0, "KVCACHED_LANE_EXTENT_MB", In, 1024, 1, kNoMax, 20, nullptr, ENV, nullptr},
    {0, "KVCACHED_LANES_PER_BUFFER", In, 8, 1, kMaxLanesPerBuffer, 0, nullptr, ENV, nullptr},
    {0, "KVCACHED_RESERVE_IDLE_S", In, 10, 1, kNoMax, 0, nullptr, ENV, nullptr},
    {0, "KVCACHED_PHYS_RESERVE_MAX_MB", In, 16384, 0, kNoMax, 20, nullptr, ENV, nullptr},
    {0, "KVCACHED_ADAPTIVE_RESERVE", Bo, 1, 0, 1, 0, nullptr, ENV, nullptr},
    {0, "KVCACHED_KFD_TLB_FLUSH", Bo, 1, 0, 1, 0, nullptr, ENV, nullptr},
    {0, "KVCACHED_DRM_KFD_IMPORT", Bo, 1, 0, 1, 0, nullptr, ENV, nullptr},
    {0, "KVCACHED_DRM_KFD_CREATE", Bo, 1, 0, 1, 0, nullptr, ENV, nullptr},
    {0, "KVCACHED_EXPORTABLE_HANDLES", Bo, 0, 0, 1, 0, nullptr, ENV, nullptr},
    {0, "KVCACHED_STRICT_ABORT", Bo, 0, 0, 1, 0, nullptr, ENV, nullptr},
    {0, "KVCACHED_PRT", Bo, kByMode, 0, 1, 0, nullptr, ENV, nullptr}, // compat: true, lazy: false
    {0, "KVCACHED_ZERO_EXTENT", Bo, 1, 0, 1, 0, nullptr, ENV, nullptr},
};

const OptionRow *row_of(int id) {
  for (const OptionRow &r : kRows)
    if (r.id == id) return &r;
  return nullptr;
}
const OptionRow &row_of(const char *env) {
  for (const OptionRow &r : kRows)
    if (r.env && !std::strcmp(r.env, env)) return r;
  throw InvalidError(std::string(env) + " has no row in the option table");
}

int64_t clamped(const OptionRow &r, int64_t v) { return v < r.min ? r.min : v > r.max ? r.max : v; }

// The variable's value by its row, in stored units; where it is unset or empty, the row's default (`dflt` for kByMode).
int64_t parse(const OptionRow &r, int64_t dflt) {
  switch (r.kind) {
  case OptKind::Bool: return env_bool(r.env, dflt != 0) ? 1 : 0;
  case OptKind::Keyword: {
    const char *e = std::getenv(r.env);
    return e && !std::strcmp(e, r.text) ? 1 : 0;
  }
  case OptKind::Int: break;
  }
  return clamped(r, env_i64(r.env, dflt)) * (int64_t(1) << r.shift);
}
} // namespace

const OptionRow *option_rows(size_t *count) {
  *count = sizeof kRows / sizeof kRows[0];
  return kRows;
}

void load_options_from_env() {
  for (const OptionRow &r : kRows)
    if (r.env && r.member) options().*r.member = parse(r, r.dflt);
}

bool set_stored_option(int id, int64_t value) {
  const OptionRow *r = id ? row_of(id) : nullptr;
  if (!r || r->access != OptAccess::ReadWrite) return false;
  // (Bool rows store what they are given, as they always have; the bounded rows have no shift)
  options().*r->member = r->kind == OptKind::Int ? clamped(*r, value) : value;
  return true;
}

bool get_stored_option(int id, int64_t *value) {
  const OptionRow *r = id ? row_of(id) : nullptr;
  if (!r || r->access == OptAccess::EnvOnly) return false;
  *value = options().*r->member;
  return true;
}

int64_t env_option(const char *env) {
  const OptionRow &r = row_of(env);
  return parse(r, r.dflt);
}
bool env_flag(const char *env, bool by_mode) { return parse(row_of(env), by_mode) != 0; }
const char *env_word(const char *env) {
  const char *e = std::getenv(env);
  return e ? e : row_of(env).text;
}
double env_gpu_utilization() {
  static const double v = std::atof(env_word("KVCACHED_GPU_UTILIZATION"));
  return v;
}

} // namespace kvc
