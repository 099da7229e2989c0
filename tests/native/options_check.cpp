// options_check.cpp — the option table (kvcached_amd/csrc/options.cpp) on the CPU, compiled with g++ -fsanitize=address,undefined
// against options.cpp alone (tests/test_options.py). The rows that kvc_get_option cannot reach are loaded from the environment
// here and held to the figures written out below; `--dump` prints one "NAME default min max" line per variable.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../kvcached_amd/csrc/options.hpp"

using namespace kvc;

static int failures = 0;
#define REQUIRE(cond)                                                     \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: REQUIRE(%s)\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

// `text` == nullptr: the variable is unset
static int64_t loaded(const char *env, const char *text, std::atomic<int64_t> Options::*member) {
  if (text) setenv(env, text, 1);
  else unsetenv(env);
  load_options_from_env();
  unsetenv(env);
  return options().*member;
}

static void int_row(const char *env, std::atomic<int64_t> Options::*m, int64_t dflt, int64_t min, const int64_t *max, int shift) {
  const int64_t unit = int64_t(1) << shift;
  REQUIRE(loaded(env, nullptr, m) == dflt * unit);
  REQUIRE(loaded(env, "", m) == dflt * unit);
  REQUIRE(loaded(env, std::to_string(min + 3).c_str(), m) == (min + 3) * unit);
  REQUIRE(loaded(env, std::to_string(min - 1).c_str(), m) == min * unit);
  if (max) REQUIRE(loaded(env, std::to_string(*max + 1).c_str(), m) == *max * unit);
  REQUIRE(loaded(env, "banana", m) == min * unit); // (atoll: 0, which none of these rows has below its minimum)
}

static void bool_row(const char *env, std::atomic<int64_t> Options::*m, bool dflt) {
  REQUIRE(loaded(env, nullptr, m) == dflt);
  REQUIRE(loaded(env, "", m) == dflt);
  for (const char *on : {"1", "true", "yes", "on", "TRUE"}) REQUIRE(loaded(env, on, m) == 1);
  for (const char *off : {"0", "false", "off", "banana"}) REQUIRE(loaded(env, off, m) == 0);
}

static int dump() {
  size_t n = 0;
  const OptionRow *rows = option_rows(&n);
  auto bound = [](int64_t v) { return v == kNoMin || v == kNoMax ? std::string("-") : std::to_string(v); };
  for (size_t i = 0; i < n; ++i) {
    const OptionRow &r = rows[i];
    if (!r.env) continue;
    std::string dflt = std::to_string(r.dflt), lo = "-", hi = "-";
    if (r.kind == OptKind::Bool) dflt = r.dflt == kByMode ? "mode" : r.dflt ? "true" : "false";
    if (r.kind == OptKind::Keyword) dflt = r.member ? "off" : r.text;
    if (r.kind == OptKind::Int) lo = bound(r.min), hi = bound(r.max);
    std::printf("%s %s %s %s\n", r.env, dflt.c_str(), lo.c_str(), hi.c_str());
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && std::string(argv[1]) == "--dump") return dump();
  size_t n = 0;
  const OptionRow *rows = option_rows(&n);
  for (size_t i = 0; i < n; ++i) // the caller's environment is not part of the check
    if (rows[i].env) unsetenv(rows[i].env);

  const int64_t hundred = 100;
  int_row("KVCACHED_HIP_REG_GROUP_MB", &Options::hip_reg_group_mb, 64, 0, nullptr, 0); // (stored in MB)
  int_row("KVCACHED_DRM_CLEAR_RUN", &Options::clear_run_slots, 16, 0, nullptr, 0);
  int_row("KVCACHED_EXTENT_WASTE_PCT", &Options::extent_waste_pct, 5, 0, &hundred, 0);
  int_row("KVCACHED_PHYS_RESERVE_MB", &Options::phys_reserve_bytes, 2048, 0, nullptr, 20);
  bool_row("KVCACHED_SCRUB_ON_RELEASE", &Options::scrub_on_release, true);
  bool_row("KVCACHED_MAP_WAITS_FOR_ALL_FLUSHES", &Options::map_waits_for_all_flushes, false);
  const char *ms = "KVCACHED_MAP_SHOOTDOWN";
  REQUIRE(loaded(ms, nullptr, &Options::map_shootdown_always) == 0);
  REQUIRE(loaded(ms, "always", &Options::map_shootdown_always) == 1);
  for (const char *other : {"", "ALWAYS", "1", "true", "never"}) REQUIRE(loaded(ms, other, &Options::map_shootdown_always) == 0);

  // what a process sees before its first init is what an init with nothing set loads
  load_options_from_env();
  Options fresh;
  for (size_t i = 0; i < n; ++i)
    if (rows[i].member) REQUIRE((fresh.*rows[i].member).load() == (options().*rows[i].member).load());

  // the switches read in place go through the same rows
  REQUIRE(env_option("KVCACHED_LANE_EXTENT_MB") == 1024ll << 20 && env_option("KVCACHED_LANES_PER_BUFFER") == 8);
  setenv("KVCACHED_LANES_PER_BUFFER", "1000", 1);
  setenv("KVCACHED_LANE_EXTENT_MB", "0", 1);
  REQUIRE(env_option("KVCACHED_LANES_PER_BUFFER") == 64 && env_option("KVCACHED_LANE_EXTENT_MB") == 1ll << 20);
  REQUIRE(env_flag("KVCACHED_PRT", true) && !env_flag("KVCACHED_PRT", false));
  setenv("KVCACHED_PRT", "false", 1);
  REQUIRE(!env_flag("KVCACHED_PRT", true));
  REQUIRE(std::string(env_word("KVCACHED_VMM_BACKEND")) == "drm");
  setenv("KVCACHED_VMM_BACKEND", "", 1); // (set and empty is not unset: init refuses it)
  REQUIRE(std::string(env_word("KVCACHED_VMM_BACKEND")).empty());
  REQUIRE(env_gpu_utilization() == 0.95);

  // numbers: a row answers set / get by its access, the bounded ones clamp
  int64_t v = 0;
  REQUIRE(set_stored_option(KVC_OPT_POOL_IDLE_MS, -5) && get_stored_option(KVC_OPT_POOL_IDLE_MS, &v) && v == 0);
  REQUIRE(!set_stored_option(KVC_OPT_MAX_EXTENT_PAGES, 7) && get_stored_option(KVC_OPT_MAX_EXTENT_PAGES, &v) && v == 1024);
  REQUIRE(!set_stored_option(0, 1) && !get_stored_option(0, &v) && !set_stored_option(999, 1) && !get_stored_option(999, &v));

  if (failures) return 1;
  std::puts("ok");
  return 0;
}
