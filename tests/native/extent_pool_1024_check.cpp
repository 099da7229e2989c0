// extent_pool_1024_check.cpp — extent_pool.hpp at extents of up to one bench batch (kMaxExtentPages = 1024 pages), on the
// CPU: the invariants of the bench shape, the handle tag round trip, foreign handles, and the footprint of request-shaped
// churn and of its adversary (tides) at 1024 against 64. Built and run by tests/test_extent_pool_1024.py (g++, ASan +
// UBSan, no HIP). Prints one JSON object; exits non-zero on a broken invariant.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../../kvcached_amd/csrc/extent_pool.hpp"

using namespace kvc;

#define REQUIRE(cond, ...)                                                                                             \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);                                                 \
      fprintf(stderr, __VA_ARGS__);                                                                                    \
      fprintf(stderr, "\n");                                                                                           \
      exit(1);                                                                                                         \
    }                                                                                                                  \
  } while (0)

struct FakeDriver {
  std::map<phys_handle_t, unsigned> live; // extent -> pages
  uint64_t next = 0x1000;       // (set gpu_id bits to exercise the packed encoding)
  uint64_t high_bits = 0; // single-page pools: handles like ROCr's, with bits above 48 set
  size_t creates = 0, releases = 0, before_release_calls = 0, fail_after = (size_t)-1;
  bool pressure = false, give_tags = false;
  size_t prepared = 0;
  ExtentPool *pool = nullptr;
  bool check_no_waste_at_create = true;
  ExtentDriver make() {
    ExtentDriver d;
    d.prepare_release = [this](phys_handle_t h, uint64_t tag, size_t pages) {
      REQUIRE(live.count(h) && live[h] == pages && tag == (give_tags ? 0x7000000000ull + (h & 0xffffffffull) * 0x100000 : 0), "prepare_release of the right extent");
      ++prepared;
    };
    d.create = [this](size_t pages, uint64_t *tag) -> phys_handle_t {
      if (creates >= fail_after) throw std::runtime_error("out of memory [injected]");
      if (pool && check_no_waste_at_create) {
        auto f = pool->footprint();
        REQUIRE(f.free_pieces == 0 && f.idle_pages == 0, "created %zu pages while %zu free pieces and %zu idle pages existed",
                pages, f.free_pieces, f.idle_pages);
      }
      ++creates;
      const phys_handle_t h = next | high_bits;
      next += 0x10;
      live[h] = (unsigned)pages;
      if (tag) *tag = give_tags ? 0x7000000000ull + (h & 0xffffffffull) * 0x100000 : 0;
      return h;
    };
    d.release = [this](phys_handle_t h) {
      auto it = live.find(h);
      REQUIRE(it != live.end(), "release of an unknown extent %llx", (unsigned long long)h);
      live.erase(it);
      ++releases;
      return true;
    };
    d.before_release = [this] { ++before_release_calls; };
    d.under_pressure = [this] { return pressure; };
    return d;
  }
  size_t live_pages() const {
    size_t n = 0;
    for (auto &kv : live) n += kv.second;
    return n;
  }
};

// what the allocator does with the pool: back a sorted set of slots run by run, give pages back
struct Harness {
  FakeDriver drv;
  VmmCounters ctr;
  ExtentPool pool;
  std::map<int64_t, Phys> slot;             // slot -> piece
  std::set<phys_handle_t> out;              // pieces handed out
  size_t map_ioctls = 0, pages_mapped = 0;
  Harness(unsigned kmax, size_t cap_pages, double waste) : pool(2u << 20, kmax, drv.make(), &ctr) {
    drv.pool = &pool;
    pool.set_cap_bytes(cap_pages * (2u << 20));
    pool.set_waste_frac(waste);
  }
  void map(std::vector<int64_t> ids) {
    std::sort(ids.begin(), ids.end());
    std::vector<Phys> got(kMaxExtentPages);
    for (size_t i = 0; i < ids.size();) {
      size_t j = i + 1;
      while (j < ids.size() && ids[j] == ids[j - 1] + 1) ++j;
      while (i < j) {
        bool rec = false;
        size_t n = pool.acquire_run(j - i, got.data(), &rec, false);
        if (n == 0) n = pool.acquire_run(j - i, got.data(), &rec, true);
        REQUIRE(n >= 1 && n <= j - i, "acquire_run(%zu) returned %zu", j - i, n);
        // (only a pool that makes multi-page extents encodes anything into its handles)
        const bool multi = pool.multi_page();
        auto ext_of = [&](phys_handle_t h) { return multi ? chunk_of(h) : h; };
        auto idx_of = [&](phys_handle_t h) { return multi ? piece_of(h) : 0u; };
        const phys_handle_t ext = ext_of(got[0].h);
        for (size_t k = 0; k < n; ++k) {
          REQUIRE(ext_of(got[k].h) == ext, "a run spans two extents");
          REQUIRE(idx_of(got[k].h) == idx_of(got[0].h) + k, "pieces of a run are not consecutive");
          REQUIRE(drv.live.count(ext), "piece of an extent the driver does not know");
          REQUIRE((multi ? pages_of(got[k].h) : 1u) == drv.live[ext] && idx_of(got[k].h) < drv.live[ext], "piece index / size encoding");
          REQUIRE(out.insert(got[k].h).second, "piece %llx handed out twice", (unsigned long long)got[k].h);
          REQUIRE(!slot.count(ids[i + k]), "slot mapped twice by the harness");
          slot[ids[i + k]] = got[k];
        }
        ++map_ioctls;
        pages_mapped += n;
        i += n;
      }
    }
    check();
  }
  void unmap(const std::vector<int64_t> &ids) {
    std::vector<Phys> back;
    for (auto id : ids) {
      auto it = slot.find(id);
      REQUIRE(it != slot.end(), "unmap of an unmapped slot");
      back.push_back(it->second);
      out.erase(it->second.h);
      slot.erase(it);
    }
    pool.release_batch(back.data(), back.size());
    check();
  }
  void check() {
    auto f = pool.footprint();
    REQUIRE(f.out_pages == out.size(), "out %zu != %zu", f.out_pages, out.size());
    REQUIRE(f.held_pages == drv.live_pages(), "held %zu != driver's %zu", f.held_pages, drv.live_pages());
    REQUIRE(f.held_pages == f.out_pages + f.idle_pages + f.free_pieces, "held %zu != out %zu + idle %zu + free pieces %zu",
            f.held_pages, f.out_pages, f.idle_pages, f.free_pieces);
    REQUIRE(f.bad_releases == 0, "bad releases");
    REQUIRE((size_t)(ctr.created - ctr.released) == f.held_pages, "counters: created - released != held");
  }
};

static double pct(std::vector<double> v, double q) {
  if (v.empty()) return 0;
  std::sort(v.begin(), v.end());
  return v[std::min(v.size() - 1, (size_t)(v.size() * q))];
}

struct Churn {
  double p50, p90, max;
};

static Churn churn(std::mt19937_64 &rng, unsigned kmax, double straggle, bool sorted_free) {
  Harness h(kmax, 0, 0.05); // pool off: only fragmentation is left
  std::vector<int64_t> free_ids;
  for (int64_t i = 0; i < 4096; ++i) free_ids.push_back(i);
  std::vector<std::vector<int64_t>> reqs;
  std::vector<double> ratio;
  for (int op = 0; op < 30000; ++op) {
    const bool grow = reqs.empty() || (h.slot.size() < 3000 && rng() % 100 < 52);
    if (grow) {
      size_t n = rng() % 5 == 0 ? 1 + rng() % 40 : 1 + rng() % 6;
      n = std::min(n, free_ids.size());
      if (!n) continue;
      if (sorted_free) std::sort(free_ids.begin(), free_ids.end());
      std::vector<int64_t> ids(free_ids.begin(), free_ids.begin() + n);
      free_ids.erase(free_ids.begin(), free_ids.begin() + n);
      h.map(ids);
      std::vector<int64_t> main, late;
      for (auto id : ids) ((double)(rng() % 1000) / 1000.0 < straggle ? late : main).push_back(id);
      if (!main.empty()) reqs.push_back(main);
      if (!late.empty()) reqs.push_back(late);
    } else {
      const size_t k = rng() % reqs.size();
      h.unmap(reqs[k]);
      for (auto id : reqs[k]) free_ids.push_back(id);
      reqs[k] = reqs.back();
      reqs.pop_back();
    }
    auto f = h.pool.footprint();
    if (f.out_pages >= 256) ratio.push_back((double)f.held_pages / f.out_pages);
  }
  for (auto &r : reqs) h.unmap(r);
  REQUIRE(h.drv.live.empty(), "pool off: everything went back");
  return Churn{pct(ratio, 0.5), pct(ratio, 0.9), pct(ratio, 1.0)};
}

// bench-shaped batches of 256-1024 adjacent slots, mapped by one call each, with `straggle` of their pages freed on their
// own later (a request that keeps a few pages): the case in which one straggler can pin a whole 2 GiB extent
static Churn batches(std::mt19937_64 &rng, unsigned kmax, double straggle) {
  Harness h(kmax, 0, 0.05); // pool off: only fragmentation is left
  std::vector<int64_t> free_ids;
  for (int64_t i = 0; i < 16384; ++i) free_ids.push_back(i);
  std::vector<std::vector<int64_t>> reqs;
  std::vector<double> ratio;
  for (int op = 0; op < 3000; ++op) {
    const bool grow = reqs.empty() || (h.slot.size() < 10000 && rng() % 100 < 52);
    if (grow) {
      std::sort(free_ids.begin(), free_ids.end()); // runs wherever the free list has them
      const size_t n = std::min<size_t>(256 + rng() % 769, free_ids.size());
      if (!n) continue;
      std::vector<int64_t> ids(free_ids.begin(), free_ids.begin() + n);
      free_ids.erase(free_ids.begin(), free_ids.begin() + n);
      h.map(ids);
      std::vector<int64_t> main, late;
      for (auto id : ids) ((double)(rng() % 1000) / 1000.0 < straggle ? late : main).push_back(id);
      if (!main.empty()) reqs.push_back(main);
      for (auto id : late) reqs.push_back({id}); // every straggler on its own
    } else {
      const size_t k = rng() % reqs.size();
      h.unmap(reqs[k]);
      for (auto id : reqs[k]) free_ids.push_back(id);
      reqs[k] = reqs.back();
      reqs.pop_back();
    }
    auto f = h.pool.footprint();
    if (f.out_pages >= 256) ratio.push_back((double)f.held_pages / f.out_pages);
  }
  for (auto &r : reqs) h.unmap(r);
  REQUIRE(h.drv.live.empty(), "pool off: everything went back");
  return Churn{pct(ratio, 0.5), pct(ratio, 0.9), pct(ratio, 1.0)};
}

// memory grows in runs (here: runs as long as an extent may be) and ebbs page by page at random
static Churn tides(std::mt19937_64 &rng, unsigned kmax, size_t run) {
  Harness h(kmax, 0, 0.05);
  std::vector<double> ratio;
  std::vector<int64_t> mapped;
  int64_t next_id = 0;
  for (int tide = 0; tide < 6; ++tide) {
    while (mapped.size() < 1500u * (tide + 1)) {
      std::vector<int64_t> ids;
      for (size_t i = 0; i < run; ++i) ids.push_back(next_id++);
      h.map(ids);
      mapped.insert(mapped.end(), ids.begin(), ids.end());
      auto f = h.pool.footprint();
      if (f.out_pages >= 256) ratio.push_back((double)f.held_pages / f.out_pages);
    }
    std::shuffle(mapped.begin(), mapped.end(), rng);
    while (mapped.size() > 150u * (tide + 1)) {
      std::vector<int64_t> ids(mapped.end() - 20, mapped.end());
      mapped.resize(mapped.size() - 20);
      h.unmap(ids);
      auto f = h.pool.footprint();
      if (f.out_pages >= 256) ratio.push_back((double)f.held_pages / f.out_pages);
    }
  }
  h.unmap(mapped);
  REQUIRE(h.drv.live.empty(), "everything went back");
  return Churn{pct(ratio, 0.5), pct(ratio, 0.9), pct(ratio, 1.0)};
}

static std::string fmt(const char *name, const Churn &c) {
  char buf[256];
  snprintf(buf, sizeof buf, "\"%s\": {\"held_over_mapped_p50\": %.3f, \"p90\": %.3f, \"max\": %.3f}", name, c.p50, c.p90, c.max);
  return buf;
}

int main() {
  std::string js = "{";
  // 1. the tag: every (size, index) up to 1024 x 1024 over KFD-shaped handles round-trips; what is not a piece passes through
  {
    const uint64_t handles[] = {0x1000, (0xffffull << 32) | kIdrMask, (0x1234ull << 32) | 7, (0x8000ull << 32)};
    size_t checked = 0;
    for (uint64_t h : handles) {
      REQUIRE(can_tag(h), "KFD-shaped handle %llx packs", (unsigned long long)h);
      for (unsigned pages = 2; pages <= kMaxExtentPages; ++pages)
        for (unsigned piece = 0; piece < pages; ++piece) {
          const phys_handle_t id = piece_id(h, piece, pages);
          REQUIRE(is_piece(id) && chunk_of(id) == h && piece_of(id) == piece && pages_of(id) == pages,
                  "round trip of (%llx, %u of %u)", (unsigned long long)h, piece, pages);
          ++checked;
        }
      REQUIRE(piece_id(h, 0, 1) == h, "a one-page extent is its own handle");
    }
    const uint64_t foreign[] = {0x7fff12345678ull, 0x00ab000000001000ull, 0x7fffffffffffffffull, 0x1000};
    for (uint64_t h : foreign)
      REQUIRE(!is_piece(h) && chunk_of(h) == h && piece_of(h) == 0 && pages_of(h) == 1, "foreign handle %llx untouched", (unsigned long long)h);
    REQUIRE(!can_tag(1ull << 48) && !can_tag(kIdrMask + 1) && !can_tag(0x80ab000000000000ull), "handles that do not pack are refused");
    js += "\"tag_round_trips\": " + std::to_string(checked);
  }
  // 2. the bench shape at 1024: one extent serves every batch, one ioctl per batch
  {
    Harness h(kMaxExtentPages, 8192, 0.05);
    h.drv.next = (0xbeefull << 32) | 0x100; // a realistic gpu_id in the handles
    for (int rep = 0; rep < 6; ++rep)
      for (int b = 0; b < 4; ++b) {
        std::vector<int64_t> ids;
        for (int i = 0; i < 1024; ++i) ids.push_back(b * 1024 + i);
        h.map(ids);
        REQUIRE(h.pool.footprint().free_pieces == 0, "whole runs leave no waste");
        h.unmap(ids);
      }
    REQUIRE(h.drv.creates == 1, "one extent of 1024 pages serves every batch, %zu were created", h.drv.creates);
    REQUIRE(h.map_ioctls == 6 * 4, "one ioctl per batch: %zu", h.map_ioctls);
    REQUIRE(h.ctr.reused == (6 * 4 - 1) * 1024, "reuse counter %lld", (long long)h.ctr.reused.load());
    h.pool.drain(0);
    REQUIRE(h.drv.live.empty(), "drain(0) leaves nothing");
    js += ", \"bench_shape\": {\"creates\": 1, \"map_ioctls_per_page\": " + std::to_string(h.map_ioctls / (24.0 * 1024)) + "}";
  }
  // 3. a 1024-page extent taken apart and put back piece by piece: runs past bit 63 of a word, partial reuse, scrub tickets
  {
    Harness h(kMaxExtentPages, 1 << 20, 1e9); // (no governor: the point is the bookkeeping of one extent)
    h.drv.give_tags = true;
    std::vector<int64_t> all;
    for (int i = 0; i < 1024; ++i) all.push_back(i);
    h.map(all);
    // give back a run that straddles words 0-2 and a scattered set, then ask for the run again: one extent, one ioctl
    std::vector<int64_t> run, scattered;
    for (int i = 60; i < 140; ++i) run.push_back(i);
    for (int i = 200; i < 1024; i += 7) scattered.push_back(i);
    h.unmap(run);
    h.unmap(scattered);
    auto f = h.pool.footprint();
    REQUIRE(f.free_pieces == run.size() + scattered.size() && f.partial_extents == 1, "free pieces %zu", f.free_pieces);
    const size_t ioctls = h.map_ioctls;
    h.map(std::vector<int64_t>{5000, 5001, 5002}); // (slots elsewhere: the pieces come from the free run, lowest first)
    REQUIRE(h.map_ioctls == ioctls + 1 && piece_of(h.slot[5000].h) == 60 && piece_of(h.slot[5002].h) == 62, "lowest free run first");
    std::vector<int64_t> run77;
    for (int i = 0; i < 77; ++i) run77.push_back(6000 + i);
    h.map(run77);
    REQUIRE(h.map_ioctls == ioctls + 2 && piece_of(h.slot[6000].h) == 63 && piece_of(h.slot[6076].h) == 139, "a run of 77 across words");
    uint64_t addr[1024];
    std::vector<Phys> back;
    for (auto &kv : h.slot) back.push_back(kv.second);
    REQUIRE(h.pool.scrub_addresses(back.data(), back.size(), addr) == back.size(), "every piece has an alias address");
    for (size_t i = 0; i < back.size(); ++i)
      REQUIRE(addr[i] == h.pool.tag_of(back[i].h) + (uint64_t)piece_of(back[i].h) * (2u << 20), "alias address of piece %u", piece_of(back[i].h));
    h.slot.clear();
    h.out.clear();
    h.pool.release_batch(back.data(), back.size(), 5);
    f = h.pool.footprint();
    REQUIRE(f.idle_pages == 1024 && f.free_pieces == 0 && f.out_pages == 0 && f.bad_releases == 0, "whole again: idle %zu", f.idle_pages);
    Phys q[1024];
    bool rec = false;
    REQUIRE(h.pool.acquire_run(1024, q, &rec, false) == 1024 && rec, "the whole extent again");
    size_t clean = 0;
    for (auto &p : q) clean += p.scrub_ticket == 5;
    REQUIRE(clean == back.size(), "the pieces that came back scrubbed carry the ticket: %zu of %zu", clean, back.size());
    // released twice, or a piece index beyond the extent: counted and ignored
    h.pool.release_batch(q, 1024);
    h.pool.release(q[3]);
    h.pool.release(Phys{piece_id(chunk_of(q[0].h), 1023, 1024) ^ (1ull << kPagesShift), 1}); // (same buffer, claims 1023 pages)
    REQUIRE(h.pool.footprint().bad_releases == 2, "bad releases %zu", h.pool.footprint().bad_releases);
    h.pool.drain(0);
    REQUIRE(h.drv.live.empty() && h.drv.prepared == 1, "one alias dropped, nothing left");
  }
  // 4. a buffer handle that does not pack is given back and the call fails; nothing is left behind
  {
    Harness h(kMaxExtentPages, 1 << 20, 0.05);
    h.drv.next = kIdrMask + 1;
    Phys p[16];
    bool rec = false, threw = false;
    try {
      h.pool.acquire_run(16, p, &rec, true);
    } catch (const std::exception &) {
      threw = true;
    }
    REQUIRE(threw && h.drv.live.empty() && h.pool.footprint().held_pages == 0, "refused and released");
    REQUIRE(h.pool.refill_reserve(64, 64) == 0 && h.drv.live.empty(), "the reserve refuses it too");
  }
  // 5. footprint at 1024 against 64: request-shaped churn and the tides must not get worse
  std::mt19937_64 rng(1);
  for (bool sorted : {false, true}) {
    std::mt19937_64 r64 = rng, r1k = rng;
    const Churn c64 = churn(r64, 64, 0.05, sorted), c1k = churn(r1k, kMaxExtentPages, 0.05, sorted);
    REQUIRE(c1k.p50 <= c64.p50 + 0.005 && c1k.p90 <= c64.p90 + 0.005 && c1k.p90 <= 1.10, "requests%s: p50 %.3f / p90 %.3f at 1024 vs %.3f / %.3f at 64",
            sorted ? " (sorted)" : "", c1k.p50, c1k.p90, c64.p50, c64.p90);
    js += std::string(", ") + fmt(sorted ? "requests_sorted_free_list_k64" : "requests_k64", c64) + ", " +
          fmt(sorted ? "requests_sorted_free_list_k1024" : "requests_k1024", c1k);
  }
  for (double straggle : {0.0, 0.01, 0.05}) {
    std::mt19937_64 r64 = rng, r1k = rng;
    const Churn c64 = batches(r64, 64, straggle), c1k = batches(r1k, kMaxExtentPages, straggle);
    // One straggler pins a whole extent, and a 1024-page extent is 16 times what a 64-page one pins: the governor (5 %) keeps
    // the p90 within a few points of the 64-page pool (measured: +0.3 points at 1 %, +1.8 at 5 % of the pages late).
    REQUIRE(c1k.p90 <= 1.10 && c1k.p90 <= c64.p90 + 0.03, "batches, %.0f %% late: p90 %.3f at 1024 vs %.3f at 64", straggle * 100,
            c1k.p90, c64.p90);
    const std::string n = "batches_straggle" + std::to_string((int)(straggle * 100)) + "pct";
    js += ", " + fmt((n + "_k64").c_str(), c64) + ", " + fmt((n + "_k1024").c_str(), c1k);
  }
  for (size_t run : {32, 256}) {
    std::mt19937_64 r64 = rng, r1k = rng;
    const Churn c64 = tides(r64, 64, run), c1k = tides(r1k, kMaxExtentPages, run);
    REQUIRE(c1k.p50 <= c64.p50 + 0.005 && c1k.p90 <= c64.p90 + 0.005, "tides of runs of %zu: p50 %.3f / p90 %.3f at 1024 vs %.3f / %.3f at 64", run,
            c1k.p50, c1k.p90, c64.p50, c64.p90);
    const std::string n = "tides_run" + std::to_string(run);
    js += ", " + fmt((n + "_k64").c_str(), c64) + ", " + fmt((n + "_k1024").c_str(), c1k);
  }
  js += "}";
  puts(js.c_str());
  return 0;
}
