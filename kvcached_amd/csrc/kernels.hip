// kernels.hip — the device kernels of the path, written for gfx950 (CDNA4) only.
//
// All are byte movers, bound by HBM or by the host link (no MFMA: there is no contraction anywhere on this path); the only
// arithmetic is the opt-in MXFP8 codec of the host copies (encode_blocks_to_host / decode_blocks_from_host, at the end).
// What matters on MI355X, and what the code below does:
//   * every wave-instruction touches 64 lanes x 16 B = 1 KiB of contiguous memory
//     (global_store_dwordx4 / global_load_dwordx4 / global_load_lds_dwordx4);
//   * one workgroup per 64 KiB slab (fill) or per <=32 KiB tile (compaction) and NO grid-stride
//     loop: with 256 CUs in 8 XCDs a batch is tens of thousands of workgroups, and the probe
//     showed short-lived workgroups beating a persistent 2048-block grid (6.9 vs 6.1 TB/s);
//   * the page / region tables ride in the kernarg segment (scalar loads, no table in HBM,
//     no extra copy on the launch path);
//   * the blockIdx -> work mapping is XCD-aware: each XCD (own L2) owns whole pages instead of
//     every XCD touching every page (+12 % measured, see zero_fill_pages below).
//
// Algorithmic bytes: zero_fill_pages writes page_bytes per page (2 097 152 B
// for a 2 MiB page) and reads nothing; compact_blocks reads + writes block_bytes per
// (region, move) = 2 x block_bytes x n_regions per moved block.

#include "codec_math.hpp"
#include "kernels.hpp"

namespace kvc {

typedef unsigned int v4u __attribute__((ext_vector_type(4)));

struct PageTable {
  void *p[kMaxPtrsPerLaunch];
};

// ---------------------------------------------------------------------------- zero_fill_pages
// One workgroup zeroes one 64 KiB slab: THREADS x STORES x 16 B, lane l of the workgroup stores at
// slab + (i*THREADS + l)*16, so every store instruction of a wave covers one aligned 1 KiB run.
//
// blockIdx -> (page, slab) is XCD-aware. Workgroups are dealt round-robin over the 8 XCDs (block b
// runs on XCD b % 8), so the naive "consecutive blocks take consecutive slabs" makes all eight
// XCD L2s write into every page at once. Here XCD x owns pages x, x+8, x+16, ... completely:
//     x = b % 8, i = b / 8, page = (i / slabs_per_page) * 8 + x, slab = i % slabs_per_page
// Measured on MI355X against the interleaved mapping and hipMemsetAsync (tools/fill_bench.cpp, 2 GiB of 2 MiB pages,
// sequential and shuffled lists: profiles/r01_fill_bench.log; today's rates of the default: DESIGN.md §5, §6).
// The placement is a speed heuristic only: any block->XCD assignment is correct.
// XCD_BLOCKED (variant 4, A/B): XCD x owns the pages [x * ceil(n/8), (x+1) * ceil(n/8)) - a contiguous eighth of the list (the
// list arrives sorted into runs of up to 64 adjacent pages of one physical extent) - instead of every eighth page.
template <int THREADS, bool NT, bool XCD_PAGES, bool XCD_BLOCKED = false>
__global__ __launch_bounds__(THREADS) void zero_fill_pages_kernel(PageTable pages, unsigned slabs_per_page,
                                                                   unsigned n_pages) {
  constexpr int STORES = (int)(kFillSlabBytes / 16 / THREADS);
  unsigned page, slab;
  if (XCD_PAGES) {
    const unsigned x = blockIdx.x & 7u, i = blockIdx.x >> 3;
    const unsigned q = i / slabs_per_page;
    slab = i - q * slabs_per_page;
    page = XCD_BLOCKED ? x * ((n_pages + 7u) >> 3) + q : q * 8u + x;
    if (page >= n_pages) return; // the grid is padded to a multiple of 8 pages (wave-uniform exit)
  } else {
    page = blockIdx.x / slabs_per_page;
    slab = blockIdx.x - page * slabs_per_page;
  }
  v4u *dst = reinterpret_cast<v4u *>(static_cast<char *>(pages.p[page]) + (size_t)slab * kFillSlabBytes) + threadIdx.x;
  const v4u z = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < STORES; ++i) {
    if (NT)
      __builtin_nontemporal_store(z, dst + i * THREADS);
    else
      dst[i * THREADS] = z;
  }
}

// variant number -> kernel and how it is launched: row i is KVC_OPT_FILL_VARIANT i. Rows 1-5 are kept for A/B runs.
using FillKernel = void (*)(PageTable, unsigned, unsigned);
struct FillVariant {
  FillKernel kernel;
  int threads;  // per workgroup
  bool pad8;    // grid padded to a multiple of 8 pages (every XCD-aware placement)
  bool shuffle; // page table laid out in the fixed pseudo-random order (below)
  const char *name; // for the reader of this table
};
static const FillVariant kFillVariants[] = {
    {zero_fill_pages_kernel<512, false, true>, 512, true, true, "every eighth page per XCD (default)"},
    {zero_fill_pages_kernel<512, false, false>, 512, false, true, "interleaved slabs (the pre-XCD-aware mapping)"},
    {zero_fill_pages_kernel<512, true, true>, 512, true, true, "non-temporal stores (slower on gfx950: DESIGN.md §5)"},
    {zero_fill_pages_kernel<1024, false, true>, 1024, true, true, "1024 threads per workgroup"},
    {zero_fill_pages_kernel<512, false, true, true>, 512, true, true, "a contiguous eighth of the page list per XCD"},
    {zero_fill_pages_kernel<512, false, true>, 512, true, false, "the default kernel on the caller's order of pages"},
};
static constexpr int kNumFillVariants = (int)(sizeof(kFillVariants) / sizeof(kFillVariants[0]));
static_assert(kNumFillVariants == 6, "a row added or removed renumbers the variants that KVC_OPT_FILL_VARIANT names");

hipError_t launch_zero_fill_pages(void *const *pages, int n, size_t page_bytes, hipStream_t stream, int variant) {
  if (n <= 0) return hipSuccess;
  if (n > kMaxPtrsPerLaunch || page_bytes == 0 || page_bytes % kFillSlabBytes != 0) return hipErrorInvalidValue;
  // A number outside the table selects the default (callers pass an environment variable's integer through).
  const FillVariant &v = kFillVariants[variant >= 0 && variant < kNumFillVariants ? variant : 0];
  // The order of the table decides which pages are written AT THE SAME TIME (the ~64 pages the chip has in flight are consecutive
  // table entries), and the memory system likes those scattered: a list of adjacent pages in address order fills slowest, the
  // same pages shuffled fastest, runs of 64 adjacent pages in shuffled order - what the allocator's sorted batches look like - in
  // between (benchmarks/probe_fill_rate_per_buffer.py; figures: DESIGN.md §5). A regular stride is not enough (i * 0.618 n mod n),
  // so the table is laid out in a fixed pseudo-random order (Fisher-Yates with a constant seed, the same for every launch of
  // the same size): whatever order the caller's list has, the kernel sees a shuffled one. Zeroing does not care about the order.
  PageTable t;
  static thread_local int perm_n = 0;
  static thread_local unsigned short perm[kMaxPtrsPerLaunch];
  const bool shuffle = v.shuffle && n > 16;
  if (shuffle && perm_n != n) {
    for (int i = 0; i < n; ++i) perm[i] = (unsigned short)i;
    uint64_t x = 0x9e3779b97f4a7c15ull; // (splitmix-style steps; any fixed sequence will do)
    for (int i = n - 1; i > 0; --i) {
      x += 0x9e3779b97f4a7c15ull;
      uint64_t z = x;
      z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
      z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
      z ^= z >> 31;
      const int j = (int)(z % (uint64_t)(i + 1));
      const unsigned short tmp = perm[i];
      perm[i] = perm[j];
      perm[j] = tmp;
    }
    perm_n = n;
  }
  for (int i = 0; i < n; ++i) {
    if (reinterpret_cast<uintptr_t>(pages[i]) % 16 != 0) return hipErrorInvalidValue;
    t.p[shuffle ? perm[i] : i] = pages[i];
  }
  const unsigned slabs = (unsigned)(page_bytes / kFillSlabBytes);
  const size_t padded = ((size_t)n + 7) / 8 * 8;
  if ((size_t)slabs * padded > 0x7fffffffull) return hipErrorInvalidValue; // the padded grid bounds every variant's
  const size_t grid = (size_t)slabs * (v.pad8 ? padded : (size_t)n);
  v.kernel<<<dim3((unsigned)grid), dim3(v.threads), 0, stream>>>(t, slabs, (unsigned)n);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------- peek_poke (init self test)
// One lane writes `value` to *p (if do_write) and copies *p to *out, with system-scope loads/stores that bypass nothing
// they should not: what the TLB self test of KvAllocator::init looks at memory with (through the GPU's own address
// translation, which is the thing under test - a host copy would go another way).
__global__ void peek_poke_kernel(unsigned *p, unsigned *out, unsigned value, int do_write) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if (do_write) __hip_atomic_store(p, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    *out = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
hipError_t launch_peek_poke(void *p, unsigned *out_dev, unsigned value, bool do_write, hipStream_t stream) {
  peek_poke_kernel<<<dim3(1), dim3(64), 0, stream>>>(static_cast<unsigned *>(p), out_dev, value, do_write ? 1 : 0);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------- the tile copy (compact_blocks, host copies)
static constexpr int kCopyThreads = 256; // 4 waves
static constexpr int kCopyWaves = kCopyThreads / 64;
static constexpr int kPiece = 1024; // one wave-instruction
static constexpr int kTile16 = 16 * 1024, kTile32 = 32 * 1024; // bytes per workgroup

// Where tile t (TILE bytes each) of block `id` of the region at `base` starts. 64 bits throughout: regions are larger than 4 GiB.
template <int TILE>
__device__ __forceinline__ char *tile_address(void *base, int64_t id, unsigned block_bytes, unsigned t) {
  return static_cast<char *>(base) + id * (int64_t)block_bytes + (size_t)t * TILE;
}

// A workgroup of 4 waves copies one tile of at most TILE bytes, 1 KiB per wave-instruction; `remain` = bytes of the tile that
// exist (>= 16, a multiple of 16). A full tile (a wave-uniform test) takes a path without per-lane predicates.
//   LDS              staged through LDS: each wave DMAs its pieces global->LDS (global_load_lds_dwordx4: per-lane source address,
//                    wave-uniform LDS base + lane*16), waits for its own DMAs (vmcnt), reads them back with ds_read_b128 and
//                    streams them out with global_store_dwordx4. A wave only ever reads LDS bytes it loaded itself, so no barrier
//                    is needed; TILE bytes of LDS per workgroup. Otherwise staged through registers: all loads of a lane in
//                    flight first, then the stores.
//   NT_LOAD/NT_STORE the nt bit on that side: for memory whose every byte is touched exactly once.
//   INTERLEAVED      a wave owns every fourth piece (k * waves + wave), so that a block smaller than the tile keeps all four
//                    waves busy; otherwise a contiguous quarter of the tile (wave * pieces + k). It decides which bytes are in
//                    flight together, and the recorded A/B figures of the 16 KiB compaction variants were taken with the latter.
//   RAGGED_IN_FLIGHT (register staging) a ragged tile, too, has all its loads issued before its first store and keeps the nt
//                    bits: the host copies, for the link's latency. Otherwise a ragged tile goes one piece at a time with plain
//                    accesses: all of them in flight would cost the 32 KiB compaction kernel 228 VGPRs instead of 46.
template <int TILE, bool LDS, bool NT_LOAD, bool NT_STORE, bool INTERLEAVED, bool RAGGED_IN_FLIGHT>
__device__ __forceinline__ void copy_tile(const char *src, char *dst, unsigned remain) {
  constexpr int PIECES = TILE / kPiece / kCopyWaves; // per wave
  __shared__ __attribute__((aligned(16))) unsigned char tile[LDS ? TILE : 16];
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool full = remain >= (unsigned)TILE; // wave-uniform: every tile but a ragged last one
  const unsigned limit = full ? (unsigned)TILE : remain; // bytes to copy
  auto piece = [&](int k) -> unsigned { return INTERLEAVED ? k * kCopyWaves + wave : wave * PIECES + k; };
  if (LDS) {
#pragma unroll
    for (int k = 0; k < PIECES; ++k) {
      const unsigned off = piece(k) * kPiece + lane * 16;
      if (full || off < limit)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + off),
                                         (__attribute__((address_space(3))) void *)(tile + piece(k) * kPiece), 16, 0,
                                         NT_LOAD ? 2 : 0); // aux bit 1 = nt on gfx94x/gfx950
    }
    // The DMA writes LDS behind the compiler's back: wait for this wave's pieces by hand.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  auto load = [](const char *p) {
    const v4u *in = reinterpret_cast<const v4u *>(p);
    return NT_LOAD ? __builtin_nontemporal_load(in) : *in;
  };
  auto store = [](char *p, v4u v) {
    if (NT_STORE)
      __builtin_nontemporal_store(v, reinterpret_cast<v4u *>(p));
    else
      *reinterpret_cast<v4u *>(p) = v;
  };
  if (full) { // every piece into registers (from LDS, or from global memory with all loads in flight), then out
    v4u v[PIECES];
#pragma unroll
    for (int k = 0; k < PIECES; ++k) {
      const unsigned p = piece(k) * kPiece; // (wave-uniform; the lane's part is added to the pointer on its own)
      v[k] = LDS ? *reinterpret_cast<const v4u *>(tile + p + lane * 16) : load(src + p + lane * 16);
    }
#pragma unroll
    for (int k = 0; k < PIECES; ++k) store(dst + piece(k) * kPiece + lane * 16, v[k]);
  } else if (!LDS && RAGGED_IN_FLIGHT) {
    v4u v[PIECES];
#pragma unroll
    for (int k = 0; k < PIECES; ++k) {
      const unsigned off = piece(k) * kPiece + lane * 16;
      if (off < limit) v[k] = load(src + off);
    }
#pragma unroll
    for (int k = 0; k < PIECES; ++k) {
      const unsigned off = piece(k) * kPiece + lane * 16;
      if (off < limit) store(dst + off, v[k]);
    }
  } else {
    for (int k = 0; k < PIECES; ++k) {
      const unsigned off = piece(k) * kPiece + lane * 16;
      const v4u *in = LDS ? reinterpret_cast<const v4u *>(tile + off) : reinterpret_cast<const v4u *>(src + off);
      if (off < limit) *reinterpret_cast<v4u *>(dst + off) = *in;
    }
  }
}

// ---------------------------------------------------------------------------- compact_blocks
struct CompactArgs {
  void *base[kMaxRegionsPerLaunch];
  int64_t src[kMaxMovesPerLaunch];
  int64_t dst[kMaxMovesPerLaunch];
};
static_assert(sizeof(CompactArgs) <= 8192, "kernarg segment budget");

// blockIdx -> (region, move, tile); speed only, any placement is correct. Workgroups are dealt round-robin over the 8 XCDs
// (block b runs on XCD b % 8), and all but kFlat let one XCD copy a whole block (all its tiles) - the placement idea of
// zero_fill_pages - over a grid padded to a multiple of 8 (region, move) pairs.
enum Placement {
  kFlat,              // consecutive workgroups take consecutive tiles: every XCD touches every block
  kXcdEveryEighth,    // XCD x takes the pairs x, x+8, ...
  kXcdEighth,         // XCD x takes a contiguous eighth of the pairs: neighbouring moves of a planner-made list share their source
                      // and destination pages, and an XCD has its own L2 / translation cache
  kXcdEighthRotated,  // the same, and XCD x starts x * (an eighth of its range + 57) pairs into its range (wrapping round): with
                      // every XCD walking the SAME move list through its own regions in step, the eight streams would read the
                      // same block index of regions that lie a power of two apart at the same moment
};
template <Placement PLACE>
__device__ __forceinline__ bool compact_index(unsigned n_moves, unsigned n_regions, unsigned tiles_per_block, unsigned &r,
                                              unsigned &m, unsigned &t) {
  if (PLACE == kFlat) {
    t = blockIdx.x % tiles_per_block;
    m = (blockIdx.x / tiles_per_block) % n_moves;
    r = blockIdx.x / (tiles_per_block * n_moves);
    return true;
  }
  const unsigned x = blockIdx.x & 7u, i = blockIdx.x >> 3;
  unsigned q = i / tiles_per_block;
  t = i - q * tiles_per_block;
  unsigned pair = q * 8u + x;
  if (PLACE != kXcdEveryEighth) {
    const unsigned per_xcd = (n_moves * n_regions + 7u) >> 3;
    if (PLACE == kXcdEighthRotated) q = (q + x * ((per_xcd >> 3) + 57u)) % per_xcd;
    pair = x * per_xcd + q;
  }
  if (pair >= n_moves * n_regions) return false; // the padding of the grid (wave-uniform exit)
  r = pair / n_moves;
  m = pair - r * n_moves;
  return true;
}

template <int TILE, bool LDS, bool NT, Placement PLACE, bool INTERLEAVED>
__global__ __launch_bounds__(kCopyThreads) void compact_blocks_kernel(CompactArgs a, unsigned n_moves, unsigned n_regions,
                                                                       unsigned tiles_per_block, unsigned block_bytes) {
  unsigned r, m, t;
  if (!compact_index<PLACE>(n_moves, n_regions, tiles_per_block, r, m, t)) return;
  copy_tile<TILE, LDS, NT, NT, INTERLEAVED, false>(tile_address<TILE>(a.base[r], a.src[m], block_bytes, t),
                                                   tile_address<TILE>(a.base[r], a.dst[m], block_bytes, t),
                                                   block_bytes - t * TILE);
}

// variant number -> kernel and how it is launched: row i is KVC_OPT_COMPACT_VARIANT i, and row 0, the default, repeats row 9.
// Rows 1-8, 10 and 11 are kept for A/B runs. What the history says:
//   * nt on loads and stores: every byte is touched exactly once, and keeping it out of the way of the L2/MALL is worth +2..7 %
//     (profiles/r01_compact_bench.jsonl; same on a plain contiguous copy, tools/copy_bench.cpp);
//   * 32 KiB tiles (8 KiB in flight per wave): the same rate as 16 KiB tiles on 32 KiB blocks, +2.6 % on 16 KiB blocks and +12 %
//     on ragged 18 KiB MLA blocks - one tile per block instead of a full one and a 2 KiB tail (profiles/r03_compact_bench.jsonl);
//   * a contiguous eighth of the pairs per XCD instead of every eighth pair: with 64 regions an XCD then works inside 8 of them,
//     and its L2 / translation cache sees an eighth of the pages - +10..18 % on the Llama-3-8B geometry, random or
//     planner-ordered moves alike (profiles/r03_compact_bench_blocked.jsonl).
using CompactKernel = void (*)(CompactArgs, unsigned, unsigned, unsigned, unsigned);
struct CompactVariant {
  CompactKernel kernel; // kCopyThreads per workgroup, every one
  int tile;             // bytes per workgroup
  bool pad8;            // grid padded to a multiple of 8 pairs (every placement but kFlat)
  const char *name;     // for the reader of this table
};
static const CompactVariant kCompactVariants[] = {
    {compact_blocks_kernel<kTile32, true, true, kXcdEighth, true>, kTile32, true, "the default: row 9"},
    {compact_blocks_kernel<kTile16, false, true, kXcdEveryEighth, false>, kTile16, true, "registers, 16 KiB, nt, every eighth pair per XCD"},
    {compact_blocks_kernel<kTile16, true, false, kFlat, false>, kTile16, false, "LDS, 16 KiB, temporal, flat (the first version)"},
    {compact_blocks_kernel<kTile16, false, false, kFlat, false>, kTile16, false, "registers, 16 KiB, temporal, flat"},
    {compact_blocks_kernel<kTile16, true, false, kXcdEveryEighth, false>, kTile16, true, "LDS, 16 KiB, temporal, every eighth pair per XCD"},
    {compact_blocks_kernel<kTile16, false, false, kXcdEveryEighth, false>, kTile16, true, "registers, 16 KiB, temporal, every eighth pair per XCD"},
    {compact_blocks_kernel<kTile32, true, true, kXcdEveryEighth, true>, kTile32, true, "LDS, 32 KiB, nt, every eighth pair per XCD (the default of most of round 3)"},
    {compact_blocks_kernel<kTile32, false, true, kXcdEveryEighth, true>, kTile32, true, "registers, 32 KiB, nt, every eighth pair per XCD"},
    {compact_blocks_kernel<kTile16, true, true, kXcdEveryEighth, false>, kTile16, true, "LDS, 16 KiB, nt, every eighth pair per XCD (the default until round 3)"},
    {compact_blocks_kernel<kTile32, true, true, kXcdEighth, true>, kTile32, true, "LDS, 32 KiB, nt, a contiguous eighth of the pairs per XCD"},
    {compact_blocks_kernel<kTile32, false, true, kXcdEighth, true>, kTile32, true, "registers, 32 KiB, nt, a contiguous eighth of the pairs per XCD"},
    {compact_blocks_kernel<kTile32, true, true, kXcdEighthRotated, true>, kTile32, true, "as row 9, the XCDs out of step"},
};
static constexpr int kNumCompactVariants = (int)(sizeof(kCompactVariants) / sizeof(kCompactVariants[0]));
// What a number outside the table has always selected (callers pass an environment variable's integer through).
static constexpr int kCompactFallbackVariant = 8;
static_assert(kNumCompactVariants == 12 && kCompactFallbackVariant < kNumCompactVariants,
              "a row added or removed renumbers the variants: KVC_OPT_COMPACT_VARIANT, bench_compact.py and the tests name them");

// Copy the region bases into a kernarg struct; false for a base that is not 16-byte aligned.
static bool copy_bases(void **out, void *const *bases, int n_regions) {
  for (int r = 0; r < n_regions; ++r) {
    if (reinterpret_cast<uintptr_t>(bases[r]) % 16 != 0) return false;
    out[r] = bases[r];
  }
  return true;
}

hipError_t launch_compact_blocks(void *const *bases, int n_regions, const int64_t *src, const int64_t *dst, int n_moves,
                                 size_t block_bytes, hipStream_t stream, int variant) {
  if (n_regions <= 0 || n_moves <= 0) return hipSuccess;
  if (n_regions > kMaxRegionsPerLaunch || n_moves > kMaxMovesPerLaunch || block_bytes == 0 || block_bytes % 16 != 0 ||
      block_bytes > 0x7fffffffull)
    return hipErrorInvalidValue;
  CompactArgs a;
  if (!copy_bases(a.base, bases, n_regions)) return hipErrorInvalidValue;
  for (int i = 0; i < n_moves; ++i) {
    if (src[i] < 0 || dst[i] < 0) return hipErrorInvalidValue;
    a.src[i] = src[i];
    a.dst[i] = dst[i];
  }
  const CompactVariant &v = kCompactVariants[variant >= 0 && variant < kNumCompactVariants ? variant : kCompactFallbackVariant];
  const size_t pairs = (size_t)n_moves * (size_t)n_regions, padded = (pairs + 7) / 8 * 8;
  // the padded grid of the smallest tile bounds every variant's: what is refused does not depend on the variant
  if ((block_bytes + kTile16 - 1) / kTile16 * padded > 0x7fffffffull) return hipErrorInvalidValue;
  const unsigned tiles = (unsigned)((block_bytes + v.tile - 1) / v.tile);
  const size_t grid = (size_t)tiles * (v.pad8 ? padded : pairs);
  v.kernel<<<dim3((unsigned)grid), dim3(kCopyThreads), 0, stream>>>(a, (unsigned)n_moves, (unsigned)n_regions, tiles,
                                                                    (unsigned)block_bytes);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------- copy_blocks_to_host / copy_blocks_from_host
// Offload / restore of live blocks (KVCacheManager.offload / .restore): for block i < n and region r < n_regions,
//   host + ((i * row_regions + region0 + r) * block_bytes)  <->  base[r] + id[i] * block_bytes
// The host image is block-major ([block][region][bytes]); `host` is the device address of pinned host memory.
// The far side is the host link (PCIe Gen5 x16, 63 GB/s by spec, against 6+ TB/s of HBM), so what matters is only that
// enough requests are in flight to cover its latency - microseconds for a read of host memory: one workgroup per
// <= 16 KiB tile of a (block, region) pair, every lane with all four of its 16-byte loads issued before its first store.
// That is 16 KiB in flight per workgroup and up to 8 workgroups per CU, where 63 GB/s x 2 us of latency is 126 KiB for
// the whole chip. No LDS, no grid-stride loop, the tables in the kernarg segment as in compact_blocks. The HBM side
// is accessed non-temporally (every byte once); the host side with plain accesses. Workgroups are ordered tile-fastest,
// then region, then block, so consecutive workgroups cover consecutive host bytes.
struct HostCopyArgs {
  void *base[kMaxRegionsPerLaunch];
  int64_t id[kMaxIdsPerLaunch];
};
static_assert(sizeof(HostCopyArgs) <= 12 * 1024, "kernarg segment budget");
// The same with a slot table (launch_copy_blocks_host_slots): block i's row of the host image is row slot[i] of a pinned arena
// (HostBlockStore), not row i. 32-bit slots: the row's byte offset is formed in 64 bits, and 2^32 rows are more than any host has.
struct HostSlotArgs {
  void *base[kMaxRegionsPerLaunch];
  int64_t id[kMaxSlotIdsPerLaunch];
  uint32_t slot[kMaxSlotIdsPerLaunch];
};
static_assert(sizeof(HostSlotArgs) <= 12 * 1024, "kernarg segment budget");
// The row of the host image that holds block i of the launch (one more scalar load per workgroup with a slot table).
__device__ __forceinline__ size_t host_row(const HostCopyArgs &, unsigned i) { return i; }
__device__ __forceinline__ size_t host_row(const HostSlotArgs &a, unsigned i) { return a.slot[i]; }

// Which (block, region) pair and which tile of it this workgroup has: the device address of the tile, the index of the pair's
// record in the host image, and the tile number. Tile-fastest, then region, then block.
struct HostTile {
  char *dev;
  size_t record;
  unsigned t;
};
template <class Args>
__device__ __forceinline__ HostTile host_tile(const Args &a, unsigned n_regions, unsigned region0, unsigned row_regions,
                                              unsigned tiles, unsigned block_bytes) {
  const unsigned pair = blockIdx.x / tiles, t = blockIdx.x - pair * tiles;
  const unsigned i = pair / n_regions, r = pair - i * n_regions;
  return {tile_address<kTile16>(a.base[r], a.id[i], block_bytes, t), host_row(a, i) * row_regions + region0 + r, t};
}

template <bool TO_HOST, class Args>
__device__ __forceinline__ void copy_blocks_host_tile(const Args &a, char *host, unsigned n_regions, unsigned region0,
                                                      unsigned row_regions, unsigned tiles, unsigned block_bytes) {
  const HostTile w = host_tile(a, n_regions, region0, row_regions, tiles, block_bytes);
  char *hst = host + w.record * block_bytes + (size_t)w.t * kTile16;
  copy_tile<kTile16, false, TO_HOST, !TO_HOST, true, true>(TO_HOST ? w.dev : hst, TO_HOST ? hst : w.dev,
                                                           block_bytes - w.t * kTile16);
}

// (two named kernels rather than one template: a profile names the direction)
__global__ __launch_bounds__(kCopyThreads) void copy_blocks_to_host_kernel(HostCopyArgs a, char *host, unsigned n_regions,
                                                                            unsigned region0, unsigned row_regions,
                                                                            unsigned tiles, unsigned block_bytes) {
  copy_blocks_host_tile<true>(a, host, n_regions, region0, row_regions, tiles, block_bytes);
}

__global__ __launch_bounds__(kCopyThreads) void copy_blocks_from_host_kernel(HostCopyArgs a, char *host, unsigned n_regions,
                                                                              unsigned region0, unsigned row_regions,
                                                                              unsigned tiles, unsigned block_bytes) {
  copy_blocks_host_tile<false>(a, host, n_regions, region0, row_regions, tiles, block_bytes);
}

__global__ __launch_bounds__(kCopyThreads) void copy_blocks_to_host_slots_kernel(HostSlotArgs a, char *host, unsigned n_regions,
                                                                                  unsigned region0, unsigned row_regions,
                                                                                  unsigned tiles, unsigned block_bytes) {
  copy_blocks_host_tile<true>(a, host, n_regions, region0, row_regions, tiles, block_bytes);
}

__global__ __launch_bounds__(kCopyThreads) void copy_blocks_from_host_slots_kernel(HostSlotArgs a, char *host, unsigned n_regions,
                                                                                    unsigned region0, unsigned row_regions,
                                                                                    unsigned tiles, unsigned block_bytes) {
  copy_blocks_host_tile<false>(a, host, n_regions, region0, row_regions, tiles, block_bytes);
}

// ---------------------------------------------------------------------------- encode_blocks_to_host / decode_blocks_from_host
// The same copies through the MXFP8 codec (KVCacheManager.offload(codec="mxfp8"); the format: INTEGRATION.md §6): the blocks
// hold bf16 or fp16, and a group of 32 consecutive elements (64 bytes) crosses the link as 32 e4m3fn codes and one shared
// power-of-two scale byte (E8M0) - 33 bytes for 64. The record of a (block, region) pair is its block_bytes / 2 codes in
// element order, then its block_bytes / 64 scale bytes in group order, at host + record index * (block_bytes / 2 +
// block_bytes / 64). block_bytes is a multiple of 1 KiB, so a tile is whole pieces and every predicate below is wave-uniform.
// Work decomposition, placement of the waves' pieces and the memory accesses are those of copy_blocks_host_tile: a lane's
// 16-byte access on the HBM side is 8 elements, a group is one quad of lanes (a DPP quad_perm reduction, no LDS, no
// barrier), a lane's codes of a piece are one 8-byte access on the host side, and the 16 scale bytes of a piece are ONE
// 16-byte access by one lane: lane k of a wave has those of the wave's piece k, gathered / spread with v_readlane.
// The arithmetic is integer work on the bit patterns plus fp32 multiplications by powers of two (exact): it does not use
// the scaled-conversion instructions of gfx950, whose rounding and scale handling nothing here could check to the bit.
// fp32 denormals (bf16 groups below 2^-100) are kept - the float mode hipcc gives these kernels - and the tests pin them too.
typedef unsigned int v2u __attribute__((ext_vector_type(2)));
static constexpr int kCodecPieces = kTile16 / kPiece / kCopyWaves; // per wave

__device__ __forceinline__ unsigned quad_max(unsigned x) { // the maximum over the lane's quad, in every lane of it
  const unsigned y = max(x, (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, true)); // quad_perm:[1,0,3,2]
  return max(y, (unsigned)__builtin_amdgcn_mov_dpp((int)y, 0x4E, 0xF, 0xF, true));             // quad_perm:[2,3,0,1]
}

// Half16<F16>, e4m3_magnitude_code and e4m3_magnitude - the steps without lane intrinsics - are in codec_math.hpp, which also
// compiles as plain C++ so that the tests can enumerate them on the CPU.

template <bool F16, bool TO_HOST, class Args>
__device__ __forceinline__ void codec_blocks_host_tile(const Args &a, char *host, unsigned n_regions, unsigned region0,
                                                       unsigned row_regions, unsigned tiles, unsigned block_bytes) {
  using H = Half16<F16>;
  const HostTile w = host_tile(a, n_regions, region0, row_regions, tiles, block_bytes);
  char *record = host + w.record * (size_t)(block_bytes / 2 + block_bytes / 64);
  char *codes = record + (size_t)w.t * (kTile16 / 2);
  char *scales = record + block_bytes / 2 + (size_t)w.t * (kTile16 / 64);
  const unsigned pieces = min(block_bytes - w.t * kTile16, (unsigned)kTile16) / kPiece; // of this tile
  // (readfirstlane: tells the compiler that the wave number, and so every test of a piece against `pieces`, is wave-uniform)
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  auto piece = [&](unsigned k) -> unsigned { return k * kCopyWaves + wave; }; // as copy_tile's INTERLEAVED
  const bool scale_lane = lane < (unsigned)kCodecPieces && piece(lane) < pieces; // lane k: the 16 scale bytes of piece k
  if (TO_HOST) {
    v4u v[kCodecPieces];
#pragma unroll
    for (int k = 0; k < kCodecPieces; ++k)
      if (piece(k) < pieces) v[k] = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(w.dev + piece(k) * kPiece) + lane);
    unsigned quad_scales = 0; // byte k: the scale byte of this lane's group in piece k
#pragma unroll
    for (int k = 0; k < kCodecPieces; ++k) {
      if (piece(k) >= pieces) continue;
      unsigned amax = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) amax = max(amax, max(v[k][j] & 0x7fffu, (v[k][j] >> 16) & 0x7fffu));
      amax = quad_max(amax);
      const bool finite = amax < H::kInf;
      const unsigned sb = finite ? H::scale_byte(amax) : 0xffu;
      const float down = __uint_as_float((254u - sb) << 23); // 2^-(sb - 127); sb <= 247 for a finite group
      v2u c = {0u, 0u};
      if (finite) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned lo = e4m3_magnitude_code(H::to_float(v[k][j] & 0x7fffu) * down),
                         hi = e4m3_magnitude_code(H::to_float((v[k][j] >> 16) & 0x7fffu) * down);
          const unsigned signs = ((v[k][j] >> 8) & 0x80u) | ((v[k][j] >> 16) & 0x8000u);
          c[j >> 1] |= (lo | (hi << 8) | signs) << ((j & 1) * 16);
        }
      }
      quad_scales |= sb << (k * 8);
      *(reinterpret_cast<v2u *>(codes + piece(k) * (kPiece / 2)) + lane) = c;
    }
    v4u s;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) // group 4j + b of every piece, from the first lane of its quad; this lane keeps its piece's
        s[j] |= ((__builtin_amdgcn_readlane((int)quad_scales, (4 * j + b) * 4) >> ((lane & 3u) * 8)) & 0xffu) << (b * 8);
    }
    if (scale_lane) *reinterpret_cast<v4u *>(scales + piece(lane) * (kPiece / 64)) = s;
  } else {
    v2u c[kCodecPieces];
    v4u s = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < kCodecPieces; ++k)
      if (piece(k) < pieces) c[k] = *(reinterpret_cast<const v2u *>(codes + piece(k) * (kPiece / 2)) + lane);
    if (scale_lane) s = *reinterpret_cast<const v4u *>(scales + piece(lane) * (kPiece / 64));
#pragma unroll
    for (int k = 0; k < kCodecPieces; ++k) {
      if (piece(k) >= pieces) continue;
      unsigned word = 0; // the four scale bytes that hold this lane's group (lane / 4) of piece k
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned sj = (unsigned)__builtin_amdgcn_readlane((int)s[j], k);
        word = (lane >> 4) == (unsigned)j ? sj : word;
      }
      const unsigned sb = (word >> (((lane >> 2) & 3u) * 8)) & 0xffu;
      const float up = __uint_as_float(sb ? sb << 23 : 0x00400000u); // 2^(sb - 127)
      v4u out;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned pair = (c[k][j >> 1] >> ((j & 1) * 16)) & 0xffffu;
        const unsigned lo = H::from_float(e4m3_magnitude(pair) * up), hi = H::from_float(e4m3_magnitude(pair >> 8) * up);
        const unsigned signs = ((pair & 0x80u) << 8) | ((pair & 0x8000u) << 16);
        out[j] = sb == 0xffu ? H::kQuietNan * 0x10001u : lo | (hi << 16) | signs;
      }
      __builtin_nontemporal_store(out, reinterpret_cast<v4u *>(w.dev + piece(k) * kPiece) + lane);
    }
  }
}

// (named kernels, as above: a profile names the direction and the element type)
#define KVC_CODEC_KERNEL(name, Args, F16, TO_HOST)                                                                            \
  __global__ __launch_bounds__(kCopyThreads) void name(Args a, char *host, unsigned n_regions, unsigned region0,               \
                                                       unsigned row_regions, unsigned tiles, unsigned block_bytes) {           \
    codec_blocks_host_tile<F16, TO_HOST>(a, host, n_regions, region0, row_regions, tiles, block_bytes);                        \
  }
KVC_CODEC_KERNEL(encode_blocks_to_host_bf16_kernel, HostCopyArgs, false, true)
KVC_CODEC_KERNEL(encode_blocks_to_host_f16_kernel, HostCopyArgs, true, true)
KVC_CODEC_KERNEL(decode_blocks_from_host_bf16_kernel, HostCopyArgs, false, false)
KVC_CODEC_KERNEL(decode_blocks_from_host_f16_kernel, HostCopyArgs, true, false)
KVC_CODEC_KERNEL(encode_blocks_to_host_slots_bf16_kernel, HostSlotArgs, false, true)
KVC_CODEC_KERNEL(encode_blocks_to_host_slots_f16_kernel, HostSlotArgs, true, true)
KVC_CODEC_KERNEL(decode_blocks_from_host_slots_bf16_kernel, HostSlotArgs, false, false)
KVC_CODEC_KERNEL(decode_blocks_from_host_slots_f16_kernel, HostSlotArgs, true, false)
#undef KVC_CODEC_KERNEL

hipError_t launch_copy_blocks_host(bool to_host, void *const *bases, int n_regions, int region0, int row_regions,
                                   const int64_t *ids, int n, size_t block_bytes, void *host, hipStream_t stream, int codec) {
  if (n_regions <= 0 || n <= 0) return hipSuccess;
  if (n_regions > kMaxRegionsPerLaunch || n > kMaxIdsPerLaunch || region0 < 0 || row_regions < region0 + n_regions ||
      block_bytes == 0 || block_bytes % 16 != 0 || block_bytes > 0x7fffffffull || reinterpret_cast<uintptr_t>(host) % 16 != 0 ||
      host_record_bytes(codec, block_bytes) == 0)
    return hipErrorInvalidValue;
  HostCopyArgs a;
  if (!copy_bases(a.base, bases, n_regions)) return hipErrorInvalidValue;
  for (int i = 0; i < n; ++i) {
    if (ids[i] < 0) return hipErrorInvalidValue;
    a.id[i] = ids[i];
  }
  const unsigned tiles = (unsigned)((block_bytes + kTile16 - 1) / kTile16);
  const size_t grid = (size_t)tiles * (size_t)n * (size_t)n_regions;
  if (grid > 0x7fffffffull) return hipErrorInvalidValue;
  // row: the codec of the host image (kCodecRaw, kCodecMxfp8Bf16, kCodecMxfp8F16); column: from the host, to the host
  using HostKernel = void (*)(HostCopyArgs, char *, unsigned, unsigned, unsigned, unsigned, unsigned);
  static const HostKernel kernels[3][2] = {{copy_blocks_from_host_kernel, copy_blocks_to_host_kernel},
                                           {decode_blocks_from_host_bf16_kernel, encode_blocks_to_host_bf16_kernel},
                                           {decode_blocks_from_host_f16_kernel, encode_blocks_to_host_f16_kernel}};
  kernels[codec][to_host ? 1 : 0]<<<dim3((unsigned)grid), dim3(kCopyThreads), 0, stream>>>(
      a, static_cast<char *>(host), (unsigned)n_regions, (unsigned)region0, (unsigned)row_regions, tiles, (unsigned)block_bytes);
  return hipGetLastError();
}

// The slot-table form: the checks of the launcher above, and a slot that fits the table's 32 bits.
hipError_t launch_copy_blocks_host_slots(bool to_host, void *const *bases, int n_regions, int region0, int row_regions,
                                         const int64_t *ids, const int64_t *slots, int n, size_t block_bytes, void *host,
                                         hipStream_t stream, int codec) {
  if (n_regions <= 0 || n <= 0) return hipSuccess;
  if (n_regions > kMaxRegionsPerLaunch || n > kMaxSlotIdsPerLaunch || region0 < 0 || row_regions < region0 + n_regions ||
      block_bytes == 0 || block_bytes % 16 != 0 || block_bytes > 0x7fffffffull || reinterpret_cast<uintptr_t>(host) % 16 != 0 ||
      host_record_bytes(codec, block_bytes) == 0)
    return hipErrorInvalidValue;
  HostSlotArgs a;
  if (!copy_bases(a.base, bases, n_regions)) return hipErrorInvalidValue;
  for (int i = 0; i < n; ++i) {
    if (ids[i] < 0 || slots[i] < 0 || slots[i] > 0xffffffffll) return hipErrorInvalidValue;
    a.id[i] = ids[i];
    a.slot[i] = (uint32_t)slots[i];
  }
  const unsigned tiles = (unsigned)((block_bytes + kTile16 - 1) / kTile16);
  const size_t grid = (size_t)tiles * (size_t)n * (size_t)n_regions;
  if (grid > 0x7fffffffull) return hipErrorInvalidValue;
  // rows and columns as in launch_copy_blocks_host
  using SlotKernel = void (*)(HostSlotArgs, char *, unsigned, unsigned, unsigned, unsigned, unsigned);
  static const SlotKernel kernels[3][2] = {{copy_blocks_from_host_slots_kernel, copy_blocks_to_host_slots_kernel},
                                           {decode_blocks_from_host_slots_bf16_kernel, encode_blocks_to_host_slots_bf16_kernel},
                                           {decode_blocks_from_host_slots_f16_kernel, encode_blocks_to_host_slots_f16_kernel}};
  kernels[codec][to_host ? 1 : 0]<<<dim3((unsigned)grid), dim3(kCopyThreads), 0, stream>>>(
      a, static_cast<char *>(host), (unsigned)n_regions, (unsigned)region0, (unsigned)row_regions, tiles, (unsigned)block_bytes);
  return hipGetLastError();
}

} // namespace kvc
