// kernels.hpp — host-side launch interface of the gfx950 kernels (kernels.hip: byte movers; index_kernels.hip:
// block id <-> token index glue).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace kvc {

// Bytes one workgroup zeroes / the alignment unit of zero_fill_pages.
static constexpr size_t kFillSlabBytes = 64 * 1024;
// Pointers (pages / regions) and moves one launch carries in its kernarg segment.
static constexpr int kMaxPtrsPerLaunch = 1024; // 8 KiB of kernarg: a whole 1024-page batch is ONE launch (no drain/ramp between 4)
static constexpr int kMaxRegionsPerLaunch = 128;
static constexpr int kMaxMovesPerLaunch = 448; // 448 x 16 B + 128 x 8 B = 8 KiB of kernarg (32 KiB / 1984 moves per launch was tried in round 3: fewer launches, but no faster on 32 KiB blocks and 8-10 % slower on 16-18 KiB blocks - every workgroup reads its three entries through the scalar cache)
static constexpr int kMaxIdsPerLaunch = 1024; // block ids one index-kernel launch carries in its kernarg (8 KiB)
static constexpr int kMaxSlotIdsPerLaunch = 768; // (block id, host slot) pairs of one slot-table host copy: 768 x (8 + 4) B + 128 x 8 B = 10 KiB of kernarg

// Zero `n` pages of `page_bytes` each (n <= kMaxPtrsPerLaunch). Asynchronous on `stream`.
// variant: 0 = default; the others are tuning variants kept for A/B runs (kFillVariants in kernels.hip is the list).
hipError_t launch_zero_fill_pages(void *const *pages, int n, size_t page_bytes, hipStream_t stream, int variant = 0);

// Copy blocks inside each region: for r < n_regions, m < n_moves:
//   bases[r] + dst[m]*block_bytes  <-  bases[r] + src[m]*block_bytes
// n_regions <= kMaxRegionsPerLaunch, n_moves <= kMaxMovesPerLaunch. variant: 0 = default; the others are tuning variants kept
// for A/B runs (kCompactVariants in kernels.hip is the list: staging, tile, nt, placement of each).
hipError_t launch_compact_blocks(void *const *bases, int n_regions, const int64_t *src, const int64_t *dst, int n_moves,
                                 size_t block_bytes, hipStream_t stream, int variant = 0);

// What a (block, region) pair of the host image holds (the KVC_CODEC_* numbers of the C ABI; 0 = the bytes themselves).
enum HostCodec { kCodecRaw = 0, kCodecMxfp8Bf16 = 1, kCodecMxfp8F16 = 2 };
// Bytes of one (block, region) record of the host image; 0 for an unknown codec or a block size the codec cannot take.
// MXFP8: one e4m3fn code per 16-bit element and one scale byte per 32 elements; whole 1 KiB pieces only (one wave-instruction
// of the tile copy), which also keeps every record and every 512 B + 16 B part of it 16-byte aligned.
inline size_t host_record_bytes(int codec, size_t block_bytes) {
  if (codec == kCodecRaw) return block_bytes;
  if ((codec != kCodecMxfp8Bf16 && codec != kCodecMxfp8F16) || block_bytes == 0 || block_bytes % 1024 != 0) return 0;
  return block_bytes / 2 + block_bytes / 64;
}

// Copy blocks between the regions and a block-major host image, to the image (to_host) or from it: for i < n, r < n_regions,
//   host + ((i * row_regions + region0 + r) * record)  <->  bases[r] + ids[i]*block_bytes
// with record = host_record_bytes(codec, block_bytes): the block's bytes, or their MXFP8 encoding (kernels.hip has the layout).
// `host` is the device address of pinned host memory, 16-byte aligned, and is only read when !to_host; n <= kMaxIdsPerLaunch,
// n_regions <= kMaxRegionsPerLaunch (the caller splits larger requests; region0 / row_regions place a slice of the regions
// inside a row of the image).
hipError_t launch_copy_blocks_host(bool to_host, void *const *bases, int n_regions, int region0, int row_regions,
                                   const int64_t *ids, int n, size_t block_bytes, void *host, hipStream_t stream,
                                   int codec = kCodecRaw);

// The same copies with a slot table: block i's row of the image is row slots[i] of a pinned arena, not row i:
//   host + ((slots[i] * row_regions + region0 + r) * record)  <->  bases[r] + ids[i]*block_bytes
// n <= kMaxSlotIdsPerLaunch, 0 <= slots[i] < 2^32 (the kernarg carries 32-bit slots; host offsets are formed in 64 bits);
// everything else as above. Two blocks on one slot race when to_host: the caller refuses that.
hipError_t launch_copy_blocks_host_slots(bool to_host, void *const *bases, int n_regions, int region0, int row_regions,
                                         const int64_t *ids, const int64_t *slots, int n, size_t block_bytes, void *host,
                                         hipStream_t stream, int codec = kCodecRaw);

// One lane: optionally store `value` to *p, then copy *p to *out_dev (the TLB self test's view of memory).
hipError_t launch_peek_poke(void *p, unsigned *out_dev, unsigned value, bool do_write, hipStream_t stream);

// ---- index_kernels.hip. Block ids come either from the host (`ids_host`, <= kMaxIdsPerLaunch, carried in the
// kernarg) or from device memory (`ids_dev` != nullptr, any count). All asynchronous on `stream`.
// out[i*tpb + j] = ids[i]*tpb + j
hipError_t launch_expand_block_ids(const int64_t *ids_host, const int64_t *ids_dev, size_t n_ids, int64_t tpb,
                                   int64_t *out, hipStream_t stream);
// token slots for requests growing pre_lens[r] -> seq_lens[r] (see the kernel); out has out_len entries
hipError_t launch_alloc_extend(const int64_t *ids_host, const int64_t *ids_dev, size_t n_ids, const int64_t *pre_lens,
                               const int64_t *seq_lens, const int64_t *last_loc, size_t bs, int64_t tpb, int64_t *out,
                               size_t out_len, hipStream_t stream);
// token slot of the one new token of every request; out has bs entries
hipError_t launch_alloc_decode(const int64_t *ids_host, const int64_t *ids_dev, size_t n_ids, const int64_t *seq_lens,
                               const int64_t *last_loc, size_t bs, int64_t tpb, int64_t *out, hipStream_t stream);
// result[0] = number of distinct blocks (or -(number of out-of-range indices)), result[1..] = ascending block ids.
// n_blocks <= kMaxUniqueBlocks: the kernels carry a block number in 32 bits (bitmap word = block >> 5, bit = block & 31).
// `bitmap` (>= ceil(n_blocks/32) zeroed words) and `header` (16 bytes {0xffffffff,0,0,0}) are left in that state.
static constexpr int64_t kMaxUniqueBlocks = 1ll << 32;
hipError_t launch_unique_block_ids(const int64_t *idx, size_t n, int64_t tpb, int64_t n_blocks, unsigned *bitmap,
                                   void *header, int64_t *result, size_t cap, hipStream_t stream);

} // namespace kvc
