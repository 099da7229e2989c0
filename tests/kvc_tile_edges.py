"""The ragged last tile of the byte movers (copy_tile and codec_blocks_host_tile, kvcached_amd/csrc/kernels.hip): the block
sizes that reach every state of its predicate, a restatement of the predicate, and the sweeps that hold a copy against numpy.

A workgroup of 4 waves copies one tile of TILE bytes (16 or 32 KiB) in pieces of 1 KiB, one piece per wave-instruction, 16
bytes per lane. Wave w's k-th piece is piece k * 4 + w of the tile (INTERLEAVED) or piece w * (TILE / 4096) + k (a contiguous
quarter). A lane copies its 16 bytes when they begin below `remain`, the bytes of the block that are left for this tile. So a
tile's behaviour depends only on `remain` (16 .. TILE in steps of 16) and on how many full tiles come before it.

The sweeps take the copy as a callable: tests/test_gpu_tile_edges.py hands in the kernels, tests/test_tile_edges.py numpy
stand-ins, a correct one (the sweeps must pass) and one that drops 16 bytes at some lengths (they must fail). Everything is
compared bit for bit; a mismatch is reported with the block size, region, block and byte offset of its first byte."""
import numpy as np
import torch

import kvc_mx_exact as X
import kvc_mx_ref as R
from test_gpu_host_offload import GUARD, _expected_image
from test_gpu_kv_codec import SCALES
from test_gpu_kv_codec import _expected_image as _coded_image

PIECE, WAVES, LANES, LANE_BYTES = 1024, 4, 64, 16
TILE16, TILE32 = 16 * 1024, 32 * 1024
FILL = 0xA5                                   # what a host buffer holds where nothing may be written
IDS = [5, 1, 3]                               # odd ids (the even neighbours are canaries), not in order
SLOTS, N_SLOTS = [6, 0, 3], 8                 # rows of the slot arena, not in order, with unused rows on every side
MOVES = ([3, 1], [0, 2])                      # compaction, per region of 4 blocks: 3 -> 0 and 1 -> 2


# ------------------------------------------------------------------ the lengths
def all_tails(tile):
    """Every `remain` a tile can have."""
    return list(range(LANE_BYTES, tile + 1, LANE_BYTES))


def edge_tails(tile):
    """Around every piece boundary: a cut at the last lane of a piece, on the boundary, at lane 0 of the next piece, at lane 33."""
    vals = {k * PIECE + d for k in range(tile // PIECE + 1) for d in (-16, 0, 16, 528)}
    return sorted(v for v in vals if LANE_BYTES <= v <= tile)


def codec_sizes():
    """The codec's blocks are whole pieces: a last tile of 1 .. 16 pieces behind 0, 1 and 2 full tiles."""
    return [PIECE * p + TILE16 * t for t in range(3) for p in range(1, 17)]


def compact_lengths():
    """Block sizes of the compaction sweep: every tail of a 32 KiB tile (for 16 KiB tiles: every tail alone and behind one
    full tile), and the edge tails behind two full 32 KiB tiles (four and five full 16 KiB tiles)."""
    return all_tails(TILE32) + [2 * TILE32 + r for r in edge_tails(TILE32)]


def host_lengths():
    """Block sizes of the raw host copies (16 KiB tiles): every tail alone, the edge tails behind one and two full tiles."""
    return all_tails(TILE16) + [t * TILE16 + r for t in (1, 2) for r in edge_tails(TILE16)]


def last_tile(tile, bb):
    """(full tiles before the last tile of a block of bb bytes, bytes in that last tile)."""
    t = (bb - 1) // tile
    return t, bb - t * tile


# ------------------------------------------------------------------ the predicate
def piece(tile, interleaved, wave, k):
    return k * WAVES + wave if interleaved else wave * (tile // PIECE // WAVES) + k


def active(tile, interleaved, remain):
    """The (wave, k, lane) triples that copy their 16 bytes in a tile with `remain` bytes left."""
    limit = min(remain, tile)
    return {(w, k, lane) for w in range(WAVES) for k in range(tile // PIECE // WAVES) for lane in range(LANES)
            if piece(tile, interleaved, w, k) * PIECE + lane * LANE_BYTES < limit}


# ------------------------------------------------------------------ reporting
def _first_difference(got, want):
    """Index of the first differing element of two flat arrays of one shape, or None."""
    step = 1 << 24
    for lo in range(0, want.size, step):
        if not np.array_equal(got[lo:lo + step], want[lo:lo + step]):
            return lo + int(np.argmax(got[lo:lo + step] != want[lo:lo + step]))
    return None


def _assert_same(got, want, where):
    """where(i) names byte i for the message."""
    assert got.shape == want.shape, (got.shape, want.shape)
    i = _first_difference(got, want)
    if i is not None:
        raise AssertionError(f"{where(i)}: got {int(got[i]):#04x}, want {int(want[i]):#04x}")


# ------------------------------------------------------------------ compaction
class CompactSweep:
    """One buffer for all the lengths: per block size a sub-range of 2 regions x 4 blocks of random bytes, and what the buffer
    must hold after (3 -> 0) and (1 -> 2) in both regions of every sub-range: each destination lies before a block that stays."""

    def __init__(self, lengths, seed=20):
        self.lengths = list(lengths)
        self.offsets = np.concatenate([[0], np.cumsum([8 * bb for bb in self.lengths])]).astype(np.int64)
        self.before = np.random.default_rng(seed).integers(0, 256, size=int(self.offsets[-1]), dtype=np.uint8)
        self.expected = numpy_compact(self.before, self.launches())
        self.expected.flags.writeable = False

    def launches(self):
        """(byte offsets of the two regions in the buffer, source blocks, destination blocks, block size) per length."""
        return [([int(off), int(off) + 4 * bb], MOVES[0], MOVES[1], bb) for bb, off in zip(self.lengths, self.offsets)]

    def where(self, i):
        j = int(np.searchsorted(self.offsets, i, side="right")) - 1
        bb, rel = self.lengths[j], i - int(self.offsets[j])
        return f"bb={bb} region={rel // (4 * bb)} block={rel % (4 * bb) // bb} byte={rel % bb}"

    def check(self, copy, label):
        """copy(before, launches) -> the buffer after all the launches; `before` itself stays."""
        got = copy(self.before, self.launches())
        _assert_same(got, self.expected, lambda i: f"{label} {self.where(i)}")


def numpy_compact(before, launches, dropped=lambda bb: 0):
    """The launches by numpy slices; dropped(bb): how many bytes at the end of every moved block are left out."""
    out = before.copy()
    for bases, src, dst, bb in launches:
        keep = bb - dropped(bb)
        for base in bases:
            for s, d in zip(src, dst):
                out[base + d * bb:base + d * bb + keep] = before[base + s * bb:base + s * bb + keep]
    return out


# ------------------------------------------------------------------ raw host copies
def _rows(slots):
    return (N_SLOTS, SLOTS) if slots else (len(IDS), list(range(len(IDS))))


def _where_host(bb, record, n_regions, n_rows):
    def where(i):
        row, rel = divmod(i, record * n_regions)
        return f"bb={bb} row={row} region={rel // record} byte={rel % record}" if row < n_rows else f"bb={bb} behind the rows, byte={i}"
    return where


def _where_region(bb, r):
    return lambda i: f"bb={bb} region={r} block={i // bb} byte={i % bb}"


def sweep_to_host(copy, regs, host, lengths, slots, label):
    """copy(bb) writes blocks IDS of the regions (regs: their bytes, numpy) to `host` (the whole pinned buffer, guard
    included): dense, rows 0 .. 2; with slots, rows SLOTS of N_SLOTS. Every other byte of `host` keeps FILL."""
    n_rows, rows = _rows(slots)
    for bb in lengths:
        row = len(regs) * bb
        assert n_rows * row + GUARD <= host.size
        host[:] = FILL
        copy(bb)
        want = np.full(host.size, FILL, dtype=np.uint8)
        want[:n_rows * row].reshape(n_rows, row)[rows] = _expected_image(regs, IDS, bb).reshape(len(IDS), row)
        _assert_same(host, want, lambda i: f"{label} {_where_host(bb, bb, len(regs), n_rows)(i)}")


def _host_image(host, pool, j, nbytes):
    """Fill the first nbytes of `host` from a window of `pool` that moves with j, the rest with 0x5A."""
    off = (j * 4099 * 16) % max(pool.size - nbytes, 1)
    host[:nbytes] = pool[off:off + nbytes] if nbytes <= pool.size else np.resize(pool, nbytes)
    host[nbytes:] = 0x5A


def sweep_from_host(copy, read_back, regs, host, lengths, slots, label):
    """copy(bb) reads blocks IDS of the regions from `host` (rows as in sweep_to_host). regs: the regions' bytes before the
    sweep; they are updated to what the regions must hold. read_back(n) -> the first n bytes of every region (None: all of
    them). Per length the first 8 blocks are compared (the targets and their neighbours), at the end the whole regions."""
    n_rows, rows = _rows(slots)
    pool = np.random.default_rng(21).integers(0, 256, size=4 << 20, dtype=np.uint8)
    for j, bb in enumerate(lengths):
        nbytes = n_rows * len(regs) * bb
        assert nbytes + GUARD <= host.size
        _host_image(host, pool, j, nbytes)
        image = host.copy()
        copy(bb)
        picked = image[:nbytes].reshape(n_rows, len(regs), bb)[rows]
        got = read_back(8 * bb)
        for r, reg in enumerate(regs):
            reg[:8 * bb].reshape(8, bb)[IDS] = picked[:, r]
            _assert_same(got[r], reg[:8 * bb], lambda i: f"{label} {_where_region(bb, r)(i)}")
        assert np.array_equal(host, image), f"{label} bb={bb}: the host image changed"
    for r, (g, reg) in enumerate(zip(read_back(None), regs)):
        _assert_same(g, reg, lambda i: f"{label} after the sweep: region={r} byte={i}")


def numpy_to_host(regs, host, slots, dropped=lambda bb: 0):
    """A stand-in for the to-host kernels over numpy regions (the regions as they are when the copy is called)."""
    n_rows, rows = _rows(slots)

    def copy(bb):
        keep = bb - dropped(bb)
        out = host[:n_rows * len(regs) * bb].reshape(n_rows, len(regs), bb)
        for i, row in zip(IDS, rows):
            for r, reg in enumerate(regs):
                out[row, r, :keep] = reg[i * bb:i * bb + keep]
    return copy


def numpy_from_host(device, host, slots, dropped=lambda bb: 0):
    """A stand-in for the from-host kernels; `device`: numpy arrays that play the regions."""
    n_rows, rows = _rows(slots)

    def copy(bb):
        keep = bb - dropped(bb)
        src = host[:n_rows * len(device) * bb].reshape(n_rows, len(device), bb)
        for i, row in zip(IDS, rows):
            for r, reg in enumerate(device):
                reg[i * bb:i * bb + keep] = src[row, r, :keep]
    return copy


def drops_16_bytes(bb):
    """The mutation: a block's last 16 bytes are left out whenever bb % 1024 is an odd multiple of 16 greater than 16. In the
    kernel: `limit - ((limit & 16u) && (limit & 1023u) > 16u ? 16u : 0u)` for `limit` in copy_tile's ragged branches."""
    return 16 if (bb & 16) and (bb & 1023) > 16 else 0


# ------------------------------------------------------------------ codec copies
def _selected(regs, bb, dt):
    """(3, regions, bb / 2) elements of blocks IDS; regs: uint8 torch tensors on the CPU."""
    return torch.stack([reg.view(dt)[:8 * (bb // 2)].view(8, bb // 2)[IDS] for reg in regs], dim=1)


def sweep_encode(copy, regs, host, sizes, dt, slots, label):
    """copy(bb) encodes blocks IDS of the regions (regs: their bytes, uint8 torch tensors on the CPU) into `host` (numpy, the
    whole buffer): the record of (block i, region r) as tests/kvc_mx_ref.py states it, in row i or, with slots, row SLOTS[i]."""
    n_rows, rows = _rows(slots)
    for bb in sizes:
        rec = R.record_bytes(bb)
        row = len(regs) * rec
        assert n_rows * row + GUARD <= host.size
        host[:] = FILL
        copy(bb)
        want = np.full(host.size, FILL, dtype=np.uint8)
        want[:n_rows * row].reshape(n_rows, row)[rows] = _coded_image(_selected(regs, bb, dt), bb).numpy().reshape(len(IDS), row)
        _assert_same(host, want, lambda i: f"{label} {_where_host(bb, rec, len(regs), n_rows)(i)}")


def sweep_decode(copy, read_back, regs, host, sizes, dt, slots, label):
    """copy(bb) decodes blocks IDS from `host`. The image: any byte as a code, scale bytes under which every product is a
    normal number and, every 7th group, 0xFF. regs (numpy, the regions before the sweep) are updated to what the regions must
    hold; a NaN code under a finite scale byte decodes to some NaN, which is taken over from what was read back."""
    n_rows, rows = _rows(slots)
    rng = np.random.default_rng(22)
    lo, hi = SCALES[dt]
    for bb in sizes:
        rec, pairs = R.record_bytes(bb), n_rows * len(regs)
        assert pairs * rec + GUARD <= host.size
        codes = rng.integers(0, 256, size=(pairs, bb // 2), dtype=np.uint8)
        scales = rng.integers(lo, hi + 1, size=(pairs, bb // 64), dtype=np.uint8)
        scales.reshape(-1)[::7] = 0xFF
        host[:pairs * rec] = np.concatenate([codes, scales], axis=1).reshape(-1)
        host[pairs * rec:] = 0x5A
        image = host.copy()
        copy(bb)
        want = X.as_bits(R.decode(torch.from_numpy(codes).reshape(-1, R.GROUP), torch.from_numpy(scales).reshape(-1), dt))
        want = want.reshape(n_rows, len(regs), bb // 2)[rows]
        loose = X.nan_code_positions(codes, scales).reshape(n_rows, len(regs), bb // 2)[rows]
        got = read_back(8 * bb)
        for r, reg in enumerate(regs):
            g, w = got[r].view(np.uint16).reshape(8, bb // 2), reg[:8 * bb].view(np.uint16).reshape(8, bb // 2)
            w[IDS] = want[:, r]
            some_nan = np.zeros((8, bb // 2), dtype=bool)
            some_nan[IDS] = loose[:, r]
            assert X.is_nan(g[some_nan], dt).all() and X.is_nan(w[some_nan], dt).all(), f"{label} bb={bb} region={r}: a NaN code"
            w[some_nan] = g[some_nan]
            _assert_same(got[r], reg[:8 * bb], lambda i: f"{label} {_where_region(bb, r)(i)}")
        assert np.array_equal(host, image), f"{label} bb={bb}: the host image changed"
    for r, (g, reg) in enumerate(zip(read_back(None), regs)):
        _assert_same(g, reg, lambda i: f"{label} after the sweep: region={r} byte={i}")


def reference_encode(regs, host, dt, slots, scale_pieces=lambda pieces: pieces):
    """A stand-in for the encode kernels: tests/kvc_mx_ref.py itself, record by record. scale_pieces(p): of a last tile of p
    pieces, how many get their scale bytes written (the kernel: lane k of a wave stores those of the wave's k-th piece)."""
    n_rows, rows = _rows(slots)

    def copy(bb):
        rec = R.record_bytes(bb)
        out = host[:n_rows * len(regs) * rec].reshape(n_rows, len(regs), rec)
        t, remain = last_tile(TILE16, bb)
        written = bb // 2 + (t * TILE16 + scale_pieces(remain // PIECE) * PIECE) // 64
        for i, row in zip(IDS, rows):
            for r, reg in enumerate(regs):
                out[row, r, :written] = R.encode_block(reg.view(dt)[i * (bb // 2):(i + 1) * (bb // 2)]).numpy()[:written]
    return copy


def reference_decode(device, host, dt, slots, pieces_decoded=lambda pieces: pieces):
    """A stand-in for the decode kernels; `device`: numpy arrays that play the regions. pieces_decoded(p): of a last tile of
    p pieces, how many are written."""
    n_rows, rows = _rows(slots)

    def copy(bb):
        rec = R.record_bytes(bb)
        src = host[:n_rows * len(device) * rec].reshape(n_rows, len(device), rec)
        t, remain = last_tile(TILE16, bb)
        keep = t * TILE16 + pieces_decoded(remain // PIECE) * PIECE
        for i, row in zip(IDS, rows):
            for r, reg in enumerate(device):
                block = X.as_bits(R.decode_block(torch.from_numpy(src[row, r].copy()), dt)).view(np.uint8)
                reg[i * bb:i * bb + keep] = block[:keep]
    return copy


def misses_a_piece(pieces):
    """The codec's mutation: a last tile whose waves do not all hold the same number of pieces loses its last piece."""
    return pieces - 1 if pieces % WAVES else pieces
