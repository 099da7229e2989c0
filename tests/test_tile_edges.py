"""What tests/test_gpu_tile_edges.py rests on, without a GPU: the block sizes of its sweeps reach every state of the ragged
tile's predicate (tests/kvc_tile_edges.py: active), its comparison code passes a correct copy, and it fails a copy that drops
16 bytes at lengths that no block size of the older GPU tests has."""
import numpy as np
import pytest
import torch

import kvc_mx_ref as R
import kvc_tile_edges as E
from test_gpu_host_offload import GUARD

KiB, MiB = 1 << 10, 1 << 20
# Every block size the GPU tests used for the byte movers before the sweeps (tests/test_gpu_kernels.py, test_gpu_host_offload.py,
# test_gpu_host_store.py, test_gpu_kv_codec.py).
OLD_SIZES = [16, 1040, 2064, 18432, 497664, 16 * KiB, 18 * KiB, 32 * KiB, 48 * KiB, 2 * MiB]


def _host_buffer(lengths):
    return np.empty(E.N_SLOTS * 2 * max(lengths) + GUARD, dtype=np.uint8)     # the slot arena: 8 rows x 2 regions


# ------------------------------------------------------------------ the lengths
def test_the_lengths_are_what_they_say():
    for tile in (E.TILE16, E.TILE32):
        tails = E.all_tails(tile)
        assert len(tails) == tile // 16 and tails[0] == 16 and tails[-1] == tile and all(t % 16 == 0 for t in tails)
        edges = E.edge_tails(tile)
        assert set(edges) <= set(tails) and edges == sorted(set(edges))
        assert edges[:4] == [16, 528, 1008, 1024] and edges[-3:] == [tile - 1024 + 528, tile - 16, tile]
    sizes = E.codec_sizes()
    assert len(sizes) == 48 and all(s % 1024 == 0 for s in sizes)
    assert sorted(E.last_tile(E.TILE16, s) for s in sizes) == [(t, p * KiB) for t in range(3) for p in range(1, 17)]
    assert len(E.compact_lengths()) == len(set(E.compact_lengths())) and len(E.host_lengths()) == len(set(E.host_lengths()))
    assert max(E.compact_lengths()) == 3 * E.TILE32 and max(E.host_lengths()) == 3 * E.TILE16


def _states(tile, interleaved, remains):
    """Per (wave, k): the set of active-lane counts over the given remains. active() gives the lanes; they are lanes 0 .. n - 1."""
    seen = {(w, k): set() for w in range(E.WAVES) for k in range(tile // E.PIECE // E.WAVES)}
    for remain in remains:
        lanes = {wk: [] for wk in seen}
        for w, k, lane in E.active(tile, interleaved, remain):
            lanes[(w, k)].append(lane)
        for wk, ls in lanes.items():
            assert sorted(ls) == list(range(len(ls)))
            seen[wk].add(len(ls))
    return seen


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("tile,lengths", [(E.TILE16, "compact"), (E.TILE32, "compact"), (E.TILE16, "host")])
def test_the_sweeps_reach_every_state_of_every_piece(tile, lengths, interleaved):
    """Grouped by the number of full tiles before the last one, the lengths show every (wave, k) wholly inactive, wholly
    active, cut at a lane strictly between 0 and 63, and cut at lane 0 (one lane active). One state does not exist: the piece
    that begins the tile is never wholly inactive, because a tile that exists has at least 16 bytes."""
    by_t = {}
    for bb in (E.compact_lengths() if lengths == "compact" else E.host_lengths()):
        t, remain = E.last_tile(tile, bb)
        by_t.setdefault(t, []).append(remain)
    if lengths == "host":
        assert sorted(by_t) == [0, 1, 2] and by_t[0] == E.all_tails(tile)
    else:
        assert sorted(by_t) == ([0, 1, 4, 5] if tile == E.TILE16 else [0, 2])
        assert by_t[0] == E.all_tails(tile)
        if tile == E.TILE16:
            assert by_t[1] == E.all_tails(tile)                      # every tail behind one full tile, too
    for t, remains in by_t.items():
        if t > 0 and len(remains) < tile // 16:
            assert set(remains) <= set(E.edge_tails(tile))
        for (w, k), counts in _states(tile, interleaved, remains).items():
            first = E.piece(tile, interleaved, w, k) == 0
            assert (0 in counts) != first, (t, w, k)
            assert 64 in counts and 1 in counts and any(1 < c < 64 for c in counts), (t, w, k, sorted(counts))
            if len(remains) == tile // 16 and not first:
                assert counts == set(range(65)), (t, w, k)           # the full sweep cuts every piece at every lane


def test_active_is_the_predicate_not_the_loop():
    """A few values by hand: 16 KiB tile, remain 5 KiB + 48 (piece 5 cut after lane 2)."""
    remain = 5 * KiB + 48
    a = E.active(E.TILE16, True, remain)            # wave w's k-th piece: 4k + w
    assert len(a) == remain // 16
    assert {(1, 1, 0), (1, 1, 2), (0, 1, 63)} <= a and not {(1, 1, 3), (2, 1, 0), (0, 2, 0)} & a
    b = E.active(E.TILE16, False, remain)           # wave w's k-th piece: 4w + k
    assert len(b) == remain // 16
    assert {(1, 1, 0), (1, 1, 2), (1, 0, 63), (0, 3, 63)} <= b and not {(1, 1, 3), (1, 2, 0), (2, 0, 0)} & b
    assert len(E.active(E.TILE32, True, 40 * KiB)) == E.TILE32 // 16


# ------------------------------------------------------------------ rehearsal and mutation: compaction
@pytest.fixture(scope="module")
def compact_sweep():
    return E.CompactSweep(E.compact_lengths())


def test_compaction_sweep_passes_numpy_and_sees_the_dropped_bytes(compact_sweep):
    s = compact_sweep
    assert (s.offsets % 16 == 0).all() and len(s.launches()) == len(E.compact_lengths()) == 2048 + len(E.edge_tails(E.TILE32))
    s.check(E.numpy_compact, "numpy")
    with pytest.raises(AssertionError, match=r"mutant bb=48 region=0 block=0 byte=32: got"):
        s.check(lambda before, launches: E.numpy_compact(before, launches, E.drops_16_bytes), "mutant")


def test_the_mutation_only_copies_less_and_misses_every_old_size():
    hit = [bb for bb in E.all_tails(E.TILE32) if E.drops_16_bytes(bb)]
    assert hit[:3] == [48, 80, 112] and len(hit) == 31 * 32 and all(E.drops_16_bytes(bb) in (0, 16) for bb in range(16, 4096, 16))
    assert not any(E.drops_16_bytes(bb) for bb in OLD_SIZES)
    assert not any(E.drops_16_bytes(bb) for bb in E.codec_sizes())    # whole pieces: the codec has a mutation of its own
    old = E.CompactSweep(OLD_SIZES)
    old.check(lambda before, launches: E.numpy_compact(before, launches, E.drops_16_bytes), "mutant")


# ------------------------------------------------------------------ rehearsal and mutation: raw host copies
def _numpy_regions(nbytes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=nbytes, dtype=np.uint8) for _ in range(2)]


def _read_back(device):
    return lambda n: [d[:n].copy() for d in device]


def _to_host(lengths, slots, dropped):
    regs, host = _numpy_regions(12 * max(lengths), 1), _host_buffer(lengths)
    E.sweep_to_host(E.numpy_to_host(regs, host, slots, dropped), regs, host, lengths, slots, "to host")


def _from_host(lengths, slots, dropped):
    device, host = _numpy_regions(12 * max(lengths), 2), _host_buffer(lengths)
    regs = [d.copy() for d in device]
    E.sweep_from_host(E.numpy_from_host(device, host, slots, dropped), _read_back(device), regs, host, lengths, slots, "from host")


@pytest.mark.parametrize("slots", [False, True], ids=["dense", "slots"])
@pytest.mark.parametrize("sweep", [_to_host, _from_host])
def test_host_copy_sweeps_pass_numpy_and_see_the_dropped_bytes(sweep, slots):
    sweep(E.host_lengths(), slots, lambda bb: 0)
    with pytest.raises(AssertionError, match=r"host bb=48 (row|region)=\d .*byte=32: got"):
        sweep(E.host_lengths(), slots, E.drops_16_bytes)
    sweep(OLD_SIZES, slots, E.drops_16_bytes)                        # the old matrix could not see it


# ------------------------------------------------------------------ rehearsal and mutation: codec copies
def _float_regions(nbytes, dt, seed):
    """As tests/test_gpu_host_store.py fills them: normal deviates times a per-group power of two, infinities and NaNs."""
    gen = torch.Generator().manual_seed(seed)
    regs = []
    for _ in range(2):
        groups = nbytes // 64
        k = torch.randint(-8, 8, (groups, 1), generator=gen)
        x = torch.ldexp(torch.randn(groups, 32, generator=gen), k.expand(groups, 32))
        x[::97, 5] = float("inf")
        x[::89, 7] = float("nan")
        regs.append(x.to(dt).reshape(-1).view(torch.uint8))
    return regs


@pytest.mark.parametrize("slots", [False, True], ids=["dense", "slots"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_codec_sweeps_pass_the_restatement_and_see_a_missing_piece(dt, slots):
    sizes = E.codec_sizes()
    host = np.empty(E.N_SLOTS * 2 * R.record_bytes(max(sizes)) + GUARD, dtype=np.uint8)
    regs = _float_regions(8 * max(sizes), dt, 3)
    E.sweep_encode(E.reference_encode(regs, host, dt, slots), regs, host, sizes, dt, slots, "encode")
    with pytest.raises(AssertionError, match=r"encode bb=1024 row=\d region=0 byte=512: got 0xa5"):
        E.sweep_encode(E.reference_encode(regs, host, dt, slots, E.misses_a_piece), regs, host, sizes, dt, slots, "encode")

    def decode(missing):
        device = _numpy_regions(8 * max(sizes), 4)
        mirror = [d.copy() for d in device]
        E.sweep_decode(E.reference_decode(device, host, dt, slots, missing), _read_back(device), mirror, host, sizes, dt,
                       slots, "decode")
    decode(lambda pieces: pieces)
    with pytest.raises(AssertionError, match=r"decode bb=1024 region=0"):
        decode(E.misses_a_piece)
    # 1, 2, 6 and 16 pieces in the last tile are what the older tests had: 16 passes the mutation, the others do not
    assert [p for p in (1, 2, 6, 16) if E.misses_a_piece(p) == p] == [16]
