"""The ragged last tile of every byte mover on a real MI355X, enumerated: each multiple of 16 a tile can be cut at, for all
twelve compact_blocks variants and the four raw host copies, and each piece count a codec tile can have, for the eight MXFP8
kernels - where the older tests (test_gpu_kernels.py, test_gpu_host_offload.py, test_gpu_host_store.py, test_gpu_kv_codec.py)
cut a tile at lane 0 or on a piece boundary only, and gave the codec 1, 2, 6 or 16 pieces. The lengths, the layout of the
buffers and the comparisons are tests/kvc_tile_edges.py's; tests/test_tile_edges.py shows without a GPU that the lengths
reach every state of the predicate and that the comparisons notice 16 missing bytes. Everything is bit for bit.

What stays sampled: the number of regions and ids per launch and the padding of the placements' grids, which the older tests
cover at their split points."""
import numpy as np
import pytest
import torch

import kvc_mx_ref as R
import kvc_tile_edges as E
from test_gpu_host_offload import DEV, PAGE, _fill, _pinned, _regions, lib  # noqa: F401
from test_gpu_host_store import _fill_floats

pytestmark = pytest.mark.gpu

FORMS = pytest.mark.parametrize("slots", [False, True], ids=["dense", "slots"])
TYPES = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


# ------------------------------------------------------------------ compact_blocks
@pytest.fixture(scope="module")
def compact_sweep():
    """The random buffer and what it must become: the same for every variant."""
    return E.CompactSweep(E.compact_lengths())


@pytest.fixture()
def capi():
    from kvcached_amd import capi as c
    c.init(DEV, PAGE, False)
    yield c
    c.set_option(c.OPT_COMPACT_VARIANT, 0)
    c.shutdown()


@pytest.mark.parametrize("variant", range(12))   # every row of kCompactVariants (kernels.hip)
def test_compact_blocks_at_every_tail(capi, compact_sweep, variant):
    """Block sizes 16 .. 32 KiB in steps of 16, and 64 KiB + every edge tail: one launch per size into its own part of one
    device buffer (2 regions x 4 blocks, 3 -> 0 and 1 -> 2), one upload, one synchronisation, one readback."""
    def copy(before, launches):
        dev = torch.from_numpy(before).to(DEV)
        base = dev.data_ptr()
        assert base % 16 == 0
        torch.cuda.synchronize()                 # the kernels run on the library's own stream
        for offsets, src, dst, bb in launches:
            capi.compact_blocks([base + o for o in offsets], src, dst, bb, sync=False)
        torch.cuda.synchronize()
        return dev.cpu().numpy()

    capi.set_option(capi.OPT_COMPACT_VARIANT, variant)
    try:
        compact_sweep.check(copy, f"variant={variant}")
    finally:
        capi.set_option(capi.OPT_COMPACT_VARIANT, 0)


# ------------------------------------------------------------------ the host copies: two regions, blocks 5, 1, 3
def _setup(lib, largest_block, largest_record):
    ops, capi = lib
    views = _regions(ops, capi, 2, 12 * largest_block)
    buf = _pinned(E.N_SLOTS * 2 * largest_record, E.FILL)         # the slot arena (the dense image is smaller), and a guard
    assert buf.data_ptr() % 16 == 0 and all(v.data_ptr() % 16 == 0 for v in views)
    return capi, views, buf


def _read_back(views):
    return lambda n: [v[:n].cpu().numpy() for v in views]


def _to_host(capi, buf, slots, codec=0):
    if slots:
        return lambda bb: capi.copy_blocks_to_host_slots(0, E.IDS, E.SLOTS, bb, codec, buf.data_ptr(), E.N_SLOTS)
    if codec:
        return lambda bb: capi.encode_blocks_to_host(0, E.IDS, bb, codec, buf.data_ptr())
    return lambda bb: capi.copy_blocks_to_host(0, E.IDS, bb, buf.data_ptr())


def _from_host(capi, buf, slots, codec=0):
    if slots:
        return lambda bb: capi.copy_blocks_from_host_slots(0, E.IDS, E.SLOTS, bb, codec, buf.data_ptr(), E.N_SLOTS)
    if codec:
        return lambda bb: capi.decode_blocks_from_host(0, E.IDS, bb, codec, buf.data_ptr())
    return lambda bb: capi.copy_blocks_from_host(0, E.IDS, bb, buf.data_ptr())


@FORMS
def test_copy_to_host_at_every_tail(lib, slots):
    """Block sizes 16 .. 16 KiB in steps of 16, and 16 KiB and 32 KiB + every edge tail: the image (dense) or rows 6, 0, 3 of
    an arena of 8 (slots) hold the blocks; every other row and the guard keep the fill byte."""
    lengths = E.host_lengths()
    capi, views, buf = _setup(lib, max(lengths), max(lengths))
    _fill(views, seed=31)
    regs = [v.cpu().numpy() for v in views]
    E.sweep_to_host(_to_host(capi, buf, slots), regs, buf.numpy(), lengths, slots, "to host")
    for v, reg in zip(views, regs):
        assert np.array_equal(v.cpu().numpy(), reg)


@FORMS
def test_copy_from_host_at_every_tail(lib, slots):
    """The same sizes: exactly blocks 5, 1 and 3 of both regions change (blocks 0 .. 7 are read back per size, the whole
    regions after the sweep)."""
    lengths = E.host_lengths()
    capi, views, buf = _setup(lib, max(lengths), max(lengths))
    _fill(views, seed=32)
    regs = [v.cpu().numpy() for v in views]
    E.sweep_from_host(_from_host(capi, buf, slots), _read_back(views), regs, buf.numpy(), lengths, slots, "from host")


@TYPES
@FORMS
def test_encode_at_every_piece_count(lib, slots, dt):
    """1 .. 16 pieces in the last tile behind 0, 1 and 2 full tiles; infinities and NaNs among the values. The records are
    tests/kvc_mx_ref.py's; with slots, the record in row SLOTS[i] is record i of the dense image."""
    sizes = E.codec_sizes()
    capi, views, buf = _setup(lib, max(sizes), R.record_bytes(max(sizes)))
    _fill_floats(views, dt, seed=33)
    regs = [v.cpu() for v in views]
    assert all(capi.codec_record_bytes(R.CODEC[dt], bb) == R.record_bytes(bb) for bb in sizes)
    E.sweep_encode(_to_host(capi, buf, slots, R.CODEC[dt]), regs, buf.numpy(), sizes, dt, slots, "encode")
    for v, reg in zip(views, regs):
        assert torch.equal(v.cpu(), reg)


@TYPES
@FORMS
def test_decode_at_every_piece_count(lib, slots, dt):
    """The same sizes: exactly blocks 5, 1 and 3 of both regions become tests/kvc_mx_ref.py's decode of their records (NaN
    codes under a finite scale byte: some NaN); their neighbours and the rest of the regions stay."""
    sizes = E.codec_sizes()
    capi, views, buf = _setup(lib, max(sizes), R.record_bytes(max(sizes)))
    _fill(views, seed=34)
    regs = [v.cpu().numpy() for v in views]
    E.sweep_decode(_from_host(capi, buf, slots, R.CODEC[dt]), _read_back(views), regs, buf.numpy(), sizes, dt, slots, "decode")
