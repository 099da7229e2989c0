"""The MXFP8 codec of KV block offload, host side: the CPU restatement of the format (tests/kvc_mx_ref.py) is pinned by
hand-checkable anchors, its error bound and idempotence; the C entries' sizes, symbols and refusals on the "cpu" device;
KVCacheManager.offload(codec=...) refuses unfit arguments with nothing changed. The kernels are compared with the
restatement, bit for bit, on the MI355X (tests/test_gpu_kv_codec.py)."""
import ctypes
import re

import pytest
import torch

import kvc_mx_ref as R
import kvc_testlib as T
from test_host_offload import BPP, PAGE, _manager, _state, cpu_ops  # noqa: F401  (cpu_ops is a fixture)

DTYPES = [torch.bfloat16, torch.float16]


def seeded_input(dt, n=1 << 20, seed=0):
    """Normal deviates times a per-group factor 2^k, k uniform in [-40, 40) for bf16 and [-8, 8) for fp16."""
    g = torch.Generator().manual_seed(seed + (0 if dt == torch.bfloat16 else 1))
    span = 40 if dt == torch.bfloat16 else 8
    k = torch.randint(-span, span, (n // R.GROUP, 1), generator=g)
    v = torch.randn(n // R.GROUP, R.GROUP, generator=g)
    return torch.ldexp(v, k.expand_as(v)).to(dt).reshape(-1)


def _group(values, dt):
    v = torch.zeros(R.GROUP)
    v[:len(values)] = torch.tensor(values)
    return v.to(dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_anchors(dt):
    for values, scale, codes, decoded in (([1.0], 119, [0x78], [1.0]),
                                          ([448.0], 127, [0x7E], [448.0]),
                                          ([1.75, -1.0, 0.3], 119, [0x7E, 0xF8, 0x6A], [1.75, -1.0, 0.3125]),
                                          ([1.875, 1.0], 120, [0x77, 0x70], [1.875, 1.0])):
        c, s = R.encode(_group(values, dt))
        assert s.tolist() == [scale], values
        assert c[0, :len(values)].tolist() == codes and not c[0, len(values):].any(), values
        assert R.decode(c, s, dt)[:len(values)].tolist() == decoded, values
    # an all-zero group: the smallest exponent, zero codes
    c, s = R.encode(torch.zeros(R.GROUP, dtype=dt))
    assert s.tolist() == [0] and not c.any() and not R.decode(c, s, dt).any()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_group_becomes_quiet_nans(dt, bad):
    v = torch.ones(3 * R.GROUP, dtype=dt)
    v[R.GROUP + 5] = bad
    c, s = R.encode(v)
    assert s.tolist() == [119, 0xFF, 119] and not c[1].any() and (c[0] == 0x78).all()
    out = R.decode(c, s, dt).view(torch.int16).reshape(3, R.GROUP)
    assert (out[1] == R.QUIET_NAN[dt]).all() and torch.equal(out[0].view(dt), v[:R.GROUP])


@pytest.mark.parametrize("dt", DTYPES)
def test_error_bound_and_idempotence(dt):
    x = seeded_input(dt)
    c, s = R.encode(x)
    y = R.decode(c, s, dt)
    se = R.shared_exponents(s)[:, None].expand(-1, R.GROUP).reshape(-1)
    xd, yd = x.double(), y.double()
    bound = torch.maximum(xd.abs() * 2.0 ** -4, torch.ldexp(torch.ones_like(xd), se - 10))
    assert ((xd - yd).abs() <= bound).all()
    # the shared exponent is the smallest one that avoids saturation: the largest code of every group is at least 224 (0x76)
    assert ((c & 0x7F).amax(1) >= 0x76).all() and ((c & 0x7F) != 0x7F).all()
    nz = xd != 0
    rms = (((xd - yd)[nz] / xd[nz]) ** 2).mean().sqrt().item()
    assert 0.02 < rms < 0.035, rms                           # (0.027 on these inputs)
    # idempotent: what came out of the codec goes through it unchanged (the codes themselves may differ: a group maximum
    # that was rounded down to 1.75 * 2^e takes the next smaller exponent, and every code of the group doubles exactly)
    c2, s2 = R.encode(y)
    assert torch.equal(R.decode(c2, s2, dt).view(torch.int16), y.view(torch.int16))


def test_record_layout_of_the_restatement():
    x = seeded_input(torch.bfloat16, n=1024)                 # 2048 bytes: one record of 1024 + 32 bytes
    rec = R.encode_block(x)
    assert rec.numel() == R.record_bytes(2048) == 1056
    c, s = R.encode(x)
    assert torch.equal(rec[:1024], c.reshape(-1)) and torch.equal(rec[1024:], s)
    assert torch.equal(R.decode_block(rec, torch.bfloat16).view(torch.int16), R.decode(c, s, torch.bfloat16).view(torch.int16))


def test_codec_record_bytes():
    from kvcached_amd import capi
    f = capi.lib.kvc_codec_record_bytes
    assert f(1, 32768) == 16896 and f(2, 1024) == 528
    for bb in (16 * 1024, 18 * 1024, 32 * 1024, 48 * 1024, 497664, 2 << 20):
        assert f(1, bb) == f(2, bb) == capi.codec_record_bytes(1, bb) == R.record_bytes(bb) and f(1, bb) % 16 == 0
    for codec, bb in ((0, 32768), (3, 32768), (-1, 32768), (1, 16), (1, 2064), (2, 16), (2, 2064), (1, 0)):
        assert f(codec, bb) == 0, (codec, bb)


def test_header_symbols_and_capi_table_agree():
    from kvcached_amd import capi
    import os
    src = open(os.path.join(T.REPO, "include", "kvcached_amd.h")).read()
    m = re.search(r"enum\s*\{\s*KVC_CODEC_MXFP8_BF16\s*=\s*(\d+)\s*,\s*KVC_CODEC_MXFP8_F16\s*=\s*(\d+)\s*\}", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (capi.KVC_CODEC_MXFP8_BF16, capi.KVC_CODEC_MXFP8_F16) == (1, 2)
    assert R.CODEC == {torch.bfloat16: 1, torch.float16: 2}
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("kvc_codec_record_bytes", "kvc_encode_blocks_to_host", "kvc_decode_blocks_from_host"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in capi.SIGNATURES and hasattr(capi.lib, name)
    assert len(capi.SIGNATURES["kvc_encode_blocks_to_host"][1]) == len(capi.SIGNATURES["kvc_decode_blocks_from_host"][1]) == 8
    assert capi.lib.kvc_abi_version() == 5                   # additions only


def test_c_entries_refuse_the_cpu_device(cpu_ops):
    ops, capi = cpu_ops
    ops.create_kv_tensors(16 * PAGE * 2, 1, "cpu", 2, 2, 0, False)
    buf = (ctypes.c_char * (1 << 16))()
    ids = capi.i64_array([0, 1])
    for codec in (1, 2):
        assert capi.lib.kvc_encode_blocks_to_host(0, ids, 2, 1024, codec, ctypes.addressof(buf), None, 1) == capi.KVC_E_NO_GPU
        assert capi.lib.kvc_decode_blocks_from_host(0, ids, 2, 1024, codec, ctypes.addressof(buf), None, 1) == capi.KVC_E_NO_GPU
    with pytest.raises(capi.KvcError) as e:
        capi.encode_blocks_to_host(0, [0], 1024, 1, ctypes.addressof(buf))
    assert e.value.code == capi.KVC_E_NO_GPU
    with pytest.raises(capi.KvcError) as e:
        capi.decode_blocks_from_host(0, [0], 1024, 2, ctypes.addressof(buf))
    assert e.value.code == capi.KVC_E_NO_GPU
    assert not any(bytes(buf))


def test_offload_with_a_codec_refuses_unfit_arguments(cpu_ops):
    ops, capi = cpu_ops
    m = _manager(ops)
    ids = m.alloc(2 * BPP)
    before = _state(m)
    bases, bb = m._block_geometry()
    rec = R.record_bytes(bb)
    for kw in (dict(codec="mxfp4", dtype=torch.bfloat16),             # unknown codec
               dict(codec="mxfp8"),                                   # no dtype
               dict(codec="mxfp8", dtype=torch.float32),              # unfit dtypes
               dict(codec="mxfp8", dtype=torch.uint8),
               dict(codec="mxfp8", dtype="bfloat16"),
               dict(dtype=torch.bfloat16),                            # a dtype without a codec
               dict(codec="mxfp8", dtype=torch.float16,               # one byte short
                    out=torch.empty(4 * len(bases) * rec - 1, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            m.offload(ids[:4], **kw)
        assert _state(m) == before, kw
    # everything fits: the copy itself fails (no GPU) and every block stays allocated
    with pytest.raises(capi.KvcError) as e:
        m.offload(ids[:4], codec="mxfp8", dtype=torch.bfloat16)
    assert e.value.code == capi.KVC_E_NO_GPU and _state(m) == before
    m.free(ids)
    assert m.page_allocator.get_num_inuse_pages() == 0


def test_offload_with_a_codec_refuses_unfit_block_bytes(cpu_ops):
    """16 tokens x 32 bytes = 512-byte blocks: not whole 1 KiB pieces."""
    ops, capi = cpu_ops
    import kvcached_amd.kv_cache_manager as kcm
    ops.create_kv_tensors(16 * PAGE * 2, 1, "cpu", 2, 2, 0, False)
    m = kcm.KVCacheManager(num_blocks=16 * 4096, block_size=16, cell_size=32, num_layers=2)
    assert m._post_init_done.wait(10)
    ids = m.alloc(8)
    assert ids is not None and m._block_geometry()[1] == 512
    before = _state(m)
    with pytest.raises(ValueError, match="1024"):
        m.offload(ids[:2], codec="mxfp8", dtype=torch.float16)
    assert _state(m) == before
    m.free(ids)


def test_handles_keep_their_three_argument_constructor(cpu_ops):
    ops, capi = cpu_ops
    import kvcached_amd.kv_cache_manager as kcm
    m = _manager(ops)
    bases, bb = m._block_geometry()
    h = kcm.OffloadedBlocks([3, 4], torch.zeros(2 * 4 * bb, dtype=torch.uint8), (0, False, 4, bb))
    assert h.codec is None and h.dtype is None and len(h.geometry) == 4
    coded = kcm.OffloadedBlocks([3, 4], torch.zeros(2 * 4 * R.record_bytes(bb), dtype=torch.uint8), (0, False, 4, bb),
                                codec="mxfp8", dtype=torch.bfloat16)
    before = _state(m)
    with pytest.raises(capi.KvcError) as e:                  # reaches the decoder, which refuses the device
        m.restore(coded)
    assert e.value.code == capi.KVC_E_NO_GPU and _state(m)[0] == before[0]
    broken = kcm.OffloadedBlocks([3], torch.zeros(4 * bb, dtype=torch.uint8), (0, False, 4, bb), codec="zip", dtype=None)
    with pytest.raises(ValueError):
        m.restore(broken)
    assert _state(m)[0] == before[0]
