"""The MXFP8 codec of KV block offload, host side: the CPU restatement of the format (tests/kvc_mx_ref.py) is pinned by
hand-checkable anchors, its error bound and idempotence, and equals an exact float64 statement of the format
(tests/kvc_mx_exact.py) over the whole input space: every (code, scale byte) pair, the scale byte of every finite largest
magnitude, and the code of every element of both signs under every scale byte the encoder can write. The arithmetic the
kernels are compiled from (kvcached_amd/csrc/codec_math.hpp), built as plain C++, equals the restatement over the same
enumerations. NaN codes under a scale byte other than 0xFF are compared by isnan only, every other position by bit pattern.
Further: the C entries' sizes, symbols and refusals on the "cpu" device; KVCacheManager.offload(codec=...) refuses unfit
arguments with nothing changed. The kernels themselves run the same enumerations on the MI355X (tests/test_gpu_kv_codec.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import kvc_mx_exact as X
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


# ------------------------------------------------------------------ the whole input space, on the CPU
def _restated_encode(bits, dt):
    c, s = R.encode(X.as_tensor(bits, dt).reshape(-1))
    return c.numpy(), s.numpy()


def _restated_decode(codes, scales, dt):
    return X.as_bits(R.decode(torch.from_numpy(codes), torch.from_numpy(scales), dt)).reshape(-1, R.GROUP)


def _assert_decoded_alike(got, want, codes, scales, dt):
    """Bit patterns are equal, except at NaN codes under a scale byte other than 0xFF, where both are some NaN."""
    loose = X.nan_code_positions(codes, scales)
    assert X.is_nan(got[loose], dt).all() and X.is_nan(want[loose], dt).all()
    assert np.array_equal(got[~loose], want[~loose])


def test_the_exact_reference_on_hand_checked_values():
    bf, fh = torch.bfloat16, torch.float16
    assert X.value_of([0x3F80, 0xC000, 0x0001, 0x0080, 0x7F7F], bf).tolist() == [1.0, -2.0, 2.0 ** -133, 2.0 ** -126, 255 * 2.0 ** 120]
    assert X.value_of([0x3C00, 0x0001, 0x0400, 0xFBFF], fh).tolist() == [1.0, 2.0 ** -24, 2.0 ** -14, -65504.0]
    # ties go to even, subnormals are kept, what rounds to 2^(emax + 1) is infinity
    x = np.array([1.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25, 65519.9, 65520.0, -0.0, -2.0 ** -26])
    assert X.round_to(x, fh).tolist() == [0x3C00, 0x3C00, 0x3C02, 0x0000, 0x0002, 0x7BFF, 0x7C00, 0x8000, 0x8000]
    x = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 2.0 ** -134, 3 * 2.0 ** -134, 2.0 ** 128 * (1 - 2.0 ** -9), 2.0 ** -127])
    assert X.round_to(x, bf).tolist() == [0x3F80, 0x3F82, 0x0000, 0x0002, 0x7F80, 0x0040]
    assert X.shared_exponent(np.array([0.0, 448.0, 448.5, 1.0, 1.75, 1.76, 2.0 ** -140])).tolist() == [-127, 0, 1, -8, -8, -7, -127]
    x = np.array([0.0, 2.0 ** -10, 3 * 2.0 ** -10, 1.0, 1.0625, 1.1875, -432.0, 448.0, -(2.0 ** -10) * 1.01])
    assert X.nearest_code(x).tolist() == [0x00, 0x00, 0x02, 0x38, 0x38, 0x3A, 0xFE, 0x7E, 0x81]


@pytest.mark.parametrize("dt", DTYPES)
def test_restatement_equals_exact_reference_on_every_decode_pair(dt):
    """All 256 x 256 (scale byte, code) pairs: subnormal results, overflow to infinity and scale byte 0xFF included."""
    codes, scales = X.every_decode_pair()
    assert len(set(zip(np.repeat(scales, R.GROUP).tolist(), codes.reshape(-1).tolist()))) == 65536
    got, want = _restated_decode(codes, scales, dt), X.decode(codes, scales, dt)
    _assert_decoded_alike(got, want, codes, scales, dt)
    assert (got[scales == 0xFF] == R.QUIET_NAN[dt]).all()
    inf = X.inf_pattern(dt)
    mags = want[~X.nan_code_positions(codes, scales) & (scales != 0xFF)[:, None]] & 0x7FFF
    assert (mags <= inf).all() and (mags == inf).any() and (mags == 0).any()
    assert ((mags > 0) & (mags < (0x0080 if dt == torch.bfloat16 else 0x0400))).any()      # subnormal results are among them


@pytest.mark.parametrize("dt", DTYPES)
def test_restatement_equals_exact_reference_on_every_maximum(dt):
    bits = X.every_maximum(dt)
    assert len(bits) == {torch.bfloat16: 0x7F80, torch.float16: 0x7C00}[dt]
    rc, rs = _restated_encode(bits, dt)
    xc, xs = X.encode(bits, dt)
    assert np.array_equal(rs, xs) and np.array_equal(rc, xc)
    assert np.array_equal(rs, X.scale_of_every_maximum(dt))
    # the largest code of a group is at least 224 (0x76) unless the exponent is clamped; its sign is the element's
    top = (rc & 0x7F).max(1)
    assert (top[rs > 0] >= 0x76).all() and (top <= 0x7E).all()
    assert np.array_equal(rc >> 7, bits >> 15)


@pytest.mark.parametrize("dt", DTYPES)
def test_restatement_equals_exact_reference_on_every_element_under_every_scale(dt):
    scale_bytes = X.producible_scale_bytes(dt)
    assert min(scale_bytes) == 0 and max(scale_bytes) <= 254     # (0 .. 247 for bf16; 0 and 95 .. 135 for fp16)
    assert max(scale_bytes) == X.scale_of_every_maximum(dt)[-1] and scale_bytes[max(scale_bytes)] == X.inf_pattern(dt) - 1
    bits, built_for = X.every_element_under_every_scale(dt)
    for sb, rep in scale_bytes.items():                          # every pattern 0 .. rep, with both signs, under sb
        seen = np.unique(bits[built_for == sb])
        assert np.array_equal(seen, np.concatenate([np.arange(rep + 1), np.arange(rep + 1) | 0x8000]))
    rc, rs = _restated_encode(bits, dt)
    assert np.array_equal(rs, built_for)
    xc, xs = X.encode(bits, dt)
    assert np.array_equal(rs, xs) and np.array_equal(rc, xc)


@pytest.mark.parametrize("dt", DTYPES)
def test_restatement_equals_exact_reference_on_every_non_finite_pattern(dt):
    bits = X.every_non_finite(dt)
    assert len(bits) == {torch.bfloat16: 256, torch.float16: 2048}[dt]
    rc, rs = _restated_encode(bits, dt)
    xc, xs = X.encode(bits, dt)
    assert (rs == 0xFF).all() and not rc.any() and (xs == 0xFF).all() and not xc.any()
    assert (_restated_decode(rc, rs, dt) == R.QUIET_NAN[dt]).all() and (X.decode(xc, xs, dt) == R.QUIET_NAN[dt]).all()


def _compile_codec_math(csrc, out_dir):
    """tests/native/codec_math_enum.cpp against the codec_math.hpp in `csrc`, as a shared object in out_dir, by ROCm's clang++
    (it has _Float16)."""
    from kvcached_amd import build
    compiler = next((c for c in (os.path.join(build.ROCM, "llvm", "bin", "clang++"), os.path.join(build.ROCM, "bin", "amdclang++"))
                     if os.path.exists(c)), None)
    if compiler is None:
        pytest.skip("no clang++ under %s" % build.ROCM)
    so = os.path.join(str(out_dir), "libcodec_math_enum.so")
    subprocess.check_call([compiler, "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + str(csrc),
                           os.path.join(T.REPO, "tests", "native", "codec_math_enum.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    u8, u16 = np.ctypeslib.ndpointer(np.uint8, flags="C"), np.ctypeslib.ndpointer(np.uint16, flags="C")
    lib.kvc_enum_encode_groups.argtypes = [ctypes.c_int, u16, ctypes.c_size_t, u8, u8]
    lib.kvc_enum_decode_groups.argtypes = [ctypes.c_int, u8, u8, ctypes.c_size_t, u16]
    lib.kvc_enum_encode_groups.restype = lib.kvc_enum_decode_groups.restype = None
    return lib


def _native_encode(lib, bits, dt):
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    codes, scales = np.empty(bits.shape, dtype=np.uint8), np.empty(len(bits), dtype=np.uint8)
    lib.kvc_enum_encode_groups(int(dt == torch.float16), bits, len(bits), codes, scales)
    return codes, scales


def _native_decode(lib, codes, scales, dt):
    out = np.empty(codes.shape, dtype=np.uint16)
    lib.kvc_enum_decode_groups(int(dt == torch.float16), np.ascontiguousarray(codes), np.ascontiguousarray(scales), len(scales), out)
    return out


def kernel_arithmetic_differences(lib):
    """The number of positions where the compiled kernel arithmetic differs from the restatement, per enumeration."""
    counts = {}
    for dt in DTYPES:
        name = str(dt).split(".")[-1]
        codes, scales = X.every_decode_pair()
        got, want = _native_decode(lib, codes, scales, dt), _restated_decode(codes, scales, dt)
        loose = X.nan_code_positions(codes, scales)
        counts["decode " + name] = int((got[~loose] != want[~loose]).sum() + (~X.is_nan(got[loose], dt)).sum())
        for what, bits in (("maxima", X.every_maximum(dt)), ("elements", X.every_element_under_every_scale(dt)[0]),
                           ("non-finite", X.every_non_finite(dt))):
            (gc, gs), (rc, rs) = _native_encode(lib, bits, dt), _restated_encode(bits, dt)
            counts["%s %s" % (what, name)] = int((gc != rc).sum() + (gs != rs).sum())
    return counts


def test_kernel_arithmetic_compiled_for_the_cpu_equals_restatement(tmp_path):
    """codec_math.hpp, the text the gfx950 kernels are compiled from, over every decode pair, every maximum, every element
    under every scale byte and every non-finite pattern. (A perturbed constant shows: with 0x7ffffu -> 0x80000u in
    e4m3_magnitude_code the element enumerations differ at the ties, with 0x300u -> 0x2ffu in scale_byte the fp16 ones.)"""
    lib = _compile_codec_math(os.path.join(T.REPO, "kvcached_amd", "csrc"), tmp_path)
    counts = kernel_arithmetic_differences(lib)
    assert len(counts) == 8 and not any(counts.values()), counts
