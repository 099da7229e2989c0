"""The MXFP8 codec of KV block offload on a real MI355X: encode_blocks_to_host / decode_blocks_from_host against the CPU
restatement of the format (tests/kvc_mx_ref.py), bit for bit, and KVCacheManager.offload(codec="mxfp8") / .restore.

Two kinds of input. The random ones (normal deviates times a per-group power of two, through every block size, region count
and id count of the copy kernels' matrix) stay inside what _assert_covered states: bf16 groups that are all zero, non-finite
or have a largest magnitude of at least 2^-100, and every fp16 group. The enumerations (tests/kvc_mx_exact.py, the ones
tests/test_kv_codec.py runs on the CPU) are the codec's whole input space: all 256 x 256 (scale byte, code) pairs through
the decoder in four layouts, and through the encoder every magnitude pattern of both signs under every scale byte the
encoder can write, every finite pattern as a group's lone non-zero element, and every infinity and NaN pattern. There
every position is compared by bit pattern, bf16 subnormals and the clamped scale byte 0 included (the library is built
with fp32 denormals kept, which is a property of its build and not of the machine), with one exception: a NaN code (0x7F or
0xFF) under a scale byte other than 0xFF is never written by the encoder and decodes to a NaN of unspecified sign and
payload, so those positions are compared by isnan only."""
import threading
import time

import numpy as np
import pytest
import torch

import kvc_mx_exact as X
import kvc_mx_ref as R
from test_gpu_host_offload import DEV, GUARD, MiB, PAGE, N_MATRIX, _ids, _manager_setup, _pinned, _regions, lib  # noqa: F401

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
SPAN = {torch.bfloat16: 40, torch.float16: 8}                 # per-group factor 2^k, k in [-SPAN, SPAN)
SCALES = {torch.bfloat16: (40, 200), torch.float16: (122, 134)}   # decode: scale bytes whose every product is a normal number
BB_MATRIX = [1024, 18 * 1024, 32 * 1024, 48 * 1024]


def _dt_id(dt):
    return str(dt).split(".")[-1]


def _floats(groups, dt, gen):
    """(groups, 32) of dtype dt on the GPU: normal deviates times a per-group power of two."""
    k = torch.randint(-SPAN[dt], SPAN[dt], (groups, 1), device=DEV, generator=gen)
    v = torch.randn(groups, R.GROUP, device=DEV, generator=gen)
    return torch.ldexp(v, k.expand_as(v)).to(dt)


def _fill_floats(views, dt, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    for v in views:
        v.view(dt).copy_(_floats(v.numel() // 64, dt, gen).reshape(-1))
    torch.cuda.synchronize()


def _assert_covered(x16):
    """Every group of x16 is inside the bit-exact claim (module docstring)."""
    g = x16.float().reshape(-1, R.GROUP)
    amax = g.abs().amax(1)
    ok = (amax == 0) | ~torch.isfinite(g).all(1)
    if x16.dtype == torch.bfloat16:
        ok |= amax >= 2.0 ** -100
    else:
        ok[:] = True
    assert ok.all()


def _selected(views, ids, bb, dt):
    """(n, R, bb / 2) elements of blocks `ids` of every region, on the CPU."""
    idx = torch.tensor(ids, device=DEV)
    rows = [v.view(dt)[:(max(ids) + 1) * (bb // 2)].view(-1, bb // 2)[idx] for v in views]
    return torch.stack(rows, dim=1).cpu()


def _expected_image(x, bb):
    """x: (n, R, bb / 2) elements -> the flat uint8 image: per (block, region) the codes, then the scale bytes."""
    pairs = x.shape[0] * x.shape[1]
    codes, scales = R.encode(x.reshape(-1))
    return torch.cat([codes.reshape(pairs, bb // 2), scales.reshape(pairs, bb // 64)], dim=1).reshape(-1)


def _sizes(n_regions, bb):
    """n of the matrix whose raw image stays under 256 MiB (as tests/test_gpu_host_offload.py sizes its cases)."""
    return [n for n in N_MATRIX if n <= 37 or n * n_regions * bb <= 256 * MiB]


def _encode_bit_for_bit(lib, n_regions, bb, dt):
    ops, capi = lib
    ns = _sizes(n_regions, bb)
    views = _regions(ops, capi, n_regions, (3 * max(ns) + 3) * bb)
    rec = capi.codec_record_bytes(R.CODEC[dt], bb)
    assert rec == R.record_bytes(bb)
    _fill_floats(views, dt, seed=bb + n_regions)
    before = [v.clone() for v in views]
    for n in ns:
        ids = _ids(n, seed=n * 7 + bb)
        x = _selected(views, ids, bb, dt)
        _assert_covered(x)
        want = _expected_image(x, bb)
        nbytes = n * n_regions * rec
        assert want.numel() == nbytes
        host = _pinned(nbytes, 0xA5)
        capi.encode_blocks_to_host(0, ids, bb, R.CODEC[dt], host.data_ptr())
        assert torch.equal(host[:nbytes], want), (n, bb, n_regions)
        assert (host[nbytes:] == 0xA5).all()
        for v, b in zip(views, before):
            assert torch.equal(v, b)


def _decode_bit_for_bit(lib, n_regions, bb, dt):
    ops, capi = lib
    ns = _sizes(n_regions, bb)
    views = _regions(ops, capi, n_regions, (3 * max(ns) + 3) * bb)
    rec = R.record_bytes(bb)
    g = torch.Generator(device=DEV).manual_seed(bb * 3 + n_regions)
    for v in views:
        v.copy_(torch.randint(0, 256, (v.numel(),), dtype=torch.uint8, device=DEV, generator=g))
    for n in ns:
        ids = _ids(n, seed=n * 5 + bb)
        pairs = n * n_regions
        rng = np.random.default_rng(n * 3 + bb)
        codes = rng.integers(0, 254, size=(pairs, bb // 2), dtype=np.uint8)
        codes = codes + (codes >= 0x7F)                             # any byte but 0x7f and 0xff (the NaN codes)
        assert not np.isin(codes, (0x7F, 0xFF)).any()
        lo, hi = SCALES[dt]
        scales = rng.integers(lo, hi + 1, size=(pairs, bb // 64), dtype=np.uint8)
        src = _pinned(pairs * rec, 0x5A)
        src.numpy()[:pairs * rec] = np.concatenate([codes, scales], axis=1).reshape(-1)
        want = R.decode(torch.from_numpy(codes).reshape(-1, R.GROUP), torch.from_numpy(scales).reshape(-1), dt)
        wf = want.float()
        assert torch.isfinite(wf).all() and (wf[wf != 0].abs() >= torch.finfo(dt).smallest_normal).all()
        _assert_covered(want)
        want = want.view(torch.uint8).reshape(n, n_regions, bb).to(DEV)
        before = [v.clone() for v in views]
        capi.decode_blocks_from_host(0, ids, bb, R.CODEC[dt], src.data_ptr())
        idx = torch.tensor(ids, device=DEV)
        for r, (v, exp) in enumerate(zip(views, before)):
            exp[:(max(ids) + 1) * bb].view(-1, bb)[idx] = want[:, r, :]   # the even-id neighbours and the rest stay
            assert torch.equal(v, exp), (n, bb, n_regions, r)
        assert (src[pairs * rec:] == 0x5A).all()


@pytest.mark.parametrize("dt", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("n_regions", [1, 2, 64])
@pytest.mark.parametrize("bb", BB_MATRIX)
def test_encode_bit_for_bit(lib, n_regions, bb, dt):
    _encode_bit_for_bit(lib, n_regions, bb, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("n_regions", [1, 2, 64])
@pytest.mark.parametrize("bb", BB_MATRIX)
def test_decode_bit_for_bit(lib, n_regions, bb, dt):
    _decode_bit_for_bit(lib, n_regions, bb, dt)


# Blocks of the contiguous layout: 2 MiB (128 tiles of 16 KiB) and 497 664 B (30 full tiles and a ragged 6 KiB one).
@pytest.mark.parametrize("dt", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("n_regions", [1, 2])
@pytest.mark.parametrize("bb", [497664, 2 * MiB])
def test_encode_blocks_of_the_contiguous_layout(lib, n_regions, bb, dt):
    _encode_bit_for_bit(lib, n_regions, bb, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("n_regions", [1, 2])
@pytest.mark.parametrize("bb", [497664, 2 * MiB])
def test_decode_blocks_of_the_contiguous_layout(lib, n_regions, bb, dt):
    _decode_bit_for_bit(lib, n_regions, bb, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=_dt_id)
def test_special_groups(lib, dt):
    """Zero groups, a NaN group, an infinite group, a group of 31 zeros and one value, the anchors of the format."""
    ops, capi = lib
    bb = 2048                                                    # 32 groups per block
    views = _regions(ops, capi, 2, 16 * bb)
    gen = torch.Generator(device=DEV).manual_seed(11)
    for v in views:
        e = v.view(dt).view(-1, R.GROUP)
        e.copy_(_floats(e.shape[0], dt, gen))
    ids = [1, 3, 6]
    for r, v in enumerate(views):
        e = v.view(dt).view(-1, bb // 2)                         # (block, element)
        e[1, :64] = 0                                            # two zero groups
        e[1, 64 + 7] = float("nan")
        e[1, 96 + 31] = float("inf")
        e[1, 128] = float("-inf")
        e[1, 160:192] = 0
        e[1, 160 + 13 + r] = -3.0e-3                             # 31 zeros and one value
        e[3, :] = 0                                              # a whole block of zeros
        e[6, 0:32] = 0
        e[6, 0] = 448.0
        e[6, 32:64] = 0
        e[6, 32:35] = torch.tensor([1.75, -1.0, 0.3], dtype=dt, device=DEV)
        e[6, 64:96] = 0
        e[6, 64:66] = torch.tensor([1.875, 1.0], dtype=dt, device=DEV)
        e[6, 96:128] = -0.0
    torch.cuda.synchronize()
    x = _selected(views, ids, bb, dt)
    _assert_covered(x)
    want = _expected_image(x, bb)
    rec = R.record_bytes(bb)
    nbytes = len(ids) * 2 * rec
    host = _pinned(nbytes, 0xA5)
    capi.encode_blocks_to_host(0, ids, bb, R.CODEC[dt], host.data_ptr())
    assert torch.equal(host[:nbytes], want) and (host[nbytes:] == 0xA5).all()
    img = host[:nbytes].view(len(ids) * 2, rec)
    assert img[0, bb // 2:bb // 2 + 6].tolist()[:5] == [0, 0, 0xFF, 0xFF, 0xFF]      # block 1, region 0: its scale bytes
    assert not img[0, 64:160].any()                                                  # zero codes in the non-finite groups
    assert not img[2].any() and not img[3].any()                                     # the block of zeros
    assert img[4, bb // 2:bb // 2 + 4].tolist() == [127, 119, 120, 0]
    assert img[4, 0].item() == 0x7E and img[4, 32:35].tolist() == [0x7E, 0xF8, 0x6A] and img[4, 64:66].tolist() == [0x77, 0x70]
    assert (img[4, 96:128] == 0x80).all()                                            # negative zeros keep their sign
    # and back, into other blocks
    back = [9, 11, 13]
    capi.decode_blocks_from_host(0, back, bb, R.CODEC[dt], host.data_ptr())
    got = _selected(views, back, bb, dt)
    codes = img[:, :bb // 2].reshape(-1, R.GROUP)
    exp = R.decode(codes, img[:, bb // 2:].reshape(-1), dt).reshape(got.shape)
    assert torch.equal(got.view(torch.int16), exp.view(torch.int16))
    nan = got.view(torch.int16)[0, 0, 64:160]
    assert (nan == R.QUIET_NAN[dt]).all()


# ------------------------------------------------------------------ the whole input space (tests/kvc_mx_exact.py)
class _Blocks:
    """Two regions of 32 KiB blocks (512 groups each: two tiles, every wave, four pieces per wave) for `groups` groups."""
    BB, REGIONS = 32 * 1024, 2

    def __init__(self, lib, groups, dt):
        self.ops, self.capi = lib
        self.dt = dt
        self.per_block = self.BB // 64 * self.REGIONS                       # groups of one id, over both regions
        self.n = -(-groups // self.per_block)
        self.views = _regions(self.ops, self.capi, self.REGIONS, (3 * self.n + 3) * self.BB)
        self.rec = R.record_bytes(self.BB)
        assert self.capi.codec_record_bytes(R.CODEC[dt], self.BB) == self.rec

    def _padded(self, a):
        """Whole blocks: the groups of `a`, then as many of them again from the start as the last block needs."""
        return np.resize(a, (self.n * self.per_block,) + a.shape[1:])

    def encode(self, bits, seed=1):
        """bits [groups, 32] -> (the patterns that were encoded, padding included, and the kernel's codes and scale bytes)."""
        bits = self._padded(bits)
        x = X.as_tensor(bits, self.dt).reshape(self.n, self.REGIONS, self.BB // 2)
        ids = _ids(self.n, seed)
        idx = torch.tensor(ids, device=DEV)
        for r, v in enumerate(self.views):
            v.view(self.dt)[:(max(ids) + 1) * (self.BB // 2)].view(-1, self.BB // 2)[idx] = x[:, r].to(DEV)
        torch.cuda.synchronize()
        assert torch.equal(_selected(self.views, ids, self.BB, self.dt).view(torch.int16), x.view(torch.int16))
        nbytes = self.n * self.REGIONS * self.rec
        host = _pinned(nbytes, 0xA5)
        self.capi.encode_blocks_to_host(0, ids, self.BB, R.CODEC[self.dt], host.data_ptr())
        assert (host[nbytes:] == 0xA5).all()
        img = host[:nbytes].numpy().reshape(-1, self.rec)
        return bits, img[:, :self.BB // 2].reshape(-1, R.GROUP).copy(), img[:, self.BB // 2:].reshape(-1).copy()

    def decode(self, codes, scales, seed=2):
        """(codes [groups, 32], scale bytes [groups]) -> (both with the padding, and the kernel's patterns [groups, 32])."""
        codes, scales = self._padded(codes), self._padded(scales)
        pairs = self.n * self.REGIONS
        src = _pinned(pairs * self.rec, 0x5A)
        src.numpy()[:pairs * self.rec] = np.concatenate([codes.reshape(pairs, -1), scales.reshape(pairs, -1)], axis=1).reshape(-1)
        ids = [i + 1 for i in _ids(self.n, seed)]                           # even ids: not the blocks encode() reads
        self.capi.decode_blocks_from_host(0, ids, self.BB, R.CODEC[self.dt], src.data_ptr())
        torch.cuda.synchronize()
        assert (src[pairs * self.rec:] == 0x5A).all()
        return codes, scales, X.as_bits(_selected(self.views, ids, self.BB, self.dt)).reshape(-1, R.GROUP)


def _restated_encode(bits, dt):
    c, s = R.encode(X.as_tensor(bits, dt).reshape(-1))
    return c.numpy(), s.numpy()


def _differences(got, want):
    """For an assertion's message: how many positions differ, and the first few as (position, got, want)."""
    at = np.argwhere(got != want)
    return len(at), [(tuple(int(i) for i in a), hex(int(got[tuple(a)])), hex(int(want[tuple(a)]))) for a in at[:8]]


def _assert_encoded_like_the_restatement(blocks, bits, built_for=None):
    bits, codes, scales = blocks.encode(bits)
    want_codes, want_scales = _restated_encode(bits, blocks.dt)
    if built_for is not None:
        assert np.array_equal(want_scales, blocks._padded(built_for))
    assert np.array_equal(scales, want_scales), _differences(scales, want_scales)
    assert np.array_equal(codes, want_codes), _differences(codes, want_codes)
    return bits, codes, scales


@pytest.mark.parametrize("dt", DTYPES, ids=_dt_id)
def test_decode_every_pair(lib, dt):
    """All 256 x 256 (scale byte, code) pairs, in natural order and in three shuffles of the groups and of the codes inside
    them, so that every pair meets different lanes, quads, pieces and waves. fp16 subnormal results (rounded by the
    conversion instruction), overflow to infinity, bf16 subnormal results, the denormal multiplier of scale byte 0 and
    the negative zeros (code 0x80) under every scale byte are all among them."""
    layouts = [X.every_decode_pair(seed) for seed in (None, 1, 2, 3)]
    codes, scales = np.concatenate([c for c, _ in layouts]), np.concatenate([s for _, s in layouts])
    blocks = _Blocks(lib, len(scales), dt)
    assert blocks.n * blocks.per_block == len(scales) == 4 * 2048           # no padding: each pair exactly four times
    codes, scales, got = blocks.decode(codes, scales)
    want = X.as_bits(R.decode(torch.from_numpy(codes), torch.from_numpy(scales), dt)).reshape(-1, R.GROUP)
    loose = X.nan_code_positions(codes, scales)                             # NaN codes under a finite scale byte: some NaN
    assert loose.sum() == 4 * 2 * 255
    assert X.is_nan(got[loose], dt).all() and X.is_nan(want[loose], dt).all()
    got, want = np.where(loose, 0, got), np.where(loose, 0, want)
    # first the positions that no treatment of subnormal numbers can touch, then all of them
    plain = X.exact_product_class(codes, scales, dt) & (scales != 0)[:, None] if dt == torch.bfloat16 else ~loose
    assert np.array_equal(got[plain], want[plain]), _differences(np.where(plain, got, 0), np.where(plain, want, 0))
    assert np.array_equal(got, want), _differences(got, want)
    assert (got[(codes == 0x80) & (scales != 0xFF)[:, None]] == 0x8000).all()


@pytest.mark.parametrize("dt", DTYPES, ids=_dt_id)
def test_encode_every_element_under_every_scale(lib, dt):
    """Per scale byte sb the encoder can write: groups that hold the largest magnitude pattern that gets sb once, in a
    rotating slot with alternating sign, and otherwise every smaller pattern with both signs. The whole image - codes
    and scale bytes - is the restatement's (for bf16 that includes the groups below 2^-100 and subnormal elements)."""
    bits, built_for = X.every_element_under_every_scale(dt)
    blocks = _Blocks(lib, len(bits), dt)
    _assert_encoded_like_the_restatement(blocks, bits, built_for)


@pytest.mark.parametrize("dt", DTYPES, ids=_dt_id)
def test_encode_every_maximum(lib, dt):
    """Every finite magnitude pattern as the lone non-zero element of a group: the scale byte and the one code."""
    bits = X.every_maximum(dt)
    blocks = _Blocks(lib, len(bits), dt)
    bits, codes, scales = _assert_encoded_like_the_restatement(blocks, bits)
    n = X.inf_pattern(dt)
    assert np.array_equal(scales[:n], X.scale_of_every_maximum(dt)) and (np.count_nonzero(codes[:n] & 0x7F, axis=1)[1:] == 1).all()


@pytest.mark.parametrize("dt", DTYPES, ids=_dt_id)
def test_encode_every_non_finite_pattern(lib, dt):
    """Every infinity and NaN pattern of both signs as the one bad element of a random finite group: scale byte 0xFF and 32
    zero codes, which decode to 32 canonical quiet NaNs."""
    bits = X.every_non_finite(dt)
    assert len(bits) == {torch.bfloat16: 256, torch.float16: 2048}[dt]
    blocks = _Blocks(lib, len(bits), dt)
    bits, codes, scales = _assert_encoded_like_the_restatement(blocks, bits)
    assert (scales == 0xFF).all() and not codes.any()
    _, _, back = blocks.decode(codes, scales)
    assert (back == R.QUIET_NAN[dt]).all()


def test_refusals_launch_and_write_nothing(lib):
    ops, capi = lib
    bb = 32 * 1024
    rec = R.record_bytes(bb)
    ops.init_kvcached(DEV, PAGE, False)
    ts = ops.create_kv_tensors(8 * PAGE, 1, DEV, 2, 2, 0, False)
    assert ops.map_to_kv_tensors([0, PAGE, 3 * PAGE])          # page 2 of each half stays unbacked
    for t in ts:
        u = t.view(torch.uint8)
        half = u.numel() // 2
        for h in range(2):
            for p in (0, 1, 3):
                u[h * half + p * PAGE:h * half + (p + 1) * PAGE] = 0x11
    torch.cuda.synchronize()
    bpp = PAGE // bb
    host = _pinned(4 * 4 * bb, 0xC3)
    enc, dec = capi.lib.kvc_encode_blocks_to_host, capi.lib.kvc_decode_blocks_from_host
    ids = capi.i64_array([1, bpp + 5, 2 * bpp + 7, 3 * bpp])  # the third lies on an unbacked slot
    ok = capi.i64_array([1, bpp + 5, 3 * bpp])
    for fn in (enc, dec):
        for codec in (1, 2):
            assert fn(0, ids, 4, bb, codec, host.data_ptr(), None, 1) == capi.KVC_E_INVALID
            assert "not backed" in capi.last_error()
            assert fn(0, ok, 3, bb, codec, host.data_ptr() + 8, None, 1) == capi.KVC_E_INVALID      # misaligned
            assert fn(0, capi.i64_array([4 * bpp]), 1, bb, codec, host.data_ptr(), None, 1) == capi.KVC_E_INVALID
            assert fn(0, capi.i64_array([-1]), 1, bb, codec, host.data_ptr(), None, 1) == capi.KVC_E_INVALID
            for unfit in (0, 16, 2064, bb + 512):
                assert fn(0, ok, 3, unfit, codec, host.data_ptr(), None, 1) == capi.KVC_E_INVALID, unfit
        for codec in (0, 3, -1):
            assert fn(0, ok, 3, bb, codec, host.data_ptr(), None, 1) == capi.KVC_E_INVALID
            assert "codec" in capi.last_error()
    assert dec(0, capi.i64_array([1, 1]), 2, bb, 1, host.data_ptr(), None, 1) == capi.KVC_E_INVALID   # the writes would race
    assert "duplicate" in capi.last_error()
    pageable = np.full(4 * 4 * bb, 0x3C, dtype=np.uint8)
    for fn in (enc, dec):
        assert fn(0, ok, 3, bb, 1, pageable.ctypes.data, None, 1) == capi.KVC_E_INVALID
        assert "pinned" in capi.last_error()
    torch.cuda.synchronize()
    assert (pageable == 0x3C).all() and (host.numpy() == 0xC3).all()
    for t in ts:
        u = t.view(torch.uint8)
        half = u.numel() // 2
        for h in range(2):
            for p in (0, 1, 3):
                assert (u[h * half + p * PAGE:h * half + (p + 1) * PAGE] == 0x11).all()
    # the same ids without the unbacked one pass, in both directions; a duplicate id is fine when only reading
    assert enc(0, ok, 3, bb, 1, host.data_ptr(), None, 1) == capi.KVC_OK
    assert (host[:3 * 4 * rec] != 0xC3).any() and (host[3 * 4 * rec:] == 0xC3).all()
    assert dec(0, ok, 3, bb, 1, host.data_ptr(), None, 1) == capi.KVC_OK
    assert enc(0, capi.i64_array([1, 1]), 2, bb, 2, host.data_ptr(), None, 1) == capi.KVC_OK
    del ts


# ------------------------------------------------------------------ manager level
def _stamp_floats(views, ids, dt, seed):
    """Float data into blocks `ids` of every region; returns the (n, bmem / 2) elements per region, on the GPU."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    idx = torch.tensor(ids, device=DEV)
    data = []
    for v in views:
        x = _floats(len(ids) * v.shape[1] // 64, dt, gen).reshape(len(ids), -1)
        v[idx] = x.view(torch.uint8)
        data.append(x)
    return data


def _round_trip_of(x):
    """decode(encode(x)) by the restatement, after checking that x is inside the bit-exact claim and that the result
    is within max(|x| * 2^-4, 2^(se - 10)) of x."""
    xc = x.cpu()
    _assert_covered(xc)
    c, s = R.encode(xc.reshape(-1))
    y = R.decode(c, s, xc.dtype)
    se = R.shared_exponents(s)[:, None].expand(-1, R.GROUP).reshape(-1)
    xd, yd = xc.reshape(-1).double(), y.double()
    assert ((xd - yd).abs() <= torch.maximum(xd.abs() * 2.0 ** -4, torch.ldexp(torch.ones_like(xd), se - 10))).all()
    return y.reshape(xc.shape)


def _holds_exactly(views, ids, want):
    idx = torch.tensor(ids, device=DEV)
    return all(torch.equal(v[idx].cpu(), w.contiguous().view(torch.uint8).cpu()) for v, w in zip(views, want))


@pytest.mark.parametrize("dt", DTYPES, ids=_dt_id)
@pytest.mark.parametrize("layout", ["per_layer", "contiguous", "mla"])
def test_offload_and_restore_through_the_codec(lib, monkeypatch, layout, dt):
    ops, capi = lib
    m, views = _manager_setup(ops, monkeypatch, layout)
    bpp = views[0].shape[0] // 16
    ids = m.alloc(bpp * 6)
    live = ids[bpp:3 * bpp] + ids[4 * bpp:4 * bpp + 9] + ids[5 * bpp + 3:5 * bpp + 40]
    kept = [b for b in ids if b not in set(live)]
    x_kept = _stamp_floats(views, kept, dt, seed=1)
    x = _stamp_floats(views, live, dt, seed=2)
    torch.cuda.synchronize()
    y = [_round_trip_of(xr) for xr in x]
    inuse = m.page_allocator.get_num_inuse_pages()
    h = m.offload(live, codec="mxfp8", dtype=dt)                 # two whole pages among them
    assert (h.block_ids, h.codec, h.dtype) == (live, "mxfp8", dt) and len(h.geometry) == 4
    assert m.page_allocator.get_num_inuse_pages() == inuse - 2
    bases, bb = m._block_geometry()
    assert h.data.is_pinned() and h.data.numel() == len(live) * len(bases) * R.record_bytes(bb)
    with pytest.raises(ValueError):
        m._check_live_blocks(live[:1])                           # freed
    rest = m.alloc(m.available_size())                           # the freed blocks are handed out again and scribbled over
    for v in views:
        v[torch.tensor(rest, device=DEV)] = 0xEE
    torch.cuda.synchronize()
    assert m.restore(h) is None                                  # the pool is full: nothing happens
    m.free(rest)
    new = m.restore(h)
    assert new is not None and len(new) == len(live)
    m._check_live_blocks(new)
    torch.cuda.synchronize()
    assert _holds_exactly(views, new, y)
    again = m.restore(h)                                         # a second restore is a second, independent copy
    assert again is not None and not set(again) & set(new)
    torch.cuda.synchronize()
    assert _holds_exactly(views, again, y) and _holds_exactly(views, new, y)
    assert _holds_exactly(views, kept, x_kept)
    h.release()
    assert h.data is None
    # a caller's own buffer of exactly the coded size
    out = torch.empty(len(new) * len(bases) * R.record_bytes(bb), dtype=torch.uint8, pin_memory=True)
    h2 = m.offload(new, out=out, codec="mxfp8", dtype=dt)
    assert h2.data.data_ptr() == out.data_ptr()
    new2 = m.restore(h2)
    torch.cuda.synchronize()
    assert _holds_exactly(views, new2, y)                        # idempotent: already-coded data goes through unchanged


def test_raw_and_coded_handles_in_one_session(lib, monkeypatch):
    ops, capi = lib
    dt = torch.bfloat16
    m, views = _manager_setup(ops, monkeypatch, "per_layer")
    bpp = views[0].shape[0] // 16
    ids = m.alloc(bpp + 21)
    x = _stamp_floats(views, ids, dt, seed=5)
    torch.cuda.synchronize()
    y = [_round_trip_of(xr) for xr in x]
    raw = m.offload(ids)
    assert raw.codec is None and raw.dtype is None
    a = m.restore(raw)
    coded = m.offload(a, codec="mxfp8", dtype=dt)
    assert coded.data.numel() * 64 == raw.data.numel() * 33
    b = m.restore(coded)
    c = m.restore(raw)
    d = m.restore(coded)
    torch.cuda.synchronize()
    assert len(set(b) | set(c) | set(d)) == 3 * len(ids)
    assert _holds_exactly(views, c, x)
    assert _holds_exactly(views, b, y) and _holds_exactly(views, d, y)


def test_coded_round_trips_next_to_background_mapping(lib, monkeypatch):
    """Prealloc thread on, a second thread allocating and freeing other blocks in a loop: every coded round trip gives
    decode(encode(x)) exactly."""
    ops, capi = lib
    dt = torch.float16
    m, views = _manager_setup(ops, monkeypatch, "per_layer", n_pages=32, layers=4, prealloc=True, async_sched=True)
    bpp = views[0].shape[0] // 32
    stop = threading.Event()
    errors = []

    def churn():
        rng = np.random.default_rng(1)
        try:
            while not stop.is_set():
                got = m.alloc(int(rng.integers(1, 3 * bpp)))
                time.sleep(0.001)
                if got:
                    m.free(got)
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)

    t = threading.Thread(target=churn, daemon=True)
    t.start()
    rounds = 0
    try:
        t0 = time.time()
        while time.time() - t0 < 3.0:
            ids = m.alloc(bpp + 17)
            assert ids is not None
            x = _stamp_floats(views, ids, dt, seed=rounds)
            h = m.offload(ids, codec="mxfp8", dtype=dt)
            new = m.restore(h)
            assert new is not None
            torch.cuda.synchronize()
            assert _holds_exactly(views, new, [_round_trip_of(xr) for xr in x]), rounds
            m.free(new)
            rounds += 1
    finally:
        stop.set()
        t.join(10)
    assert not errors and rounds > 3
