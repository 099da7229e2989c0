"""The MXFP8 format of the KV block codec stated a second time, in exact float64 arithmetic on numpy
arrays, with neither torch's float8 type nor the bit tricks of the kernels, and the enumerations of the codec's whole input
space that tests/test_kv_codec.py (CPU) and tests/test_gpu_kv_codec.py (MI355X) run the restatement (tests/kvc_mx_ref.py),
the kernels' arithmetic compiled for the CPU (tests/native/codec_math_enum.cpp) and the kernels themselves over.

Every product below is a float64 times a power of two inside float64's range, so nothing here rounds except where the
format says so: the code of an element (to the nearest e4m3fn value, ties to even) and the decoded value (to the nearest
bf16 / fp16 value, ties to even, subnormals kept, overflow to infinity).

Elements travel as their 16-bit patterns (numpy uint16). A NaN code (0x7F or 0xFF) under a scale byte other than 0xFF is
never written by the encoder and decodes to a NaN of unspecified sign and payload: decode() answers the quiet NaN there and
nan_code_positions() names those positions, which every comparison takes by isnan only."""
import functools

import numpy as np
import torch

import kvc_mx_ref as R

GROUP = R.GROUP
# (bits of the significand with the hidden one, exponent of the smallest normal number, of the largest, sign-less infinity)
_FORMAT = {torch.bfloat16: (8, -126, 127, 0x7F80), torch.float16: (11, -14, 15, 0x7C00)}
E4M3_VALUES = np.array([m * 2.0 ** -9 if e == 0 else (8 + m) * 2.0 ** (e - 10)
                        for e in range(16) for m in range(8)][:0x7F])   # of the codes 0x00 .. 0x7E, ascending; 0x7E is 448
assert E4M3_VALUES[0x7E] == 448.0 and E4M3_VALUES[0x38] == 1.0 and E4M3_VALUES[1] == 2.0 ** -9


def inf_pattern(dt):
    return _FORMAT[dt][3]


def as_tensor(bits, dt):
    """uint16 patterns -> a torch tensor of dtype dt with those patterns."""
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(dt)


def as_bits(t):
    """A bf16 / fp16 tensor on the CPU -> its uint16 patterns."""
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def value_of(bits, dt):
    """The float64 values of finite 16-bit patterns, from the fields of the pattern."""
    p, emin, _, inf = _FORMAT[dt]
    bits = np.asarray(bits, dtype=np.int64)
    mag = bits & 0x7FFF
    assert (mag < inf).all()
    field, frac = mag >> (p - 1), mag & ((1 << (p - 1)) - 1)
    v = np.where(field == 0, np.ldexp(frac.astype(np.float64), emin - (p - 1)),
                 np.ldexp((frac + (1 << (p - 1))).astype(np.float64), field - 1 + emin - (p - 1)))
    return np.where(bits & 0x8000, -v, v)


def round_to(x, dt):
    """Finite float64 values -> the patterns of the nearest values of dt, ties to even."""
    p, emin, emax, inf = _FORMAT[dt]
    ax = np.abs(x)
    _, e = np.frexp(ax)                                        # ax = f * 2^e, f in [0.5, 1)
    quantum = np.maximum(e - 1, emin) - (p - 1)                # the exponent of the last place of dt at ax
    n = np.rint(np.ldexp(ax, -quantum))                        # exact scaling; rint rounds halves to even
    r = np.ldexp(n, quantum)
    _, e = np.frexp(r)                                         # (rounding may have carried into the next binade)
    normal = (r > 0) & ((e - 1) >= emin)
    field = np.where(normal, e - 1 - emin + 1, 0)
    frac = np.where(normal, np.ldexp(r, -(e - 1) + (p - 1)) - (1 << (p - 1)), np.ldexp(r, -(emin - (p - 1))))
    mag = (field.astype(np.int64) << (p - 1)) | frac.astype(np.int64)
    mag = np.where(r >= 2.0 ** (emax + 1), inf, mag)
    return (mag | np.where(np.signbit(x), 0x8000, 0)).astype(np.uint16)


def shared_exponent(amax):
    """The smallest integer se with amax * 2^-se <= 448, clamped to [-127, 127]; -127 for 0. amax: float64 >= 0."""
    _, e = np.frexp(amax)
    se = e - 12                                                # amax * 2^-(e - 12) >= 2^11 > 448: below every answer
    for _ in range(8):
        se = np.where(np.ldexp(amax, -se) <= 448.0, se, se + 1)
    assert (np.ldexp(amax, -se) <= 448.0).all() and ((np.ldexp(amax, -(se - 1)) > 448.0) | (amax == 0)).all()
    return np.clip(np.where(amax == 0, -127, se), -127, 127)


def nearest_code(x):
    """float64 values, |x| <= 448 -> their e4m3fn codes: the nearest value, ties to the even code, the sign on top."""
    ax = np.abs(x)
    assert (ax <= 448.0).all()
    hi = np.clip(np.searchsorted(E4M3_VALUES, ax, side="left"), 1, 0x7E)   # E4M3_VALUES[hi - 1] <= ax <= E4M3_VALUES[hi]
    lo = hi - 1
    middle = (E4M3_VALUES[lo] + E4M3_VALUES[hi]) / 2                       # five significant bits: exact
    code = np.where(ax < middle, lo, np.where(ax > middle, hi, np.where(lo & 1, hi, lo)))
    return (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


def encode(bits, dt):
    """uint16 patterns, size % 32 == 0 -> (codes uint8 [groups, 32], scale bytes uint8 [groups])."""
    bits = np.asarray(bits, dtype=np.uint16).reshape(-1, GROUP)
    bad = ((bits & 0x7FFF) >= inf_pattern(dt)).any(1)
    v = value_of(np.where(bad[:, None], 0, bits), dt)
    se = shared_exponent(np.abs(v).max(1))
    codes = nearest_code(np.ldexp(v, -se[:, None]))
    codes[bad] = 0
    return codes, np.where(bad, 0xFF, se + 127).astype(np.uint8)


def decode(codes, scales, dt):
    """(codes [groups, 32], scale bytes [groups]) -> uint16 patterns [groups, 32]."""
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1, GROUP)
    scales = np.asarray(scales, dtype=np.uint8).reshape(-1)
    em = codes & 0x7F
    v = np.where(codes & 0x80, -1.0, 1.0) * E4M3_VALUES[np.minimum(em, 0x7E)]
    out = round_to(np.ldexp(v, scales.astype(np.int64)[:, None] - 127), dt)
    out[(em == 0x7F) | (scales == 0xFF)[:, None]] = R.QUIET_NAN[dt]
    return out


def nan_code_positions(codes, scales):
    """[groups, 32] bool: a NaN code under a scale byte other than 0xFF (compared by isnan only)."""
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1, GROUP)
    return ((codes & 0x7F) == 0x7F) & (np.asarray(scales).reshape(-1) != 0xFF)[:, None]


def is_nan(bits, dt):
    return (np.asarray(bits) & 0x7FFF) > inf_pattern(dt)


def exact_product_class(codes, scales, dt):
    """[groups, 32] bool: the exact product code * 2^se is zero or at least the smallest normal number of dt (and the code
    is no NaN code): where the decoded value does not depend on any treatment of subnormal numbers."""
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1, GROUP)
    em = codes & 0x7F
    v = np.ldexp(E4M3_VALUES[np.minimum(em, 0x7E)], np.asarray(scales, dtype=np.int64).reshape(-1)[:, None] - 127)
    return ((v == 0) | (v >= 2.0 ** _FORMAT[dt][1])) & (em != 0x7F)


# ------------------------------------------------------------------ the enumerations
def _rotated(n_groups):
    """Per group: the slot of its marked element (rotates through all 32) and that element's sign bit (alternates, and
    changes phase every 32 groups so that every slot meets both signs)."""
    g = np.arange(n_groups)
    return g % GROUP, (((g + g // GROUP) & 1) << 15).astype(np.uint16)


def every_maximum(dt):
    """[inf_pattern, 32] patterns: group p holds the finite magnitude pattern p as its lone non-zero element."""
    n = inf_pattern(dt)
    slot, sign = _rotated(n)
    bits = np.zeros((n, GROUP), dtype=np.uint16)
    bits[np.arange(n), slot] = np.arange(n, dtype=np.uint16) | sign
    return bits


@functools.lru_cache(maxsize=None)
def scale_of_every_maximum(dt):
    """uint8 [inf_pattern]: the restatement's scale byte of a group whose largest magnitude has the pattern p."""
    return R.encode(as_tensor(every_maximum(dt), dt).reshape(-1))[1].numpy()


def producible_scale_bytes(dt):
    """{scale byte the encoder can write for a finite group: the largest magnitude pattern that gets it}."""
    s = scale_of_every_maximum(dt)
    assert (np.diff(s.astype(np.int64)) >= 0).all()
    return {int(sb): int(np.nonzero(s == sb)[0].max()) for sb in np.unique(s)}


def every_element_under(sb, rep):
    """[groups, 32] patterns whose every group holds `rep` (the largest magnitude pattern whose group gets the scale byte
    sb) once, its slot rotating and its sign alternating, and in the other 31 slots consecutive patterns, so that every
    magnitude pattern 0 .. rep appears with both signs (the last group is filled up with +0)."""
    seq = np.repeat(np.arange(rep + 1, dtype=np.uint16), 2)
    seq[1::2] |= 0x8000
    n = -(-seq.size // (GROUP - 1))
    seq = np.concatenate([seq, np.zeros(n * (GROUP - 1) - seq.size, dtype=np.uint16)]).reshape(n, GROUP - 1)
    slot, sign = _rotated(n)
    bits = np.empty((n, GROUP), dtype=np.uint16)
    rest = np.arange(GROUP)[None, :] != slot[:, None]
    bits[rest] = seq.reshape(-1)
    bits[~rest] = np.uint16(rep) | sign
    return bits


def every_element_under_every_scale(dt):
    """(patterns [groups, 32], the scale byte each group is built for [groups])."""
    parts = [(every_element_under(sb, rep), sb) for sb, rep in sorted(producible_scale_bytes(dt).items())]
    return np.concatenate([b for b, _ in parts]), np.concatenate([np.full(len(b), sb, dtype=np.uint8) for b, sb in parts])


def every_non_finite(dt, seed=0):
    """[patterns, 32]: each infinity and NaN pattern of each sign as the single bad element, its slot rotating, of a group of
    random finite patterns."""
    inf = inf_pattern(dt)
    bad = np.concatenate([np.arange(inf, 0x8000), np.arange(inf, 0x8000) | 0x8000]).astype(np.uint16)
    rng = np.random.default_rng(seed)
    bits = (rng.integers(0, inf, size=(bad.size, GROUP)) | (rng.integers(0, 2, size=(bad.size, GROUP)) << 15)).astype(np.uint16)
    bits[np.arange(bad.size), np.arange(bad.size) % GROUP] = bad
    return bits


def every_decode_pair(seed=None):
    """(codes [2048, 32], scale bytes [2048]): all 256 x 256 (scale byte, code) pairs, eight groups per scale byte. With a
    seed, the order of the groups and the order of the codes inside every group are shuffled."""
    codes = np.tile(np.arange(256, dtype=np.uint8).reshape(8, GROUP), (256, 1))
    scales = np.repeat(np.arange(256, dtype=np.uint8), 8)
    if seed is not None:
        rng = np.random.default_rng(seed)
        order = rng.permutation(len(scales))
        codes, scales = rng.permuted(codes[order], axis=1), scales[order]
    return codes, scales

