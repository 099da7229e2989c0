// The arithmetic of the MXFP8 codec (encode_blocks_to_host / decode_blocks_from_host in kernels.hip; the format:
// INTEGRATION.md §6) without lane intrinsics: what one element and one group maximum go through. kernels.hip includes it
// for the device; a plain C++ compile of the same text (tests/native/codec_math_enum.cpp) lets the tests enumerate every
// input on the CPU.
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define KVC_CODEC_FN __device__ __forceinline__
#else
#include <algorithm>
#include <cstring>
#define KVC_CODEC_FN inline
namespace kvc {
using std::max;
using std::min;
inline unsigned __float_as_uint(float f) {
  unsigned u;
  std::memcpy(&u, &f, sizeof u);
  return u;
}
inline float __uint_as_float(unsigned u) {
  float f;
  std::memcpy(&f, &u, sizeof f);
  return f;
}
} // namespace kvc
#endif

namespace kvc {

// The 16-bit float types by their bit patterns. kInf: the magnitude pattern of infinity (everything above is a NaN).
template <bool F16>
struct Half16 {
  static constexpr unsigned kInf = F16 ? 0x7c00u : 0x7f80u, kQuietNan = F16 ? 0x7e00u : 0x7fc0u;
  static KVC_CODEC_FN float to_float(unsigned h) {
    if (F16) return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
    return __uint_as_float(h << 16);
  }
  static KVC_CODEC_FN unsigned from_float(float f) { // round to nearest even; subnormals of fp16 are kept
    if (F16) return __builtin_bit_cast(unsigned short, (_Float16)f);
    const unsigned b = __float_as_uint(f);
    return (b & 0x7fffffffu) > 0x7f800000u ? kQuietNan : (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
  }
  // Scale byte (shared exponent + 127) of a group whose largest magnitude has the finite pattern `amax`: with amax = m * 2^e,
  // m in [1, 2), the exponent is e - 8 for m <= 1.75 and e - 7 above, clamped to >= -127 (bf16; fp16 never gets there).
  static KVC_CODEC_FN unsigned scale_byte(unsigned amax) {
    if (F16) {
      if (amax == 0) return 0;
      unsigned e = amax >> 10, m = amax & 0x3ffu;
      if (e == 0) { // subnormal: amax = m * 2^-24; normalise
        const unsigned p = 31u - (unsigned)__builtin_clz(m);
        m = (m << (10u - p)) & 0x3ffu;
        return p + 95u + (m > 0x300u);
      }
      return e + 104u + (m > 0x300u);
    }
    const int b = (int)(amax >> 7) - 8 + ((amax & 0x7fu) > 0x60u); // (zero and the subnormals, exponent field 0, clamp to 0)
    return (unsigned)max(b, 0);
  }
};

// The signs travel as bits, beside the floating-point operations: the compiler fuses a multiplication with the conversion
// next to it (v_fma_mix*, a * b + 0), and -0 + 0 is +0.
// |x|, 0 <= |x| <= 448, to the seven low bits of its e4m3fn code, round to nearest even.
KVC_CODEC_FN unsigned e4m3_magnitude_code(float x) {
  const unsigned a = __float_as_uint(x) & 0x7fffffffu;
  if (a >= 0x3c800000u) // >= 2^-6, a normal number of e4m3: round the 23-bit mantissa to 3 bits, rebias 127 -> 7
    return min(((a + 0x7ffffu + ((a >> 20) & 1u)) >> 20) - 0x3c0u, 0x7eu);
  // a multiple of 2^-9: 2^14 + |x| has 2^-9 as its last mantissa bit, and the addition rounds to nearest even
  return __float_as_uint(__uint_as_float(a) + 16384.0f) - 0x46800000u;
}

// The magnitude of the e4m3fn code c (its sign bit is ignored).
KVC_CODEC_FN float e4m3_magnitude(unsigned c) {
  const unsigned em = c & 0x7fu;
  return em == 0x7fu ? __uint_as_float(0x7fc00000u)
         : em >= 8u  ? __uint_as_float((em << 20) + 0x3c000000u)
                     : (float)em * 0.001953125f; // subnormal: em * 2^-9
}

} // namespace kvc
