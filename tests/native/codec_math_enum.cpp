// The arithmetic of the MXFP8 codec kernels (kvcached_amd/csrc/codec_math.hpp, the text the gfx950 kernels are compiled
// from) as a plain C++ shared object, so that tests/test_kv_codec.py can run it over every input on the CPU. The loops
// below put around it what codec_blocks_host_tile (kernels.hip) puts around it per group: the largest magnitude pattern,
// the finite test, the two powers of two, and the signs that travel as bits.
#include <cstddef>
#include <cstdint>

#include "codec_math.hpp"

namespace {

template <bool F16>
void encode_groups(const uint16_t *elems, size_t groups, uint8_t *codes, uint8_t *scales) {
  using H = kvc::Half16<F16>;
  for (size_t g = 0; g < groups; ++g) {
    const uint16_t *v = elems + g * 32;
    unsigned amax = 0;
    for (int j = 0; j < 32; ++j) amax = kvc::max(amax, v[j] & 0x7fffu);
    const bool finite = amax < H::kInf;
    const unsigned sb = finite ? H::scale_byte(amax) : 0xffu;
    const float down = kvc::__uint_as_float((254u - sb) << 23);
    for (int j = 0; j < 32; ++j)
      codes[g * 32 + j] = finite ? (uint8_t)(kvc::e4m3_magnitude_code(H::to_float(v[j] & 0x7fffu) * down) | ((v[j] >> 8) & 0x80u)) : 0;
    scales[g] = (uint8_t)sb;
  }
}

template <bool F16>
void decode_groups(const uint8_t *codes, const uint8_t *scales, size_t groups, uint16_t *elems) {
  using H = kvc::Half16<F16>;
  for (size_t g = 0; g < groups; ++g) {
    const unsigned sb = scales[g];
    const float up = kvc::__uint_as_float(sb ? sb << 23 : 0x00400000u);
    for (int j = 0; j < 32; ++j) {
      const unsigned c = codes[g * 32 + j];
      elems[g * 32 + j] = (uint16_t)(sb == 0xffu ? H::kQuietNan : H::from_float(kvc::e4m3_magnitude(c) * up) | ((c & 0x80u) << 8));
    }
  }
}

} // namespace

extern "C" {

void kvc_enum_encode_groups(int f16, const uint16_t *elems, size_t groups, uint8_t *codes, uint8_t *scales) {
  f16 ? encode_groups<true>(elems, groups, codes, scales) : encode_groups<false>(elems, groups, codes, scales);
}

void kvc_enum_decode_groups(int f16, const uint8_t *codes, const uint8_t *scales, size_t groups, uint16_t *elems) {
  f16 ? decode_groups<true>(codes, scales, groups, elems) : decode_groups<false>(codes, scales, groups, elems);
}
}
