// The number format of include/unirec_fp8.h in integer arithmetic: the row exponent, the e4m3fn rounding and the decoding.  Plain C++
// that compiles for the host and for the device, so that a host program can hold it to the rule (tests/host/catalog_fp8_layout_check.cpp);
// no convert instruction is involved, the header's rule is what runs.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define UR_FP8_FN __host__ __device__ inline
#else
#define UR_FP8_FN inline
#endif

namespace {

UR_FP8_FN uint32_t fp8_f32_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
UR_FP8_FN float fp8_bits_f32(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

// e of a row whose largest magnitude has the bits `abits` (sign clear): a = m 2^x, m in [0.5, 1); e = 9 - x if m <= 0.875, else 8 - x,
// clamped to [-64, 64]; 0 for a == 0 and for a row that is not finite.  A subnormal a has x <= -126, far past the clamp.
UR_FP8_FN int fp8_row_exponent(uint32_t abits) {
  const uint32_t ex = abits >> 23, man = abits & 0x7fffffu;
  if (abits == 0 || ex == 255) return 0;
  if (ex == 0) return 64;
  const int e = (man <= 0x600000u ? 9 : 8) - ((int)ex - 126);      // m <= 0.875 <=> the fraction of 2 m <= 0.75
  return e < -64 ? -64 : e > 64 ? 64 : e;
}
UR_FP8_FN float fp8_pow2(int e) { return fp8_bits_f32((uint32_t)(127 + e) << 23); }      // |e| <= 64

// f32 -> the nearest e4m3fn, ties to the even code.  Below 2^-6 the target is a multiple of 2^-9: adding 2^14, whose unit in the last
// place is 2^-9, rounds there to nearest even and leaves the code in the low bits.  From 2^-6 on, the exponent is rebiased (127 -> 7) and
// the 20 dropped mantissa bits are rounded by adding half a unit less one, plus the parity of the kept part; a carry runs into the
// exponent as it should.  Magnitudes from 480 on (and NaN) give the NaN code; the quantiser never produces more than 448.
UR_FP8_FN uint32_t fp8_encode(float v) {
  uint32_t u = fp8_f32_bits(v);
  const uint32_t sign = (u >> 24) & 0x80u;
  u &= 0x7fffffffu;
  uint32_t code;
  if (u >= (1087u << 20)) {
    code = 0x7fu;
  } else if (u < (121u << 23)) {
    code = fp8_f32_bits(fp8_bits_f32(u) + 16384.0f) - (141u << 23);
  } else {
    const uint32_t odd = (u >> 20) & 1u;
    code = (u - (120u << 23) + 0x7ffffu + odd) >> 20;
  }
  return code | sign;
}

// e4m3fn -> f32, exact: (e + 120) as the f32 exponent with the mantissa on top, or m 2^-9 for the subnormals (e == 0)
UR_FP8_FN float fp8_decode(uint32_t c) {
  const uint32_t em = c & 0x7fu;
  const uint32_t mag = em >= 8u ? (em << 20) + (120u << 23) : fp8_f32_bits((float)(int)em * 0x1p-9f);
  return fp8_bits_f32(mag | ((c & 0x80u) << 24));
}

}  // namespace
