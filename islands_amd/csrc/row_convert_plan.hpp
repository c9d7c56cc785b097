// Host-only definition of the row conversions (row_convert.hip): how an f32 image is narrowed to a bf16 bit
// pattern or to an e4m3 code, and which power-of-two scale a table takes from its largest magnitude.  Plain C++
// without a device header, so that tests/cpp/row_convert_dump.cpp prints it without a device; the kernels
// compile these same functions for the device (ISL_CONVERT_FN), so what the host test pins is what runs there.
// Everything is integer arithmetic on the f32 bit pattern: no rounding mode, no flush, no library call.
#pragma once

#include <cstdint>

#include "row_table_plan.hpp"

#if defined(__HIPCC__)
#define ISL_CONVERT_FN __host__ __device__ inline
#else
#define ISL_CONVERT_FN inline
#endif

namespace isl_convert {

constexpr uint32_t kAbsMask = 0x7FFFFFFFu, kInfBits = 0x7F800000u;
constexpr uint32_t kE4m3MaxCode = 0x7E;  // 448 = 1.75 * 2^8
constexpr uint32_t kElemsPerLane = 16;   // a lane of the convert kernel owns this many consecutive elements of a row

ISL_CONVERT_FN bool is_nan_bits(uint32_t b) { return (b & kAbsMask) > kInfBits; }

// round to nearest, ties to even; what rounds past the largest finite bf16 becomes infinity; a NaN keeps its
// sign and comes out quiet
ISL_CONVERT_FN uint16_t narrow_bf16(uint32_t b) {
  if (is_nan_bits(b)) return (uint16_t)((b >> 16) | 0x0040u);
  return (uint16_t)((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16);
}

// The e4m3 code of x * 2^-e (x = the float of `bits`, e in [-32, 32]): y = min(|x| * 2^-e, 448) rounded to the
// nearest e4m3 value, ties to the even code, subnormal spacing 2^-9; the sign bit of x is kept (-0.0 and what
// rounds to zero from below give 0x80); infinities saturate.  A NaN has no code: the callers refuse it first
// (it would come out as the format's NaN, 0x7F under the sign).
ISL_CONVERT_FN uint8_t narrow_e4m3(uint32_t bits, int32_t e) {
  const uint32_t sign = (bits >> 24) & 0x80u, a = bits & kAbsMask;
  if (a > kInfBits) return (uint8_t)(sign | 0x7Fu);
  const int32_t field = (int32_t)(a >> 23);
  // an f32 subnormal is below 2^-126 and e >= -32: y < 2^-94, far below half the smallest e4m3 step (2^-10)
  if (field == 0) return (uint8_t)sign;
  const int32_t ue = field - 127 - e;  // y = sig * 2^(ue - 23), sig in [2^23, 2^24)
  if (ue >= 9) return (uint8_t)(sign | kE4m3MaxCode);  // 512 and above (infinity: field 255)
  if (ue < -11) return (uint8_t)sign;                  // y < 2^-11: below half a subnormal step
  const uint32_t sig = (a & 0x007FFFFFu) | 0x00800000u;
  // q = y in units of the spacing at y: 2^(ue - 3) in the binade of a normal e4m3 value, 2^-9 below 2^-6
  const uint32_t shift = ue >= -6 ? 20u : (uint32_t)(14 - ue);  // 20 .. 25
  const uint32_t q = (sig + ((1u << (shift - 1)) - 1u) + ((sig >> shift) & 1u)) >> shift;
  // normal: q in [8, 16], and q == 16 is the first code of the next binade; subnormal: q in [0, 8], and q == 8
  // is the first normal code
  uint32_t code = ue >= -6 ? (uint32_t)(ue + 6) * 8u + q : q;
  if (code > kE4m3MaxCode) code = kE4m3MaxCode;  // 464 and above would round to 480, which is the NaN code
  return (uint8_t)(sign | code);
}

// the bits of 448 * 2^e, e in [-33, 33]
ISL_CONVERT_FN uint32_t top_bits(int32_t e) { return ((uint32_t)(127 + 8 + e) << 23) | 0x00600000u; }

// The automatic exponent: the smallest e in [-32, 32] with max|x| <= 448 * 2^e, from the bits of max|x| (sign
// clear, not a NaN).  All zeros give -32; anything above 448 * 2^32, infinity included, gives 32 and saturates.
ISL_CONVERT_FN int32_t scale_exp_for(uint32_t absmax_bits) {
  int32_t e = isl_rows::kMinScaleExp;
  while (e < isl_rows::kMaxScaleExp && absmax_bits > top_bits(e)) ++e;
  return e;
}

// chunks of kElemsPerLane elements in a row of d elements (the last one may be partial)
inline uint64_t chunks_per_row(uint64_t d) { return (d + kElemsPerLane - 1) / kElemsPerLane; }
// workgroups of `block` lanes for `items` work items, at most `cap` (the rest is a grid stride)
inline uint32_t grid_for(uint64_t items, uint32_t block, uint32_t cap) {
  const uint64_t g = (items + block - 1) / block;
  return (uint32_t)(g < 1 ? 1 : g > cap ? cap : g);
}

}  // namespace isl_convert
