// Helpers shared by the attention kernel files (attn_kernels.hip: a whole head on chip;
// attn_stream_kernels.hip: the other side of the product streamed through LDS in chunks).
#pragma once

#include "mfma.h"

namespace dpt {

namespace attn {
constexpr int D = 64;     // head dim
constexpr int RB = 128;   // LDS row bytes (64 16-bit elements)
}  // namespace attn

// 2^x on the transcendental unit (v_exp_f32) without the denormal-range fix-up libm's exp2f adds
// (compare, scale, ldexp, select: 4 more VALU per score).  It differs only where 2^x < 2^-126,
// probabilities that vanish in the bf16 operands anyway; forward and backward use the same one,
// so the recomputed P matches the forward's.
__device__ __forceinline__ float attn_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// acc + the dot product of two 16-byte chunks (8 elements each) of 16-bit data, in fp32
template <bool F16>
__device__ __forceinline__ float attn_dot8(const uint4& a, const uint4& g, float acc) {
  const uint32_t ua[4] = {a.x, a.y, a.z, a.w}, ug[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc = __builtin_fmaf(cunpack<F16>(ua[k], 0), cunpack<F16>(ug[k], 0), acc);
    acc = __builtin_fmaf(cunpack<F16>(ua[k], 1), cunpack<F16>(ug[k], 1), acc);
  }
  return acc;
}

// one fp32 -> 16 bits, round to nearest even (F16: v_cvt_f16_f32, overflow to +-inf, no clamp)
template <bool F16>
__device__ __forceinline__ uint16_t attn_cvt16(float f) {
  if constexpr (F16) return __builtin_bit_cast(uint16_t, (_Float16)f);
  else return __builtin_bit_cast(uint16_t, (__bf16)f);
}

// 32 queries (this lane's column) x 64 dims (registers of two accumulator tiles), times f, as
// packed pairs into one [.., 64] row: d = 32dt + 8g + 4h + 0..3 are registers 4g..4g+3
template <bool F16>
__device__ __forceinline__ void attn_store_rows(uint16_t* row, const f32x16_t (&x)[2], float f, int h) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x2_t v0 = {x[dt][4 * g] * f, x[dt][4 * g + 1] * f};
      const f32x2_t v1 = {x[dt][4 * g + 2] * f, x[dt][4 * g + 3] * f};
      uint2 pk;
      pk.x = cpack<F16>(v0);
      pk.y = cpack<F16>(v1);
      *reinterpret_cast<uint2*>(row + dt * 32 + 8 * g + 4 * h) = pk;
    }
}

// Stage rows [0, S) of a [S, ld]-strided bf16 matrix's 64-column slice into an LDS image of
// SP rows (rows >= S zero).
__device__ __forceinline__ void attn_stage(unsigned char* img, const uint16_t* src, int64_t ld, int S, int SP,
                                           int tid, int nthreads) {
  for (int c = tid; c < SP * 8; c += nthreads) {
    const int row = c >> 3, ch = c & 7;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (row < S) v = *reinterpret_cast<const uint4*>(src + (int64_t)row * ld + ch * 8);
    *reinterpret_cast<uint4*>(img + row * attn::RB + wg_slot<attn::RB>(row, ch) * 16) = v;
  }
}

}  // namespace dpt
