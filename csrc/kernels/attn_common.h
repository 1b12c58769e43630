// Helpers shared by the attention kernel files (attn_kernels.hip: a whole head on chip;
// attn_stream_kernels.hip: the other side of the product streamed through LDS in chunks).
#pragma once

#include "mfma.h"

namespace dpt {

namespace attn {
constexpr int D = 64;     // head dim
constexpr int RB = 128;   // LDS row bytes (64 bf16)
}  // namespace attn

// 2^x on the transcendental unit (v_exp_f32) without the denormal-range fix-up libm's exp2f adds
// (compare, scale, ldexp, select: 4 more VALU per score).  It differs only where 2^x < 2^-126,
// probabilities that vanish in the bf16 operands anyway; forward and backward use the same one,
// so the recomputed P matches the forward's.
__device__ __forceinline__ float attn_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

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
