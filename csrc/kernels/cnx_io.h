// 8-channel loads and stores of the ConvNeXt kernels (cnx_kernels.hip, grn_kernels.hip): a lane owns
// 8 consecutive channels of a row, one 16-byte vector of 16-bit values or two of fp32, widened to
// fp32 registers.  KIND is 1 (bf16) or 2 (fp16).
#pragma once

#include "common.h"

namespace dpt {

template <int KIND>
__device__ __forceinline__ float cnx_h2f(uint32_t h) {
  return KIND == 1 ? bf16_to_f32((uint16_t)h) : f16_to_f32((uint16_t)h);
}
template <int KIND>
__device__ __forceinline__ uint32_t cnx_f2h(float f) {
  return KIND == 1 ? (uint32_t)f32_to_bf16(f) : (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f);
}

// 8 consecutive values as fp32: one 16-byte load of 16-bit values, or (F32) two of fp32.
template <int KIND, bool F32>
__device__ __forceinline__ void cnx_load8(const void* base, int64_t off, float v[8]) {
  if (F32) {
    const float4* p = reinterpret_cast<const float4*>(static_cast<const float*>(base) + off);
    const float4 a = p[0], b = p[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
    const uint4 q = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(base) + off);
    const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[2 * k] = cnx_h2f<KIND>(u[k] & 0xffff);
      v[2 * k + 1] = cnx_h2f<KIND>(u[k] >> 16);
    }
  }
}
template <int KIND, bool F32>
__device__ __forceinline__ void cnx_store8(void* base, int64_t off, const float v[8]) {
  if (F32) {
    float4* p = reinterpret_cast<float4*>(static_cast<float*>(base) + off);
    p[0] = make_float4(v[0], v[1], v[2], v[3]);
    p[1] = make_float4(v[4], v[5], v[6], v[7]);
  } else {
    uint4 q;
    q.x = cnx_f2h<KIND>(v[0]) | (cnx_f2h<KIND>(v[1]) << 16);
    q.y = cnx_f2h<KIND>(v[2]) | (cnx_f2h<KIND>(v[3]) << 16);
    q.z = cnx_f2h<KIND>(v[4]) | (cnx_f2h<KIND>(v[5]) << 16);
    q.w = cnx_f2h<KIND>(v[6]) | (cnx_f2h<KIND>(v[7]) << 16);
    *reinterpret_cast<uint4*>(static_cast<uint16_t*>(base) + off) = q;
  }
}
// 8 values of a per-channel parameter of kind 0 fp32 / 1 bf16 / 2 fp16
__device__ __forceinline__ void cnx_param8(const void* p, int kind, int64_t c0, float v[8]) {
  if (kind == 0) cnx_load8<1, true>(p, c0, v);
  else if (kind == 1) cnx_load8<1, false>(p, c0, v);
  else cnx_load8<2, false>(p, c0, v);
}

}  // namespace dpt
