// 8-element vector I/O for the three activation dtypes of the fused BatchNorm kernels
// (bn_kernels.hip) - shared with the kernels that redo the BN apply arithmetic bit for bit
// (tail_conv1_kernels.hip, tail_conv3_bwd_kernels.hip).
#pragma once

#include "common.h"

namespace dpt {

// The backward apply's dx = k1*dz + k2*(x - mean) + k3 with its contraction written out (the product
// k2*(x - mean) rounded, k1*dz fused onto it, k3 added: what the compiler made of the plain
// expression): bn_bwd_apply_kernel, bn_bwd_apply2_kernel and tail_conv3_bwd_kernel all call this, so
// their bits agree by construction and not by what a compiler version happens to fuse.
__device__ __forceinline__ float bn_bwd_dx(float k1, float dz, float k2, float x, float mean, float k3) {
  return __builtin_fmaf(k1, dz, k2 * (x - mean)) + k3;
}

// ---- 8-element vector I/O for the three activation dtypes ----------------------------------
struct BF16 {
  using raw = uint16_t;
  __device__ static void load8(const void* p, int64_t i, float f[8]) {
    uint4 w = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(p) + i);
    uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      f[2 * k] = bf16_to_f32(u[k] & 0xffff);
      f[2 * k + 1] = bf16_to_f32(u[k] >> 16);
    }
  }
  __device__ static void store8(void* p, int64_t i, const float f[8]) {
    uint4 w;
    w.x = (uint32_t)f32_to_bf16(f[0]) | ((uint32_t)f32_to_bf16(f[1]) << 16);
    w.y = (uint32_t)f32_to_bf16(f[2]) | ((uint32_t)f32_to_bf16(f[3]) << 16);
    w.z = (uint32_t)f32_to_bf16(f[4]) | ((uint32_t)f32_to_bf16(f[5]) << 16);
    w.w = (uint32_t)f32_to_bf16(f[6]) | ((uint32_t)f32_to_bf16(f[7]) << 16);
    *reinterpret_cast<uint4*>(static_cast<uint16_t*>(p) + i) = w;
  }
  // y > 0 test straight on the bits (sign clear, not +0, not NaN): no conversion needed.
  __device__ static bool pos16(uint32_t h) { return !(h & 0x8000u) && (h & 0x7fffu) && (h & 0x7fffu) <= 0x7f80u; }
  // store8 that also returns the ReLU mask of the STORED (rounded) values, bit k = channel k
  __device__ static uint32_t store8m(void* p, int64_t i, const float f[8]) {
    uint32_t h[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = f32_to_bf16(f[k]);
    *reinterpret_cast<uint4*>(static_cast<uint16_t*>(p) + i) =
        make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) m |= (pos16(h[k]) ? 1u : 0u) << k;
    return m;
  }
  __device__ static void pos8(const void* p, int64_t i, bool m[8]) {
    uint4 w = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(p) + i);
    uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint16_t lo = u[k] & 0xffff, hi = u[k] >> 16;
      m[2 * k] = !(lo & 0x8000) && (lo & 0x7fff) && (lo & 0x7fff) <= 0x7f80;
      m[2 * k + 1] = !(hi & 0x8000) && (hi & 0x7fff) && (hi & 0x7fff) <= 0x7f80;
    }
  }
};

struct F16 {
  __device__ static void load8(const void* p, int64_t i, float f[8]) {
    uint4 w = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(p) + i);
    uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      f[2 * k] = f16_to_f32(u[k] & 0xffff);
      f[2 * k + 1] = f16_to_f32(u[k] >> 16);
    }
  }
  __device__ static uint16_t to16(float v) { return __builtin_bit_cast(uint16_t, (_Float16)v); }
  __device__ static void store8(void* p, int64_t i, const float f[8]) {
    uint4 w;
    w.x = (uint32_t)to16(f[0]) | ((uint32_t)to16(f[1]) << 16);
    w.y = (uint32_t)to16(f[2]) | ((uint32_t)to16(f[3]) << 16);
    w.z = (uint32_t)to16(f[4]) | ((uint32_t)to16(f[5]) << 16);
    w.w = (uint32_t)to16(f[6]) | ((uint32_t)to16(f[7]) << 16);
    *reinterpret_cast<uint4*>(static_cast<uint16_t*>(p) + i) = w;
  }
  __device__ static uint32_t store8m(void* p, int64_t i, const float f[8]) {
    store8(p, i, f);
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) m |= ((float)__builtin_bit_cast(_Float16, to16(f[k])) > 0.0f ? 1u : 0u) << k;
    return m;
  }
  __device__ static void pos8(const void* p, int64_t i, bool m[8]) {
    float f[8];
    load8(p, i, f);
#pragma unroll
    for (int k = 0; k < 8; ++k) m[k] = f[k] > 0.0f;
  }
};

struct F32 {
  __device__ static void load8(const void* p, int64_t i, float f[8]) {
    const float4* q = reinterpret_cast<const float4*>(static_cast<const float*>(p) + i);
    float4 a = q[0], b = q[1];
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  }
  __device__ static void store8(void* p, int64_t i, const float f[8]) {
    float4* q = reinterpret_cast<float4*>(static_cast<float*>(p) + i);
    q[0] = make_float4(f[0], f[1], f[2], f[3]);
    q[1] = make_float4(f[4], f[5], f[6], f[7]);
  }
  __device__ static uint32_t store8m(void* p, int64_t i, const float f[8]) {
    store8(p, i, f);
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) m |= (f[k] > 0.0f ? 1u : 0u) << k;
    return m;
  }
  __device__ static void pos8(const void* p, int64_t i, bool m[8]) {
    float f[8];
    load8(p, i, f);
#pragma unroll
    for (int k = 0; k < 8; ++k) m[k] = f[k] > 0.0f;
  }
};

}  // namespace dpt
