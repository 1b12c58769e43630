// The 128-row streamed-A tile of the two tail-fused 1x1 kernels (tail_conv1_kernels.hip,
// tail_conv3_bwd_kernels.hip), for gfx950.
//
// Both kernels form 128 rows of a 16-bit tensor a 64-channel K-step at a time in registers, store
// them, write the same bits into an XOR-swizzled LDS A tile next to a register-staged weight slice
// and run a 128 x BN GEMM whose result is bit-equal to conv_fwd_kernel<128, BN, 1, LDSEPI, ...>: the
// same wave tiling (4x1 waves at BN = 64, 2x2 at BN = 128), v_mfma_f32_32x32x16 with ks and kk
// ascending, the cvt_pk rounding into the LDS image.  That promise is kept here, once: a kernel
// brings its loads, its apply expression, its weight loader and its statistics epilogue.
#pragma once

#include <type_traits>

#include "bn_io.h"
#include "common.h"
#include "mfma.h"

namespace dpt {
namespace tail {

constexpr int BM = 128;
constexpr int BK = 64;
constexpr int kThreads = 256;
constexpr int kRowBytes = BK * 2;
constexpr int A_BYTES = BM * kRowBytes;
constexpr uint32_t kOOB = 0xFFFFFF00u;  // past every descriptor's range: the load returns zeros

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

// K-loop image (A tile, B tile; a kernel's coefficients behind them) and the epilogue's [BM][BN]
// image with padded rows share the front of the LDS
__host__ __device__ constexpr int tile_bytes(int BN) { return A_BYTES + BN * kRowBytes; }
__host__ __device__ constexpr int image_bytes(int BN) { return BM * (BN * 2 + 16); }

// the conversions of IO::load8 / IO::store8, an element at a time
template <typename IO>
__device__ __forceinline__ float up16(uint32_t h) {
  if constexpr (std::is_same<IO, F16>::value) return f16_to_f32((uint16_t)h);
  else return bf16_to_f32((uint16_t)h);
}
template <typename IO>
__device__ __forceinline__ uint32_t down16(float v) {
  if constexpr (std::is_same<IO, F16>::value) return F16::to16(v);
  else return f32_to_bf16(v);
}
template <typename IO>
__device__ __forceinline__ void unpack8(const u32x4& w, float f[8]) {
  const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int k = 0; k < 8; ++k) f[k] = up16<IO>(k & 1 ? u[k >> 1] >> 16 : u[k >> 1] & 0xffffu);
}
__device__ __forceinline__ u32x4 pack8(const uint32_t h[8]) {
  return u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
}

// A block's M-tile and this thread's chunks of a [M, C] tensor: column c (8 channels) of rows
// rb, rb + 32, rb + 64, rb + 96 of the tile.
struct Rows {
  int mt, c, rb;
  int64_t m0;
  uint32_t voff[4];  // byte offset of chunk i at K-step 0
  bool live[4];      // row i is below M
  // rev: the tiles last-to-first (kTailReverse)
  __device__ __forceinline__ Rows(int64_t M, int C, int m_tiles, int rev) {
    const int tid = threadIdx.x;
    mt = rev ? m_tiles - 1 - (int)blockIdx.x : (int)blockIdx.x;
    m0 = (int64_t)mt * BM;
    c = tid & 7;
    rb = tid >> 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t m = m0 + rb + 32 * i;
      live[i] = m < M;
      voff[i] = live[i] ? (uint32_t)((m * C + c * 8) * 2) : kOOB;
    }
  }
  __device__ __forceinline__ uint32_t off(int i, int ks) const {
    return live[i] ? voff[i] + (uint32_t)ks * kRowBytes : kOOB;
  }
};

template <bool F16V, int BN>
struct Tile {
  static constexpr int WN = BN / 64, WM = 4 / WN, MI = BM / (WM * 32), NI = 2;
  static constexpr int B_PER_T = BN * 8 / kThreads;  // weight chunks per thread and K-step
  static constexpr int C_STRIDE = BN * 2 + 16;       // a row of the epilogue's image, padded
  // the [M, BN] output leaves the image in rows of CPR 16-byte chunks, RPP rows per pass
  static constexpr int CPR = BN / 8, RPP = kThreads / CPR, NPASS = BM / RPP;
  static_assert(image_bytes(BN) == BM * C_STRIDE, "the image's rows");
  typedef f32x16_t Acc[MI][NI];

  static __device__ __forceinline__ void zero(Acc& acc) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  }

  // this thread's chunks of the A tile (rows past M: zeros) and of the weight slice into the LDS
  static __device__ __forceinline__ void stage(unsigned char* lds, const u32x4 (&av)[4], const u32x4 (&wb)[B_PER_T]) {
    const int c = threadIdx.x & 7, rb = threadIdx.x >> 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = rb + 32 * i;
      *reinterpret_cast<u32x4*>(lds + row * kRowBytes + swz(row, c) * 16) = av[i];
    }
#pragma unroll
    for (int i = 0; i < B_PER_T; ++i) {
      const int row = rb + 32 * i;
      *reinterpret_cast<u32x4*>(lds + A_BYTES + row * kRowBytes + swz(row, c) * 16) = wb[i];
    }
  }

  // one K-step of the staged tiles onto the accumulators
  static __device__ __forceinline__ void mma(const unsigned char* lds, Acc& acc) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid / WN, wn = wid % WN, lr = lane & 31, lh = lane >> 5;
    const unsigned char* la = lds;
    const unsigned char* lb = lds + A_BYTES;
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      const int ch = kk * 2 + lh;
      bf16x8_t fa[MI], fb[NI];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int row = wm * (MI * 32) + i * 32 + lr;
        fa[i] = *reinterpret_cast<const bf16x8_t*>(la + row * kRowBytes + swz(row, ch) * 16);
      }
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const int row = wn * 64 + j * 32 + lr;
        fb[j] = *reinterpret_cast<const bf16x8_t*>(lb + row * kRowBytes + swz(row, ch) * 16);
      }
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = cmfma<F16V>(fa[i], fb[j], acc[i][j]);
    }
  }

  // the accumulators, rounded, into the LDS image (the epilogue of conv_fwd_kernel, operation for
  // operation); pair(j, u): every packed pair u of column block j, for a kernel's statistics
  template <class Pair>
  static __device__ __forceinline__ void image(unsigned char* lds, const Acc& acc, Pair&& pair) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid / WN, wn = wid % WN, lr = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const int col = wn * 64 + j * 32 + lr;
        const int rbase = wm * (MI * 32) + i * 32 + 4 * lh;
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
          const int r0 = rbase + (e & 3) + 8 * (e >> 2);
          const f32x2_t v = {acc[i][j][e], acc[i][j][e + 1]};
          const uint32_t u = cpack<F16V>(v);
          *reinterpret_cast<uint16_t*>(lds + r0 * C_STRIDE + col * 2) = (uint16_t)u;
          *reinterpret_cast<uint16_t*>(lds + (r0 + 1) * C_STRIDE + col * 2) = (uint16_t)(u >> 16);
          pair(j, u);
        }
      }
  }
};

}  // namespace tail

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// Apply passes walk the rows last-to-first (bn_kernels.hip kBnReverse): the rows the producing
// kernel wrote last are still in the caches.  The fused kernels take their M-tiles in the same order.
constexpr int kTailReverse = 1;

// What both kernels ask of [M, K] x [N][K]: whole K-steps, one output-channel tile, 32-bit byte
// offsets through buffer descriptors as conv_fwd_kernel (conv_check_offsets).  k_msg / n_msg:
// the refusals in the caller's names for K and N.
inline const char* tail_tile_refusal(int64_t M, int64_t K, int64_t N, const char* k_msg, const char* n_msg) {
  if (K < 64 || K % 64 != 0) return k_msg;
  if (N != 64 && N != 128) return n_msg;
  if (M < 1) return "empty input";
  if (M * K * 2 >= 0xFFFFFF00ll || N * K * 2 >= 0x7FFFFFFFll) return "operand tensors beyond 2^31 elements";
  return nullptr;
}

// fn(f16, wide, flag): the element type, BN = 128 and a kernel's own switch as compile-time constants
template <class Fn>
void tail_dispatch(bool f16, bool wide, bool flag, Fn&& fn) {
  with_bool(f16, [&](auto h) { with_bool(wide, [&](auto w) { with_bool(flag, [&](auto t) { fn(h, w, t); }); }); });
}

}  // namespace dpt
