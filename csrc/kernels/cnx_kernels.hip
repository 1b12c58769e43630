// ConvNeXt block kernels for gfx950: LayerNorm over the channels of a channels-last activation
// (forward, backward) and the block tail out = x + layer_scale * (fc2 output + bias) (forward,
// backward).  With the depthwise conv (dwconv_kernels.hip) and the MLP GEMMs (ops/vit.py) these
// are the passes of a block; in the stock step they are ATen's fp32 LayerNorm kernels, the
// autocast casts around them, and four or five elementwise / column-sum passes for the tail.
//
// All tensors are row-major [T, C] views of channels-last activations, T = N*H*W.  KIND is 1
// (bf16) or 2 (fp16); accumulation is fp32, element offsets are 64-bit.  No atomics: per-block
// fp32 partials are summed in a fixed order by the colsum_rows kernel (vit_kernels.hip), so two
// runs agree bit for bit.
//
// Row geometry of the LayerNorm kernels
// -------------------------------------
// ViT's ln_fwd / ln_bwd give one wave to a row of D % 256 == 0 fp32 values.  ConvNeXt's rows are
// 96..1024 16-bit channels (192 bytes at stage 1, 401,408 of them at batch 128): one wave per
// row would leave 52 of 64 lanes idle.  Here a row is shared by LANES lanes (a power of two),
// each holding VPL 16-byte vectors of 8 channels, C = LANES * VPL * 8; vector j of lane l is at
// channel (j*LANES + l)*8, so the lanes of a row read contiguous 16-byte pieces (32-byte pieces
// of an fp32 row) and 64/LANES rows run per wave, 4 * 64/LANES per 256-thread block:
//
//      C    LANES VPL  rows/wave        C    LANES VPL  rows/wave
//      96     4    3     16            128    16    1      4
//     192     8    3      8            256    16    2      4
//     384    16    3      4            512    32    2      2
//     768    32    3      2           1024    64    2      1
//
// Every width is covered with no idle lane.  128 could also run as (4, 4) and 1024 as (32, 4); both
// were built and measured on an MI355X at batch 128 (profiles/convnext_block.md: 128 channels at
// 56 px forward 34.3 vs 36.6 us, backward 69.0 vs 69.7; 1024 at 7 px 7.0 vs 7.2 and 14.8 vs 16.3)
// and the slower instances were dropped: the backward keeps 2 * VPL * 8 column accumulators next
// to the row's 2 * VPL * 8 values, 220 VGPRs at VPL = 4 against 76 at VPL = 1 and 126 at VPL = 2
// (172 at VPL = 3: two waves per SIMD, which the 4.2-4.8 TB/s of the stage-1 and stage-2
// backward shows to be enough for a stream).
//   * The lanes of a row are neighbours in the wave (lane = row_in_wave * LANES + l): row sums
//     are __shfl_xor butterflies with offsets LANES/2 .. 1, which never leave the row.  No LDS
//     and no barrier in the forward.
//   * The row stays in registers (VPL * 8 fp32 per lane): the mean is subtracted before the
//     squares are summed (two-pass variance).  Statistics are taken on the values as loaded,
//     16-bit widened exactly, fp32 (IN_F32: the residual stream in front of the downsample
//     LayerNorms) as it is.
//   * gamma / beta are re-read per row (L1/L2 hits) rather than held in 2 * VPL * 8 registers, for
//     the reason given above load4_param in vit_kernels.hip.
//   * Rows past the end load zeros and store nothing: no lane leaves the butterflies.
//
// cnx_ln_fwd_kernel<LANES, VPL, KIND, IN_F32>   h = (y - mean) * rstd * gamma + beta, 16-bit;
//   mean / rstd fp32 per row.  Grid-strided over groups of 4 * 64/LANES rows.
// cnx_ln_bwd_kernel<LANES, VPL, KIND, IN_F32>   gy = rstd * (g - mean_c(g) - xhat * mean_c(g xhat)),
//   g = gh * gamma, in y's type, and per-block column sums of gh * xhat and gh.  A block walks a
//   contiguous slice of rows (a multiple of its 4 * 64/LANES rows per pass) with its column
//   partials in registers; at the end the 4 * 64/LANES row slots of the block are combined through
//   LDS (8 KB * VPL) in slot order and written as part[block][2C] = dgamma | dbeta.  The block
//   count fills the 256 CUs about twice (kCnxMaxBlocks).
//
// Block tail
// ----------
// 8 channels per lane, any C % 8 == 0.  A block's 256 threads are (256 / W) rows x W column groups
// with W = min(C/8, 256) (column blocks of 2048 channels on grid.y above that): a thread's column
// group never changes, so ls / b2 and, in the backward, its 2 x 8 column sums live in registers.
// cnx_scale_residual_fwd_kernel<KIND, X_F32>  out = x + ls[c] * (z + b2[c]) in fp32, one rounding;
//   x fp32 (the residual stream) or 16-bit (the first block after a stem / downsample conv), z
//   16-bit (fc2's output without its bias), out fp32.  Four rows in flight per thread.
// cnx_scale_residual_bwd_kernel<KIND>  one pass over dout (fp32) and z: dz = 16-bit(ls * dout) and
//   per-block column sums of dout * (z + b2) (-> dls) and ls * dout (-> db2), combined like the
//   LayerNorm's.  The residual gradient is dout itself: nothing is written for it.
#include "cnx_io.h"
#include "common.h"
#include "kernels.h"

namespace dpt {

// Sum over the LANES neighbouring lanes that share a row.
template <int LANES>
__device__ __forceinline__ float cnx_row_sum(float v) {
#pragma unroll
  for (int off = LANES / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- LayerNorm over channels: forward ------------------------------------------------------------
template <int LANES, int VPL, int KIND, bool IN_F32>
__global__ __launch_bounds__(kBlock) void cnx_ln_fwd_kernel(const void* __restrict__ y,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta,
                                                            uint16_t* __restrict__ h, float* __restrict__ mean_out,
                                                            float* __restrict__ rstd_out, int64_t T, float eps) {
  constexpr int C = LANES * VPL * 8, RPW = 64 / LANES, RPB = 4 * RPW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l = lane % LANES, slot = wave * RPW + lane / LANES;
  for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < T; r0 += (int64_t)gridDim.x * RPB) {
    const int64_t row = r0 + slot;
    const bool live = row < T;
    const int64_t base = row * C;
    float v[VPL][8];
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      if (live) {
        cnx_load8<KIND, IN_F32>(y, base + (j * LANES + l) * 8, v[j]);
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[j][k] = 0.f;
      }
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j)
#pragma unroll
      for (int k = 0; k < 8; ++k) sum += v[j][k];
    const float mean = cnx_row_sum<LANES>(sum) * (1.f / C);
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        v[j][k] -= mean;
        sq = fmaf(v[j][k], v[j][k], sq);
      }
    const float rstd = rsqrtf(cnx_row_sum<LANES>(sq) * (1.f / C) + eps);
    if (live) {
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        const int c0 = (j * LANES + l) * 8;
        float gm[8], bt[8], o[8];
        cnx_load8<1, true>(gamma, c0, gm);
        cnx_load8<1, true>(beta, c0, bt);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = fmaf(v[j][k] * rstd, gm[k], bt[k]);
        cnx_store8<KIND, false>(h, base + c0, o);
      }
      if (l == 0) {
        mean_out[row] = mean;
        rstd_out[row] = rstd;
      }
    }
  }
}

// ---- LayerNorm over channels: backward -----------------------------------------------------------
template <int LANES, int VPL, int KIND, bool IN_F32>
__global__ __launch_bounds__(kBlock) void cnx_ln_bwd_kernel(const uint16_t* __restrict__ gh,
                                                            const void* __restrict__ y,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, void* __restrict__ gy,
                                                            float* __restrict__ part, int64_t T,
                                                            int64_t rows_per_block) {
  constexpr int C = LANES * VPL * 8, RPW = 64 / LANES, RPB = 4 * RPW;
  __shared__ float red[RPB * C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l = lane % LANES, slot = wave * RPW + lane / LANES;
  float ag[VPL][8], ab[VPL][8];
#pragma unroll
  for (int j = 0; j < VPL; ++j)
#pragma unroll
    for (int k = 0; k < 8; ++k) ag[j][k] = ab[j][k] = 0.f;

  const int64_t row0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t row1 = min(row0 + rows_per_block, T);
  for (int64_t r0 = row0; r0 < row1; r0 += RPB) {
    const int64_t row = r0 + slot;
    const bool live = row < row1;
    const int64_t base = row * C;
    float xh[VPL][8], g[VPL][8];
    float mu = 0.f, rs = 0.f;
    if (live) {
      mu = mean[row];
      rs = rstd[row];
    }
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      if (live) {
        const int64_t off = base + (j * LANES + l) * 8;
        cnx_load8<KIND, IN_F32>(y, off, xh[j]);
        cnx_load8<KIND, false>(gh, off, g[j]);
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) xh[j][k] = g[j][k] = 0.f;
      }
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      float gm[8];
      cnx_load8<1, true>(gamma, (j * LANES + l) * 8, gm);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        xh[j][k] = (xh[j][k] - mu) * rs;   // a dead row: (0 - 0) * 0
        ab[j][k] += g[j][k];
        ag[j][k] = fmaf(g[j][k], xh[j][k], ag[j][k]);
        g[j][k] *= gm[k];
        s1 += g[j][k];
        s2 = fmaf(g[j][k], xh[j][k], s2);
      }
    }
    const float c1 = cnx_row_sum<LANES>(s1) * (1.f / C), c2 = cnx_row_sum<LANES>(s2) * (1.f / C);
    if (live) {
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        float o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = rs * (g[j][k] - c1 - xh[j][k] * c2);
        cnx_store8<KIND, IN_F32>(gy, base + (j * LANES + l) * 8, o);
      }
    }
  }

  // Combine the block's RPB row slots in slot order: part[block][0..C) = dgamma, [C..2C) = dbeta.
  float* dst = part + (int64_t)blockIdx.x * (2 * C);
#pragma unroll
  for (int which = 0; which < 2; ++which) {
#pragma unroll
    for (int j = 0; j < VPL; ++j)
#pragma unroll
      for (int k = 0; k < 8; ++k) red[slot * C + (j * LANES + l) * 8 + k] = which == 0 ? ag[j][k] : ab[j][k];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += kBlock) {
      float sum = red[c];
#pragma unroll 4
      for (int q = 1; q < RPB; ++q) sum += red[q * C + c];
      dst[which * C + c] = sum;
    }
    __syncthreads();
  }
}

// ---- block tail: out = x + ls * (z + b2) --------------------------------------------------------
constexpr int kCnxSrRows = 4;  // rows in flight per thread in the forward

template <int KIND, bool X_F32>
__global__ __launch_bounds__(kBlock) void cnx_scale_residual_fwd_kernel(const void* __restrict__ x,
                                                                        const uint16_t* __restrict__ z,
                                                                        const void* __restrict__ b2, int b2_kind,
                                                                        const float* __restrict__ ls,
                                                                        float* __restrict__ out, int64_t T, int C,
                                                                        int W) {
  const int RB = kBlock / W;
  const int cl = threadIdx.x % W, rl = threadIdx.x / W;
  const int c0 = (blockIdx.y * W + cl) * 8;
  if (rl >= RB || c0 >= C) return;
  float b[8], s[8];
  cnx_param8(b2, b2_kind, c0, b);
  cnx_load8<1, true>(ls, c0, s);
  const int64_t stride = (int64_t)gridDim.x * RB;
  for (int64_t r = (int64_t)blockIdx.x * RB + rl; r < T; r += stride * kCnxSrRows) {
    float xv[kCnxSrRows][8], zv[kCnxSrRows][8];
#pragma unroll
    for (int q = 0; q < kCnxSrRows; ++q) {
      const int64_t row = r + q * stride;
      if (row < T) {
        cnx_load8<KIND, X_F32>(x, row * C + c0, xv[q]);
        cnx_load8<KIND, false>(z, row * C + c0, zv[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < kCnxSrRows; ++q) {
      const int64_t row = r + q * stride;
      if (row < T) {
#pragma unroll
        for (int k = 0; k < 8; ++k) xv[q][k] = fmaf(s[k], zv[q][k] + b[k], xv[q][k]);
        cnx_store8<1, true>(out, row * C + c0, xv[q]);
      }
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void cnx_scale_residual_bwd_kernel(const float* __restrict__ dout,
                                                                        const uint16_t* __restrict__ z,
                                                                        const void* __restrict__ b2, int b2_kind,
                                                                        const float* __restrict__ ls,
                                                                        uint16_t* __restrict__ dz,
                                                                        float* __restrict__ part, int64_t T, int C,
                                                                        int W, int64_t rows_per_block) {
  __shared__ float red[kBlock * 8];
  const int RB = kBlock / W;
  const int cl = threadIdx.x % W, rl = threadIdx.x / W;
  const int cb = blockIdx.y * W * 8;  // first channel of this column block
  const int c0 = cb + cl * 8;
  const bool mine = rl < RB && c0 < C;
  float b[8], s[8], als[8], ab2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) b[k] = s[k] = als[k] = ab2[k] = 0.f;
  if (mine) {
    cnx_param8(b2, b2_kind, c0, b);
    cnx_load8<1, true>(ls, c0, s);
    const int64_t row0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t row1 = min(row0 + rows_per_block, T);
    int64_t r = row0 + rl;
    for (; r + RB < row1; r += 2 * RB) {  // two rows in flight
      float d0[8], z0[8], d1[8], z1[8];
      cnx_load8<1, true>(dout, r * C + c0, d0);
      cnx_load8<KIND, false>(z, r * C + c0, z0);
      cnx_load8<1, true>(dout, (r + RB) * C + c0, d1);
      cnx_load8<KIND, false>(z, (r + RB) * C + c0, z1);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        als[k] = fmaf(d0[k], z0[k] + b[k], als[k]);
        d0[k] *= s[k];
        ab2[k] += d0[k];
      }
      cnx_store8<KIND, false>(dz, r * C + c0, d0);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        als[k] = fmaf(d1[k], z1[k] + b[k], als[k]);
        d1[k] *= s[k];
        ab2[k] += d1[k];
      }
      cnx_store8<KIND, false>(dz, (r + RB) * C + c0, d1);
    }
    if (r < row1) {
      float d0[8], z0[8];
      cnx_load8<1, true>(dout, r * C + c0, d0);
      cnx_load8<KIND, false>(z, r * C + c0, z0);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        als[k] = fmaf(d0[k], z0[k] + b[k], als[k]);
        d0[k] *= s[k];
        ab2[k] += d0[k];
      }
      cnx_store8<KIND, false>(dz, r * C + c0, d0);
    }
  }
  // Combine the RB row slots in slot order: part[0][block][C] = dls, part[1][block][C] = db2 partials.
  const int WC = W * 8;
  const int64_t nb = gridDim.x;
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    if (rl < RB) {
#pragma unroll
      for (int k = 0; k < 8; ++k) red[rl * WC + cl * 8 + k] = which == 0 ? als[k] : ab2[k];
    }
    __syncthreads();
    float* dst = part + ((int64_t)which * nb + blockIdx.x) * C;
    for (int c = threadIdx.x; c < WC; c += kBlock) {
      if (cb + c < C) {
        float sum = red[c];
        for (int q = 1; q < RB; ++q) sum += red[q * WC + c];
        dst[cb + c] = sum;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// LANES for width C (VPL = C / (8 * LANES)); 0: unsupported
static int cnx_lanes(int64_t C) {
  switch (C) {
    case 96: return 4;
    case 192: return 8;
    case 384: return 16;
    case 768: return 32;
    case 128: return 16;
    case 256: return 16;
    case 512: return 32;
    case 1024: return 64;
    default: return 0;
  }
}

bool cnx_ln_supported(int64_t C) { return cnx_lanes(C) != 0; }

int cnx_ln_rows_per_block(int64_t C) { return cnx_ln_supported(C) ? 4 * 64 / cnx_lanes(C) : 0; }

// Slices of `unit`-row passes for a walk of T rows by at most max_blocks blocks: rows per block (a
// multiple of unit) and the block count, with no empty block.
static void cnx_slices(int64_t T, int unit, int max_blocks, int64_t* rows_per_block, int* blocks) {
  int64_t nb = (T + unit - 1) / unit;
  if (nb > max_blocks) nb = max_blocks;
  if (nb < 1) nb = 1;
  int64_t rpb = (T + nb - 1) / nb;
  rpb = (rpb + unit - 1) / unit * unit;
  if (rpb < unit) rpb = unit;
  *rows_per_block = rpb;
  const int64_t b = (T + rpb - 1) / rpb;
  *blocks = (int)(b < 1 ? 1 : b);
}

int cnx_ln_bwd_blocks(int64_t T, int64_t C) {
  int64_t rpb;
  int nb;
  cnx_slices(T, cnx_ln_rows_per_block(C), kCnxMaxBlocks, &rpb, &nb);
  return nb;
}

template <int LANES, int VPL, int KIND, bool IN_F32>
static void cnx_ln_fwd_go(const void* y, const float* gamma, const float* beta, uint16_t* h, float* mean, float* rstd,
                          int64_t T, float eps, hipStream_t s) {
  constexpr int RPB = 4 * 64 / LANES;
  int64_t g = (T + RPB - 1) / RPB;
  if (g > kMaxBlocks) g = kMaxBlocks;
  hipLaunchKernelGGL((cnx_ln_fwd_kernel<LANES, VPL, KIND, IN_F32>), dim3((unsigned)g), dim3(kBlock), 0, s, y, gamma,
                     beta, h, mean, rstd, T, eps);
}

template <int LANES, int VPL, int KIND, bool IN_F32>
static void cnx_ln_bwd_go(const uint16_t* gh, const void* y, const float* mean, const float* rstd, const float* gamma,
                          void* gy, float* part, int64_t T, hipStream_t s) {
  int64_t rpb;
  int nb;
  cnx_slices(T, 4 * 64 / LANES, kCnxMaxBlocks, &rpb, &nb);
  hipLaunchKernelGGL((cnx_ln_bwd_kernel<LANES, VPL, KIND, IN_F32>), dim3((unsigned)nb), dim3(kBlock), 0, s, gh, y,
                     mean, rstd, gamma, gy, part, T, rpb);
}

// fn(lanes, vpl) with the geometry of width C as compile-time constants
template <class Fn>
static void cnx_with_geometry(int64_t C, Fn&& fn) {
  using std::integral_constant;
  switch (C) {
    case 96: fn(integral_constant<int, 4>{}, integral_constant<int, 3>{}); break;
    case 192: fn(integral_constant<int, 8>{}, integral_constant<int, 3>{}); break;
    case 384: fn(integral_constant<int, 16>{}, integral_constant<int, 3>{}); break;
    case 768: fn(integral_constant<int, 32>{}, integral_constant<int, 3>{}); break;
    case 128: fn(integral_constant<int, 16>{}, integral_constant<int, 1>{}); break;
    case 256: fn(integral_constant<int, 16>{}, integral_constant<int, 2>{}); break;
    case 512: fn(integral_constant<int, 32>{}, integral_constant<int, 2>{}); break;
    default: fn(integral_constant<int, 64>{}, integral_constant<int, 2>{}); break;
  }
}

template <int KIND>
static void cnx_ln_fwd_kind(bool in_f32, const void* y, const float* gamma, const float* beta, uint16_t* h, float* mean,
                            float* rstd, int64_t T, int64_t C, float eps, hipStream_t s) {
  cnx_with_geometry(C, [&](auto lanes, auto vpl) {
    with_bool(in_f32, [&](auto f32) {
      cnx_ln_fwd_go<decltype(lanes)::value, decltype(vpl)::value, KIND, decltype(f32)::value>(y, gamma, beta, h, mean,
                                                                                              rstd, T, eps, s);
    });
  });
}

template <int KIND>
static void cnx_ln_bwd_kind(bool in_f32, const uint16_t* gh, const void* y, const float* mean, const float* rstd,
                            const float* gamma, void* gy, float* part, int64_t T, int64_t C, hipStream_t s) {
  cnx_with_geometry(C, [&](auto lanes, auto vpl) {
    with_bool(in_f32, [&](auto f32) {
      cnx_ln_bwd_go<decltype(lanes)::value, decltype(vpl)::value, KIND, decltype(f32)::value>(gh, y, mean, rstd, gamma,
                                                                                              gy, part, T, s);
    });
  });
}

void launch_cnx_ln_fwd(int kind, bool in_f32, const void* y, const float* gamma, const float* beta, uint16_t* h,
                       float* mean, float* rstd, int64_t T, int64_t C, float eps, hipStream_t s) {
  if (T <= 0) return;
  if (kind == 1) cnx_ln_fwd_kind<1>(in_f32, y, gamma, beta, h, mean, rstd, T, C, eps, s);
  else cnx_ln_fwd_kind<2>(in_f32, y, gamma, beta, h, mean, rstd, T, C, eps, s);
}

void launch_cnx_ln_bwd(int kind, bool in_f32, const uint16_t* gh, const void* y, const float* mean, const float* rstd,
                       const float* gamma, void* gy, float* part, int64_t T, int64_t C, hipStream_t s) {
  if (kind == 1) cnx_ln_bwd_kind<1>(in_f32, gh, y, mean, rstd, gamma, gy, part, T, C, s);
  else cnx_ln_bwd_kind<2>(in_f32, gh, y, mean, rstd, gamma, gy, part, T, C, s);
}

// ---- block tail ---------------------------------------------------------------------------------
bool cnx_scale_residual_supported(int64_t C) { return C > 0 && C % 8 == 0 && C / 8 <= 65535 * (int64_t)kBlock; }

static int cnx_sr_width(int64_t C) { return (int)(C / 8 < kBlock ? C / 8 : kBlock); }

int cnx_scale_residual_rows_per_block(int64_t C) { return kBlock / cnx_sr_width(C); }

static int cnx_sr_colblocks(int64_t C) {
  const int W = cnx_sr_width(C);
  return (int)((C / 8 + W - 1) / W);
}

int cnx_scale_residual_bwd_blocks(int64_t T, int64_t C) {
  int64_t rpb;
  int nb;
  const int cbk = cnx_sr_colblocks(C);
  cnx_slices(T, cnx_scale_residual_rows_per_block(C), (kCnxMaxBlocks + cbk - 1) / cbk, &rpb, &nb);
  return nb;
}

void launch_cnx_scale_residual_fwd(int kind, bool x_f32, const void* x, const uint16_t* z, const void* b2, int b2_kind,
                                   const float* ls, float* out, int64_t T, int64_t C, hipStream_t s) {
  if (T <= 0) return;
  const int W = cnx_sr_width(C), RB = kBlock / W, cbk = cnx_sr_colblocks(C);
  int64_t g = (T + (int64_t)RB * kCnxSrRows - 1) / ((int64_t)RB * kCnxSrRows);
  const int64_t cap = (kMaxBlocks + cbk - 1) / cbk;
  if (g > cap) g = cap;
  const dim3 gr((unsigned)g, (unsigned)cbk), bl(kBlock);
  with_bool(x_f32, [&](auto f32) {
    if (kind == 1)
      hipLaunchKernelGGL((cnx_scale_residual_fwd_kernel<1, decltype(f32)::value>), gr, bl, 0, s, x, z, b2, b2_kind, ls,
                         out, T, (int)C, W);
    else
      hipLaunchKernelGGL((cnx_scale_residual_fwd_kernel<2, decltype(f32)::value>), gr, bl, 0, s, x, z, b2, b2_kind, ls,
                         out, T, (int)C, W);
  });
}

void launch_cnx_scale_residual_bwd(int kind, const float* dout, const uint16_t* z, const void* b2, int b2_kind,
                                   const float* ls, uint16_t* dz, float* part, int64_t T, int64_t C, hipStream_t s) {
  const int W = cnx_sr_width(C), cbk = cnx_sr_colblocks(C);
  int64_t rpb;
  int nb;
  cnx_slices(T, kBlock / W, (kCnxMaxBlocks + cbk - 1) / cbk, &rpb, &nb);
  const dim3 gr((unsigned)nb, (unsigned)cbk), bl(kBlock);
  if (kind == 1)
    hipLaunchKernelGGL(cnx_scale_residual_bwd_kernel<1>, gr, bl, 0, s, dout, z, b2, b2_kind, ls, dz, part, T, (int)C, W,
                       rpb);
  else
    hipLaunchKernelGGL(cnx_scale_residual_bwd_kernel<2>, gr, bl, 0, s, dout, z, b2, b2_kind, ls, dz, part, T, (int)C, W,
                       rpb);
}

}  // namespace dpt
