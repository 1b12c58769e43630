// Global Response Normalization (ConvNeXt V2) for gfx950, fused with the MLP's bias + GELU:
//
//   y  = GELU(u + b1)                     u [N, R, D] 16-bit: fc1's output without its bias
//   G  = ||y||_2 over the R rows          [N, D]
//   Nx = G / (mean_D G + eps)             [N, D]
//   g  = gamma * (y * Nx) + beta + y      16-bit, fc2's operand
//
// R = H*W pixels per sample, D = 4 * dim.  y is the widest tensor of a block and no element of g can
// be written before every row of its sample has been seen, so the work is two sweeps per direction
// around a tiny per-sample kernel.  y is never stored: each sweep re-reads u and recomputes the GELU
// (about 20 fp32 instructions per element, gelu.h) instead of one more write and one more read of
// [N, R, D].  The backward needs y, GELU'(u + b1) and dg together, and both come from the one
// erf_and_gauss call, so it recomputes too.
//
// KIND is 1 (bf16) or 2 (fp16).  All arithmetic and all sums are fp32, element offsets are 64-bit.
// No atomics: every reduction is a set of fp32 partials summed in a fixed order, so two runs (and
// every replay of a captured graph) agree bit for bit.
//
// Sweep geometry (all four sweeps)
// --------------------------------
// 8 channels per lane.  A block's 256 threads are RB = 256 / W row slots x W column groups, W =
// min(D/8, 256); column blocks of 2048 channels go on grid.y above D = 2048.  A thread's column group
// never changes, so b1 and the per-(sample, channel) vectors it needs (s, t, beta) and its column
// sums live in registers (the scheme of cnx_scale_residual_bwd_kernel).  blockIdx.x = n * sps + slice:
// a block walks rows [slice * rps, min((slice + 1) * rps, R)) of sample n, rps a multiple of RB, so a
// slice never crosses a sample boundary and the statistics of a sample are the sum of its sps
// partials.  sps is chosen so that N * sps * (column blocks) is about kGrnMaxBlocks (eight blocks per
// CU: the sweeps hold 54-108 VGPRs, four to eight blocks are resident per CU, and the GELU's
// arithmetic has to overlap the loads of other waves), never more than one slice per RB rows.  Two
// rows are in flight per thread.  The RB row slots of a block are combined through LDS (8 KB) in
// slot order.  Measured on an MI355X at batch 128 (profiles/convnext_v2_grn.md): the statistics
// sweeps run at the GELU's arithmetic rate (about 1.5 T elements/s), not the memory's.
//
// grn_fwd_stats_kernel<KIND>     part[n * sps + slice][D] = sum_rows y^2
// grn_fwd_finalize_kernel        one block per sample: G = sqrt(sum_slices part) (slices in order), the
//                                mean over D (per-thread strided sums, wave butterfly, the four waves
//                                through LDS in order), inv = 1 / (mean + eps), s = 1 + gamma * G * inv.
//                                G, inv and s are kept for the backward.
// grn_fwd_apply_kernel<KIND>     g = fma(y, s[n], beta), one rounding to 16 bits
// grn_bwd_stats_kernel<KIND>     part[0][n * sps + slice][D] = sum_rows dg * y, part[1][..] = sum_rows dg
//                                (the column sum of part[1] over all its rows is dbeta)
// grn_bwd_finalize_kernel        one block per sample: S = sum_slices part[0], sn = S * Nx (its column
//                                sum over n is dgamma), dNx = gamma * S, A = sum_D dNx * G (reduced
//                                like the mean), dG = dNx * inv - A * inv^2 / D, t = dG / G (0 where
//                                G == 0: y is 0 in every row there, and so is the gradient through G)
// grn_bwd_apply_kernel<KIND>     dy = fma(dg, s[n], y * t[n]), du = dy * GELU'(u + b1), one rounding to
//                                16 bits; part[n * sps + slice][D] = sum_rows du (fp32, before the
//                                rounding; its column sum is db1)
// The column sums over the rows of a partials array are colsum_rows (vit_kernels.hip), fixed order.
#include "cnx_io.h"
#include "common.h"
#include "gelu.h"
#include "kernels.h"

namespace dpt {

// How a sweep's blocks tile [N, R, D]; filled by grn_geometry.
struct GrnGeom {
  int W, RB, cbk, sps;
  int64_t rps;
};

// Rows [*r0, *r1) of the whole [N * R, D] array that block blockIdx.x walks, and its sample.
__device__ __forceinline__ int64_t grn_slice(int64_t R, int sps, int64_t rps, int64_t* r0, int64_t* r1) {
  const int64_t n = blockIdx.x / sps, sl = blockIdx.x % sps;
  const int64_t a = sl * rps, b = min(a + rps, R);
  *r0 = n * R + a;
  *r1 = n * R + b;
  return n;
}

// y = GELU(z) and GELU'(z) from the one erf_and_gauss call (the values of gelu_f and gelu_grad)
__device__ __forceinline__ void grn_gelu_both(float z, float& y, float& dy) {
  float g;
  const float cdf = 0.5f * (1.f + erf_and_gauss(z, g));
  y = z * cdf;
  dy = cdf + z * g * 0.39894228040143268f;
}

// Combine the RB row slots of a block in slot order: dst[cb + c] = sum_slot acc of column c.  Every
// thread of the block calls it (threads with mine == false hold zeros or are outside the RB slots).
__device__ __forceinline__ void grn_combine_slots(float* red, const float acc[8], float* dst, int W, int RB, int cl,
                                                  int rl, int cb, int D) {
  const int WC = W * 8;
  if (rl < RB) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red[rl * WC + cl * 8 + k] = acc[k];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < WC; c += kBlock) {
    if (cb + c < D) {
      float sum = red[c];
      for (int q = 1; q < RB; ++q) sum += red[q * WC + c];
      dst[cb + c] = sum;
    }
  }
  __syncthreads();
}

// Sum of v over the block's 256 threads in a fixed order, returned to every thread.
__device__ __forceinline__ float grn_block_sum(float v, float* red4) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();  // red4 may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red4[0] + red4[1]) + red4[2]) + red4[3];
}

// ---- forward ------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(kBlock) void grn_fwd_stats_kernel(const uint16_t* __restrict__ u,
                                                               const void* __restrict__ b1, int b1_kind,
                                                               float* __restrict__ part, int64_t R, int D, int W,
                                                               int sps, int64_t rps) {
  __shared__ float red[kBlock * 8];
  const int RB = kBlock / W;
  const int cl = threadIdx.x % W, rl = threadIdx.x / W;
  const int cb = blockIdx.y * W * 8, c0 = cb + cl * 8;
  const bool mine = rl < RB && c0 < D;
  int64_t row0, row1;
  grn_slice(R, sps, rps, &row0, &row1);
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  if (mine) {
    float b[8];
    cnx_param8(b1, b1_kind, c0, b);
    for (int64_t r = row0 + rl; r < row1; r += 2 * RB) {
      const bool two = r + RB < row1;
      float v0[8], v1[8];
      cnx_load8<KIND, false>(u, r * D + c0, v0);
      if (two) cnx_load8<KIND, false>(u, (r + RB) * D + c0, v1);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float y = gelu_f(v0[k] + b[k]);
        acc[k] = fmaf(y, y, acc[k]);
      }
      if (two) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float y = gelu_f(v1[k] + b[k]);
          acc[k] = fmaf(y, y, acc[k]);
        }
      }
    }
  }
  grn_combine_slots(red, acc, part + (int64_t)blockIdx.x * D, W, RB, cl, rl, cb, D);
}

__global__ __launch_bounds__(kBlock) void grn_fwd_finalize_kernel(const float* __restrict__ part,
                                                                  const float* __restrict__ gamma,
                                                                  float* __restrict__ G, float* __restrict__ inv_out,
                                                                  float* __restrict__ s, int D, int sps, float eps) {
  __shared__ float red4[4];
  const int64_t n = blockIdx.x;
  const float* p = part + n * sps * D;
  float* Gn = G + n * D;
  float local = 0.f;
  for (int d = threadIdx.x; d < D; d += kBlock) {
    float sq = p[d];
#pragma unroll 8   // the slices' loads in flight together; the adds stay in slice order
    for (int q = 1; q < sps; ++q) sq += p[(int64_t)q * D + d];
    const float g = sqrtf(sq);
    Gn[d] = g;
    local += g;
  }
  const float inv = 1.f / (grn_block_sum(local, red4) * (1.f / D) + eps);
  if (threadIdx.x == 0) inv_out[n] = inv;
  for (int d = threadIdx.x; d < D; d += kBlock) s[n * D + d] = fmaf(gamma[d], Gn[d] * inv, 1.f);  // own writes
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void grn_fwd_apply_kernel(const uint16_t* __restrict__ u,
                                                               const void* __restrict__ b1, int b1_kind,
                                                               const float* __restrict__ s,
                                                               const float* __restrict__ beta,
                                                               uint16_t* __restrict__ g, int64_t R, int D, int W,
                                                               int sps, int64_t rps) {
  const int RB = kBlock / W;
  const int cl = threadIdx.x % W, rl = threadIdx.x / W;
  const int c0 = (blockIdx.y * W + cl) * 8;
  if (rl >= RB || c0 >= D) return;
  int64_t row0, row1;
  const int64_t n = grn_slice(R, sps, rps, &row0, &row1);
  float b[8], sc[8], bt[8];
  cnx_param8(b1, b1_kind, c0, b);
  cnx_load8<1, true>(s, n * D + c0, sc);
  cnx_load8<1, true>(beta, c0, bt);
  for (int64_t r = row0 + rl; r < row1; r += 2 * RB) {
    const bool two = r + RB < row1;
    float v0[8], v1[8];
    cnx_load8<KIND, false>(u, r * D + c0, v0);
    if (two) cnx_load8<KIND, false>(u, (r + RB) * D + c0, v1);
#pragma unroll
    for (int k = 0; k < 8; ++k) v0[k] = fmaf(gelu_f(v0[k] + b[k]), sc[k], bt[k]);
    cnx_store8<KIND, false>(g, r * D + c0, v0);
    if (two) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v1[k] = fmaf(gelu_f(v1[k] + b[k]), sc[k], bt[k]);
      cnx_store8<KIND, false>(g, (r + RB) * D + c0, v1);
    }
  }
}

// ---- backward -----------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(kBlock) void grn_bwd_stats_kernel(const uint16_t* __restrict__ dg,
                                                               const uint16_t* __restrict__ u,
                                                               const void* __restrict__ b1, int b1_kind,
                                                               float* __restrict__ part, int64_t R, int D, int W,
                                                               int sps, int64_t rps) {
  __shared__ float red[kBlock * 8];
  const int RB = kBlock / W;
  const int cl = threadIdx.x % W, rl = threadIdx.x / W;
  const int cb = blockIdx.y * W * 8, c0 = cb + cl * 8;
  const bool mine = rl < RB && c0 < D;
  int64_t row0, row1;
  grn_slice(R, sps, rps, &row0, &row1);
  float as[8], ab[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) as[k] = ab[k] = 0.f;
  if (mine) {
    float b[8];
    cnx_param8(b1, b1_kind, c0, b);
    for (int64_t r = row0 + rl; r < row1; r += 2 * RB) {
      const bool two = r + RB < row1;
      float v0[8], d0[8], v1[8], d1[8];
      cnx_load8<KIND, false>(u, r * D + c0, v0);
      cnx_load8<KIND, false>(dg, r * D + c0, d0);
      if (two) {
        cnx_load8<KIND, false>(u, (r + RB) * D + c0, v1);
        cnx_load8<KIND, false>(dg, (r + RB) * D + c0, d1);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        as[k] = fmaf(d0[k], gelu_f(v0[k] + b[k]), as[k]);
        ab[k] += d0[k];
      }
      if (two) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          as[k] = fmaf(d1[k], gelu_f(v1[k] + b[k]), as[k]);
          ab[k] += d1[k];
        }
      }
    }
  }
  const int64_t nb = gridDim.x;
  grn_combine_slots(red, as, part + (int64_t)blockIdx.x * D, W, RB, cl, rl, cb, D);
  grn_combine_slots(red, ab, part + (nb + blockIdx.x) * D, W, RB, cl, rl, cb, D);
}

__global__ __launch_bounds__(kBlock) void grn_bwd_finalize_kernel(const float* __restrict__ part,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ G,
                                                                  const float* __restrict__ inv_in,
                                                                  float* __restrict__ t, float* __restrict__ sn, int D,
                                                                  int sps) {
  __shared__ float red4[4];
  const int64_t n = blockIdx.x;
  const float* p = part + n * sps * D;
  const float* Gn = G + n * D;
  float* tn = t + n * D;
  const float inv = inv_in[n];
  float local = 0.f;
  for (int d = threadIdx.x; d < D; d += kBlock) {
    float S = p[d];
#pragma unroll 8
    for (int q = 1; q < sps; ++q) S += p[(int64_t)q * D + d];
    const float g = Gn[d], dnx = gamma[d] * S;
    sn[n * D + d] = S * (g * inv);
    tn[d] = dnx;  // read back below by this thread
    local = fmaf(dnx, g, local);
  }
  const float c2 = grn_block_sum(local, red4) * (1.f / D) * inv * inv;
  for (int d = threadIdx.x; d < D; d += kBlock) {
    const float g = Gn[d];
    tn[d] = g > 0.f ? (tn[d] * inv - c2) / g : 0.f;
  }
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void grn_bwd_apply_kernel(const uint16_t* __restrict__ dg,
                                                               const uint16_t* __restrict__ u,
                                                               const void* __restrict__ b1, int b1_kind,
                                                               const float* __restrict__ s,
                                                               const float* __restrict__ t,
                                                               uint16_t* __restrict__ du, float* __restrict__ part,
                                                               int64_t R, int D, int W, int sps, int64_t rps) {
  __shared__ float red[kBlock * 8];
  const int RB = kBlock / W;
  const int cl = threadIdx.x % W, rl = threadIdx.x / W;
  const int cb = blockIdx.y * W * 8, c0 = cb + cl * 8;
  const bool mine = rl < RB && c0 < D;
  int64_t row0, row1;
  const int64_t n = grn_slice(R, sps, rps, &row0, &row1);
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  if (mine) {
    float b[8], sc[8], tc[8];
    cnx_param8(b1, b1_kind, c0, b);
    cnx_load8<1, true>(s, n * D + c0, sc);
    cnx_load8<1, true>(t, n * D + c0, tc);
    for (int64_t r = row0 + rl; r < row1; r += 2 * RB) {
      const bool two = r + RB < row1;
      float v0[8], d0[8], v1[8], d1[8];
      cnx_load8<KIND, false>(u, r * D + c0, v0);
      cnx_load8<KIND, false>(dg, r * D + c0, d0);
      if (two) {
        cnx_load8<KIND, false>(u, (r + RB) * D + c0, v1);
        cnx_load8<KIND, false>(dg, (r + RB) * D + c0, d1);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float y, gp;
        grn_gelu_both(v0[k] + b[k], y, gp);
        d0[k] = fmaf(d0[k], sc[k], y * tc[k]) * gp;
        acc[k] += d0[k];
      }
      cnx_store8<KIND, false>(du, r * D + c0, d0);
      if (two) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float y, gp;
          grn_gelu_both(v1[k] + b[k], y, gp);
          d1[k] = fmaf(d1[k], sc[k], y * tc[k]) * gp;
          acc[k] += d1[k];
        }
        cnx_store8<KIND, false>(du, (r + RB) * D + c0, d1);
      }
    }
  }
  grn_combine_slots(red, acc, part + (int64_t)blockIdx.x * D, W, RB, cl, rl, cb, D);
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
bool cnx_grn_supported(int64_t D) { return D > 0 && D % 8 == 0 && D / 8 <= 65535 * (int64_t)kBlock; }

static GrnGeom grn_geometry(int64_t N, int64_t R, int64_t D) {
  GrnGeom g;
  if (N < 1) N = 1;
  if (R < 1) R = 1;
  g.W =(int)(D / 8 < kBlock ? D / 8 : kBlock);
  g.RB = kBlock / g.W;
  g.cbk = (int)((D / 8 + g.W - 1) / g.W);
  const int64_t passes = (R + g.RB - 1) / g.RB;          // most slices: one per RB rows
  int64_t want = kGrnMaxBlocks / ((int64_t)g.cbk * N);   // slices per sample within the block budget
  if (want > passes) want = passes;
  if (want < 1) want = 1;
  int64_t rps = (R + want - 1) / want;
  rps = (rps + g.RB - 1) / g.RB * g.RB;
  g.rps = rps;
  g.sps = (int)((R + rps - 1) / rps);                    // no empty slice
  return g;
}

int cnx_grn_slices(int64_t N, int64_t R, int64_t D) { return grn_geometry(N, R, D).sps; }

void launch_cnx_grn_fwd(int kind, const uint16_t* u, const void* b1, int b1_kind, const float* gamma, const float* beta,
                        uint16_t* g, float* part, float* G, float* inv, float* s, int64_t N, int64_t R, int64_t D,
                        float eps, hipStream_t st) {
  const GrnGeom q = grn_geometry(N, R, D);
  const dim3 gr((unsigned)(N * q.sps), (unsigned)q.cbk), bl(kBlock);
  if (kind == 1)
    hipLaunchKernelGGL(grn_fwd_stats_kernel<1>, gr, bl, 0, st, u, b1, b1_kind, part, R, (int)D, q.W, q.sps, q.rps);
  else
    hipLaunchKernelGGL(grn_fwd_stats_kernel<2>, gr, bl, 0, st, u, b1, b1_kind, part, R, (int)D, q.W, q.sps, q.rps);
  hipLaunchKernelGGL(grn_fwd_finalize_kernel, dim3((unsigned)N), bl, 0, st, part, gamma, G, inv, s, (int)D, q.sps, eps);
  if (kind == 1)
    hipLaunchKernelGGL(grn_fwd_apply_kernel<1>, gr, bl, 0, st, u, b1, b1_kind, s, beta, g, R, (int)D, q.W, q.sps, q.rps);
  else
    hipLaunchKernelGGL(grn_fwd_apply_kernel<2>, gr, bl, 0, st, u, b1, b1_kind, s, beta, g, R, (int)D, q.W, q.sps, q.rps);
}

void launch_cnx_grn_bwd(int kind, const uint16_t* dg, const uint16_t* u, const void* b1, int b1_kind,
                        const float* gamma, const float* G, const float* inv, const float* s, uint16_t* du,
                        float* part, float* t, float* sn, int64_t N, int64_t R, int64_t D, hipStream_t st) {
  const GrnGeom q = grn_geometry(N, R, D);
  const dim3 gr((unsigned)(N * q.sps), (unsigned)q.cbk), bl(kBlock);
  if (kind == 1)
    hipLaunchKernelGGL(grn_bwd_stats_kernel<1>, gr, bl, 0, st, dg, u, b1, b1_kind, part, R, (int)D, q.W, q.sps, q.rps);
  else
    hipLaunchKernelGGL(grn_bwd_stats_kernel<2>, gr, bl, 0, st, dg, u, b1, b1_kind, part, R, (int)D, q.W, q.sps, q.rps);
  hipLaunchKernelGGL(grn_bwd_finalize_kernel, dim3((unsigned)N), bl, 0, st, part, gamma, G, inv, t, sn, (int)D, q.sps);
  // the apply sweep's partials reuse part[0]: the finalize kernel has consumed it (same stream)
  if (kind == 1)
    hipLaunchKernelGGL(grn_bwd_apply_kernel<1>, gr, bl, 0, st, dg, u, b1, b1_kind, s, t, du, part, R, (int)D, q.W, q.sps,
                       q.rps);
  else
    hipLaunchKernelGGL(grn_bwd_apply_kernel<2>, gr, bl, 0, st, dg, u, b1, b1_kind, s, t, du, part, R, (int)D, q.W, q.sps,
                       q.rps);
}

}  // namespace dpt
