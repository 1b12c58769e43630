// Layer-wise adaptive optimizers (LARS, LAMB) over a flat fp32 arena (gfx950).
//
// sgd_kernel / adam_kernel sweep the arena blindly; a trust ratio needs ||p|| and ||g|| (or ||u||)
// per parameter.  The host cuts every parameter ("segment") into chunks of kTrustChunk elements,
// counted from the segment's own start, so no chunk crosses a segment boundary (ops/trust.py):
//
//   chunk[c]            = (start, length, segment, 0)      elements; start % 4 == 0
//   seg_first/seg_count = the segment's chunks, contiguous and in order
//   seg_flags           = bit 0 adapt (apply the trust ratio), bit 1 decay (apply weight decay)
//
//   seg_partial : one workgroup per chunk (grid-strided): partial[c] = (sum p^2, sum g^2)
//   lamb_moment : LAMB's first pass: m, v update, g = 0, partial[c] = (sum p^2, sum u^2)
//   seg_finish  : one wave per segment: sums the segment's partials, writes ratio[segment]
//   lars_apply / lamb_apply : one workgroup per chunk (grid-strided), reads ratio[segment]
//
// Summation order is fixed and depends on nothing but the chunk's contents and its index within
// the segment: thread t adds the 16 squares of float4s t, t+256, t+512, t+768 of the chunk one
// after the other, the 64 lanes of a wave are added by a 6-level xor tree, the 4 waves by a 2-level
// tree through LDS; seg_finish's lane l adds chunks l, l+64, ... in order and the same 6-level tree
// joins the lanes.  No atomics, no arrival counters: the hand-off between the passes is the kernel
// boundary.  Results are therefore bitwise repeatable and independent of where a segment lies in
// the arena, which is what lets DDP re-lay the arena after the first backward.
//
// A chunk's last float4 may reach up to 3 elements past the segment's end: that padding is zero in
// p, g and all state and every update below maps zeros to zeros.
//
// scale / host_factor / found_inf / step / zero_grad / shadow behave as in optim_kernels.hip: when
// found_inf is set neither p nor any state changes, gradients are still zeroed.
//
// Bytes per parameter:  LARS  seg_partial reads p,g (8) + lars_apply reads p,g,buf writes p,buf,g (24)
//                       LAMB  lamb_moment reads p,g,m,v writes m,v,g (28) + lamb_apply reads p,m,v
//                             writes p (16)
#include "common.h"
#include "kernels.h"

namespace dpt {

struct LambCoef {
  float lr, beta2, one_m_beta1, one_m_beta2, eps, wd;
  double beta1_d, beta2_d;
};

namespace {

constexpr int kVecPerThread = kTrustChunk / 4 / kBlock;   // float4s per thread per chunk
static_assert(kTrustChunk == kVecPerThread * 4 * kBlock, "a chunk is a whole number of block sweeps");
constexpr int kWaves = kBlock / 64;

__device__ __forceinline__ void trust_shadow4(uint16_t* shadow, int kind, int64_t i, float4 v) {
  auto cv = [kind](float f) -> uint32_t {
    return kind == 1 ? (uint32_t)f32_to_bf16(f) : (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f);
  };
  uint2 w;
  w.x = cv(v.x) | (cv(v.y) << 16);
  w.y = cv(v.z) | (cv(v.w) << 16);
  reinterpret_cast<uint2*>(shadow)[i] = w;
}

// 6-level xor tree over the 64 lanes: every lane ends with the same sum.
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// Block sum of two values: wave trees, then the 4 waves' sums as (w0 + w1) + (w2 + w3).
// Returns the sums in thread 0.  lds: 2 * kWaves floats.
__device__ __forceinline__ void block_sum2(float& a, float& b, float* lds) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    lds[wave] = a;
    lds[kWaves + wave] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    static_assert(kWaves == 4, "two-level tree over four waves");
    a = (lds[0] + lds[1]) + (lds[2] + lds[3]);
    b = (lds[kWaves + 0] + lds[kWaves + 1]) + (lds[kWaves + 2] + lds[kWaves + 3]);
  }
  __syncthreads();   // lds is reused by the next chunk
}

__device__ __forceinline__ float sq4(float acc, float4 v) {
  acc += v.x * v.x;
  acc += v.y * v.y;
  acc += v.z * v.z;
  acc += v.w * v.w;
  return acc;
}

// LAMB's update direction; the moment pass and the apply pass both call this on the same stored
// p, m, v, with contraction off, so the two agree to the bit.
__device__ __forceinline__ float lamb_u(float p, float m, float v, float bc1, float bc2, float eps,
                                        float wd) {
#pragma clang fp contract(off)
  float r = (m / bc1) / (sqrtf(v / bc2) + eps);
  return r + wd * p;
}

}  // namespace

__global__ __launch_bounds__(kBlock) void seg_partial_kernel(const float4* __restrict__ p,
                                                             const float4* __restrict__ g,
                                                             const int4* __restrict__ chunks, int nchunks,
                                                             const float* scale, float host_factor,
                                                             float2* __restrict__ partial) {
  __shared__ float lds[2 * kWaves];
  const float f = grad_factor(scale, host_factor);
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int4 ch = chunks[c];
    const int64_t base = (int64_t)ch.x >> 2;
    const int nv = (ch.y + 3) >> 2;
    float4 pv[kVecPerThread], gv[kVecPerThread];
#pragma unroll
    for (int u = 0; u < kVecPerThread; ++u) {
      const int i = threadIdx.x + u * kBlock;
      const bool in = i < nv;
      pv[u] = in ? p[base + i] : make_float4(0.f, 0.f, 0.f, 0.f);
      gv[u] = in ? g[base + i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float sp = 0.f, sg = 0.f;
#pragma unroll
    for (int u = 0; u < kVecPerThread; ++u) {
      sp = sq4(sp, pv[u]);
      sg = sq4(sg, make_float4(gv[u].x * f, gv[u].y * f, gv[u].z * f, gv[u].w * f));
    }
    block_sum2(sp, sg, lds);
    if (threadIdx.x == 0) partial[c] = make_float2(sp, sg);
  }
}

// lamb != 0: ratio = ||p|| / ||u||;  else LARS: ratio = eta ||p|| / (||g|| + wd_i ||p||).
__global__ __launch_bounds__(kBlock) void seg_finish_kernel(const float2* __restrict__ partial,
                                                            const int* __restrict__ seg_first,
                                                            const int* __restrict__ seg_count,
                                                            const int* __restrict__ seg_flags, int nseg,
                                                            int lamb, float eta, float wd,
                                                            float* __restrict__ ratio) {
  const int seg = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (seg >= nseg) return;                       // whole waves leave: no barrier below
  const int lane = threadIdx.x & 63;
  const int first = seg_first[seg], count = seg_count[seg];
  float a = 0.f, b = 0.f;
  for (int k = lane; k < count; k += 64) {
    const float2 v = partial[first + k];
    a += v.x;
    b += v.y;
  }
  a = wave_sum(a);
  b = wave_sum(b);
  if (lane != 0) return;
  const int flags = seg_flags[seg];
  float r = 1.0f;
  if (flags & 1) {
    const float wn = sqrtf(a), xn = sqrtf(b);
    if (wn > 0.f && xn > 0.f) {
      if (lamb) {
        r = wn / xn;
      } else {
        const float wdi = (flags & 2) ? wd : 0.f;
        r = eta * wn / (xn + wdi * wn);
      }
    }
  }
  ratio[seg] = r;
}

template <bool NESTEROV>
__global__ __launch_bounds__(kBlock) void lars_apply_kernel(float4* __restrict__ p, float4* __restrict__ g,
                                                            float4* __restrict__ buf,
                                                            const int4* __restrict__ chunks, int nchunks,
                                                            const int* __restrict__ seg_flags,
                                                            const float* __restrict__ ratio, float lr,
                                                            float momentum, float wd, const float* scale,
                                                            float host_factor, const float* found_inf,
                                                            const float* step, int zero_grad,
                                                            uint16_t* __restrict__ shadow, int shadow_kind) {
  const bool skip = found_inf != nullptr && found_inf[0] != 0.0f;
  if (skip && !zero_grad) return;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const float f = grad_factor(scale, host_factor);
  const bool first = step == nullptr || step[0] == 0.0f;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int4 ch = chunks[c];
    const int64_t base = (int64_t)ch.x >> 2;
    const int nv = (ch.y + 3) >> 2;
    if (skip) {
#pragma unroll
      for (int u = 0; u < kVecPerThread; ++u) {
        const int i = threadIdx.x + u * kBlock;
        if (i < nv) g[base + i] = z;
      }
      continue;
    }
    const int flags = seg_flags[ch.z];
    const float r = ratio[ch.z];
    const float wdi = (flags & 2) ? wd : 0.f;
    float4 pv[kVecPerThread], gv[kVecPerThread], bv[kVecPerThread];
#pragma unroll
    for (int u = 0; u < kVecPerThread; ++u) {
      const int i = threadIdx.x + u * kBlock;
      if (i < nv) {
        pv[u] = p[base + i];
        gv[u] = g[base + i];
        if (!first) bv[u] = buf[base + i];
      }
    }
#pragma unroll
    for (int u = 0; u < kVecPerThread; ++u) {
      const int i = threadIdx.x + u * kBlock;
      if (i >= nv) continue;
      float* pp = reinterpret_cast<float*>(&pv[u]);
      float* gg = reinterpret_cast<float*>(&gv[u]);
      float* bb = reinterpret_cast<float*>(&bv[u]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = r * (gg[k] * f + wdi * pp[k]);
        bb[k] = first ? d : momentum * bb[k] + d;
        pp[k] = pp[k] - lr * (NESTEROV ? d + momentum * bb[k] : bb[k]);
      }
      p[base + i] = pv[u];
      if (shadow) trust_shadow4(shadow, shadow_kind, base + i, pv[u]);
      buf[base + i] = bv[u];
      if (zero_grad) g[base + i] = z;
    }
  }
}

__global__ __launch_bounds__(kBlock) void lamb_moment_kernel(const float4* __restrict__ p,
                                                             float4* __restrict__ g, float4* __restrict__ m,
                                                             float4* __restrict__ v,
                                                             const int4* __restrict__ chunks, int nchunks,
                                                             const int* __restrict__ seg_flags, LambCoef co,
                                                             const float* scale, float host_factor,
                                                             const float* found_inf, const float* step,
                                                             int zero_grad, float2* __restrict__ partial) {
  __shared__ float lds[2 * kWaves];
  const bool skip = found_inf != nullptr && found_inf[0] != 0.0f;
  if (skip && !zero_grad) return;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const float f = grad_factor(scale, host_factor);
  const double t = (double)(step ? step[0] : 0.0f) + 1.0;
  const float bc1 = (float)(1.0 - pow(co.beta1_d, t));
  const float bc2 = (float)(1.0 - pow(co.beta2_d, t));
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int4 ch = chunks[c];
    const int64_t base = (int64_t)ch.x >> 2;
    const int nv = (ch.y + 3) >> 2;
    if (skip) {                                   // uniform over the grid: no barrier is skipped
#pragma unroll
      for (int u = 0; u < kVecPerThread; ++u) {
        const int i = threadIdx.x + u * kBlock;
        if (i < nv) g[base + i] = z;
      }
      continue;
    }
    const float wdi = (seg_flags[ch.z] & 2) ? co.wd : 0.f;
    float4 pv[kVecPerThread], gv[kVecPerThread], mv[kVecPerThread], vv[kVecPerThread];
#pragma unroll
    for (int u = 0; u < kVecPerThread; ++u) {
      const int i = threadIdx.x + u * kBlock;
      if (i < nv) { pv[u] = p[base + i]; gv[u] = g[base + i]; mv[u] = m[base + i]; vv[u] = v[base + i]; }
    }
    float sp = 0.f, su = 0.f;
#pragma unroll
    for (int u = 0; u < kVecPerThread; ++u) {
      const int i = threadIdx.x + u * kBlock;
      if (i >= nv) continue;
      const float* pp = reinterpret_cast<const float*>(&pv[u]);
      const float* gg = reinterpret_cast<const float*>(&gv[u]);
      float* mm = reinterpret_cast<float*>(&mv[u]);
      float* vq = reinterpret_cast<float*>(&vv[u]);
      float4 uv;
      float* uu = reinterpret_cast<float*>(&uv);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float gr = gg[k] * f;
        mm[k] = mm[k] + co.one_m_beta1 * (gr - mm[k]);
        vq[k] = co.beta2 * vq[k] + co.one_m_beta2 * gr * gr;
        uu[k] = lamb_u(pp[k], mm[k], vq[k], bc1, bc2, co.eps, wdi);
      }
      m[base + i] = mv[u];
      v[base + i] = vv[u];
      if (zero_grad) g[base + i] = z;
      sp = sq4(sp, pv[u]);
      su = sq4(su, uv);
    }
    block_sum2(sp, su, lds);
    if (threadIdx.x == 0) partial[c] = make_float2(sp, su);
  }
}

__global__ __launch_bounds__(kBlock) void lamb_apply_kernel(float4* __restrict__ p,
                                                            const float4* __restrict__ m,
                                                            const float4* __restrict__ v,
                                                            const int4* __restrict__ chunks, int nchunks,
                                                            const int* __restrict__ seg_flags,
                                                            const float* __restrict__ ratio, LambCoef co,
                                                            const float* found_inf, const float* step,
                                                            uint16_t* __restrict__ shadow, int shadow_kind) {
  if (found_inf != nullptr && found_inf[0] != 0.0f) return;
  const double t = (double)(step ? step[0] : 0.0f) + 1.0;
  const float bc1 = (float)(1.0 - pow(co.beta1_d, t));
  const float bc2 = (float)(1.0 - pow(co.beta2_d, t));
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int4 ch = chunks[c];
    const int64_t base = (int64_t)ch.x >> 2;
    const int nv = (ch.y + 3) >> 2;
    const float wdi = (seg_flags[ch.z] & 2) ? co.wd : 0.f;
    const float lrr = co.lr * ratio[ch.z];
    float4 pv[kVecPerThread], mv[kVecPerThread], vv[kVecPerThread];
#pragma unroll
    for (int u = 0; u < kVecPerThread; ++u) {
      const int i = threadIdx.x + u * kBlock;
      if (i < nv) { pv[u] = p[base + i]; mv[u] = m[base + i]; vv[u] = v[base + i]; }
    }
#pragma unroll
    for (int u = 0; u < kVecPerThread; ++u) {
      const int i = threadIdx.x + u * kBlock;
      if (i >= nv) continue;
      float* pp = reinterpret_cast<float*>(&pv[u]);
      const float* mm = reinterpret_cast<const float*>(&mv[u]);
      const float* vq = reinterpret_cast<const float*>(&vv[u]);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        pp[k] = pp[k] - lrr * lamb_u(pp[k], mm[k], vq[k], bc1, bc2, co.eps, wdi);
      p[base + i] = pv[u];
      if (shadow) trust_shadow4(shadow, shadow_kind, base + i, pv[u]);
    }
  }
}

// ------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------
namespace {

int chunk_grid(int nchunks) { return nchunks < kMaxBlocks ? nchunks : kMaxBlocks; }

void launch_finish(const TrustTable& tb, bool lamb, float eta, float wd, hipStream_t s) {
  hipLaunchKernelGGL(seg_finish_kernel, dim3((tb.nseg + kWaves - 1) / kWaves), dim3(kBlock), 0, s,
                     reinterpret_cast<const float2*>(tb.partial), tb.seg_first, tb.seg_count,
                     tb.seg_flags, tb.nseg, (int)lamb, eta, wd, tb.ratio);
}

}  // namespace

void launch_lars(float* p, float* g, float* buf, const TrustTable& tb, float lr, float momentum, float wd,
                 float eta, bool nesterov, const float* scale, float host_factor, const float* found_inf,
                 const float* step, bool zero_grad, uint16_t* shadow, int shadow_kind, hipStream_t s) {
  if (tb.nchunks == 0 || tb.nseg == 0) return;
  dim3 grid(chunk_grid(tb.nchunks)), block(kBlock);
  auto P = reinterpret_cast<float4*>(p);
  auto G = reinterpret_cast<float4*>(g);
  auto B = reinterpret_cast<float4*>(buf);
  auto CH = reinterpret_cast<const int4*>(tb.chunks);
  hipLaunchKernelGGL(seg_partial_kernel, grid, block, 0, s, P, G, CH, tb.nchunks, scale, host_factor,
                     reinterpret_cast<float2*>(tb.partial));
  launch_finish(tb, false, eta, wd, s);
  if (nesterov)
    hipLaunchKernelGGL((lars_apply_kernel<true>), grid, block, 0, s, P, G, B, CH, tb.nchunks, tb.seg_flags,
                       tb.ratio, lr, momentum, wd, scale, host_factor, found_inf, step, (int)zero_grad,
                       shadow, shadow_kind);
  else
    hipLaunchKernelGGL((lars_apply_kernel<false>), grid, block, 0, s, P, G, B, CH, tb.nchunks, tb.seg_flags,
                       tb.ratio, lr, momentum, wd, scale, host_factor, found_inf, step, (int)zero_grad,
                       shadow, shadow_kind);
}

void launch_lamb(float* p, float* g, float* m, float* v, const TrustTable& tb, double lr, double beta1,
                 double beta2, double eps, double wd, const float* scale, float host_factor,
                 const float* found_inf, const float* step, bool zero_grad, uint16_t* shadow,
                 int shadow_kind, hipStream_t s) {
  if (tb.nchunks == 0 || tb.nseg == 0) return;
  dim3 grid(chunk_grid(tb.nchunks)), block(kBlock);
  auto P = reinterpret_cast<float4*>(p);
  auto G = reinterpret_cast<float4*>(g);
  auto M = reinterpret_cast<float4*>(m);
  auto V = reinterpret_cast<float4*>(v);
  auto CH = reinterpret_cast<const int4*>(tb.chunks);
  LambCoef co;
  co.lr = (float)lr;
  co.beta2 = (float)beta2;
  co.one_m_beta1 = (float)(1.0 - beta1);
  co.one_m_beta2 = (float)(1.0 - beta2);
  co.eps = (float)eps;
  co.wd = (float)wd;
  co.beta1_d = beta1;
  co.beta2_d = beta2;
  hipLaunchKernelGGL(lamb_moment_kernel, grid, block, 0, s, P, G, M, V, CH, tb.nchunks, tb.seg_flags, co,
                     scale, host_factor, found_inf, step, (int)zero_grad,
                     reinterpret_cast<float2*>(tb.partial));
  launch_finish(tb, true, 0.f, co.wd, s);
  hipLaunchKernelGGL(lamb_apply_kernel, grid, block, 0, s, P, M, V, CH, tb.nchunks, tb.seg_flags, tb.ratio,
                     co, found_inf, step, shadow, shadow_kind);
}

}  // namespace dpt
