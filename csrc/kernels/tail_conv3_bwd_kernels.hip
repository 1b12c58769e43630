// Bottleneck tail's backward apply fused into conv3's backward-data, for gfx950.
//
// Why: in a bottleneck's backward the tail's apply pass writes dx3 = k1*dz + k2*(x3 - mean) + k3
// (bn_bwd_apply_kernel FROM_DZ, or bn_bwd_apply2_kernel with a downsample BatchNorm) and conv3's
// backward-data (conv_fwd_kernel with the BNB epilogue on the flipped weight, 4C -> C channels) reads
// all of dx3 back after the backward-weight has read it once.  In ResNet-50's layer1 and layer2 at
// batch 256 dx3 is 411 MB / 205 MB - it does not survive in the Infinity Cache - so that read is a
// second HBM pass over values that were in registers a moment earlier (docs/DESIGN.md §19).  This
// kernel is the streaming apply pass that also feeds the small GEMM: one block forms 128 rows of dx3
// a 64-channel K-step at a time, stores them (the backward-weight still needs them) and writes the
// same rounded bits into the LDS A tile of the MFMA loop.
//
// Per K-step and thread: four 16-byte chunks of dz and x3 (and of the downsample BatchNorm's input
// with TWO), each re-issued for the next K-step as soon as it is unpacked; dx3 (and dx_ds) with exactly
// the arithmetic and rounding of the apply kernels; a global store of each chunk; ds_write_b128 of
// dx3 into the XOR-swizzled A tile; the flipped-weight K-slice is register-staged the same way.
// [k1 | k2 | k3 | mean] (and [j1 | j2 | j3 | mean2]) sit in LDS, staged once per block.
//
// The [M, C] gradient and bp1/bp2 are bit-equal to conv_fwd_kernel<128, BN, 1, LDSEPI, BNB> (STATS
// off): the tile, the MFMA order and the rounded LDS image are tail_tile.h's; here, the mask
// fma(x, a, b) > 0 from bn2's input, s1/s2 summed over a thread's rows in ascending order, shfl_xor
// CPR..32, waves summed in index order.  One 128-row tile per block, plain grid, no inter-block
// communication.
#include <stdexcept>
#include <string>
#include <type_traits>

#include "bn_io.h"
#include "common.h"
#include "kernels.h"
#include "mfma.h"
#include "tail_tile.h"

namespace dpt {

namespace tc3 {
using namespace tail;

// K-loop image (A tile, B tile, coefficients) and the epilogue image share the front of the LDS
template <int BN>
__host__ __device__ constexpr int lds_bytes(int C4, bool two) {
  const int main = tile_bytes(BN) + (two ? 8 : 4) * C4 * 4, epi = image_bytes(BN);
  return main > epi ? main : epi;
}
}  // namespace tc3

template <typename IO, int BN, bool TWO>
__global__ __launch_bounds__(tail::kThreads, 2) void tail_conv3_bwd_kernel(TailConv3BwdArgs p) {
  using namespace tc3;
  constexpr bool F16V = std::is_same<IO, F16>::value;
  using T = Tile<F16V, BN>;
  constexpr int B_PER_T = T::B_PER_T, C_STRIDE = T::C_STRIDE;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  float* lc = reinterpret_cast<float*>(lds + tile_bytes(BN));  // [k1 | k2 | k3 | mean | j1 | j2 | j3 | mean2][C4]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int C4 = p.C4, nk = C4 / BK;
  const Rows t(p.M, C4, p.m_tiles, p.rev);
  const int mt = t.mt, c = t.c, rb = t.rb;
  const int64_t m0 = t.m0;

  const uint32_t nbytes = (uint32_t)(p.M * C4 * 2);
  const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)p.dz, 0, (int)nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x3, 0, (int)nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t r2 =
      __builtin_amdgcn_make_buffer_rsrc((void*)(TWO ? p.x2 : p.x3), 0, (int)nbytes, 0x00020000);
  // dx3 and dx_ds have dz's layout: the loads' byte offsets serve the stores; the weight rows go
  // through a descriptor too (32-bit offsets: no 64-bit address per row and chunk kept in VGPRs)
  const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)p.dx3, 0, (int)nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t re =
      __builtin_amdgcn_make_buffer_rsrc((void*)(TWO ? p.dx_ds : p.dx3), 0, (int)nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.wt, 0, (int)((uint32_t)BN * (uint32_t)C4 * 2u), 0x00020000);
  const uint32_t woff = (uint32_t)((rb * C4 + c * 8) * 2);  // row rb; rows rb + 32i are 64 * C4 bytes apart

  u32x4 ga[4], xa[4], qa[4];
  u32x4 wb[B_PER_T];
  auto load_g = [&](int i, int ks) { ga[i] = __builtin_amdgcn_raw_buffer_load_b128(rg, t.off(i, ks), 0, 0); };
  auto load_x = [&](int i, int ks) { xa[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, t.off(i, ks), 0, 0); };
  auto load_q = [&](int i, int ks) { qa[i] = __builtin_amdgcn_raw_buffer_load_b128(r2, t.off(i, ks), 0, 0); };
  auto load_a = [&](int i, int ks) {
    load_g(i, ks);
    load_x(i, ks);
    if (TWO) load_q(i, ks);
  };
  auto load_b = [&](int ks) {
#pragma unroll
    for (int i = 0; i < B_PER_T; ++i)
      wb[i] = __builtin_amdgcn_raw_buffer_load_b128(rw, woff + (uint32_t)(i * 64 * C4), ks * kRowBytes, 0);
  };
#pragma unroll
  for (int i = 0; i < 4; ++i) load_a(i, 0);
  load_b(0);
  for (int i = tid; i < 3 * C4; i += kThreads) {
    lc[i] = p.k[i];
    if (TWO) lc[4 * C4 + i] = p.j[i];
  }
  for (int i = tid; i < C4; i += kThreads) {
    lc[3 * C4 + i] = p.mean[i];
    if (TWO) lc[7 * C4 + i] = p.mean2[i];
  }

  typename T::Acc acc;
  T::zero(acc);

  __syncthreads();  // the coefficients are staged
  for (int ks = 0; ks < nk; ++ks) {
    const bool more = ks + 1 < nk;
    const int ch0 = ks * BK + c * 8;
    u32x4 dv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float g[8], v[8];
      unpack8<IO>(ga[i], g);
      unpack8<IO>(xa[i], v);
      // the registers are free again: the next K-step's chunks are in flight from here, while the
      // rest of this K-step is applied, staged and multiplied
      if (more) load_x(i, ks + 1);
      if (more && !TWO) load_g(i, ks + 1);
      uint32_t h[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        // the expression of bn_bwd_apply_kernel / bn_bwd_apply2_kernel (bn_io.h)
        const float k1 = lc[ch0 + k], k2 = lc[C4 + ch0 + k], k3 = lc[2 * C4 + ch0 + k], mu = lc[3 * C4 + ch0 + k];
        h[k] = down16<IO>(bn_bwd_dx(k1, g[k], k2, v[k], mu, k3));
      }
      dv[i] = pack8(h);
      if (t.live[i]) __builtin_amdgcn_raw_buffer_store_b128(dv[i], rd, t.voff[i], ks * kRowBytes, 0);
      else dv[i] = u32x4{0u, 0u, 0u, 0u};  // rows past M are zero rows of the GEMM
    }
    if (ks > 0) __syncthreads();  // every wave has multiplied the previous K-step
    T::stage(lds, dv, wb);
    if constexpr (TWO) {
      // the downsample branch's gradient (the second expression of bn_bwd_apply2_kernel) feeds no GEMM
      // here; a pass of its own after the A and B tiles are staged (their registers are free) that the
      // scheduler may not mix with its neighbours, so that only one BatchNorm's coefficients are live
      // at a time (both, next to the staged tiles: spills at BN = 128)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float g[8], q[8];
        unpack8<IO>(ga[i], g);
        unpack8<IO>(qa[i], q);
        if (more) load_g(i, ks + 1);
        if (more) load_q(i, ks + 1);
        uint32_t h2[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float j1 = lc[4 * C4 + ch0 + k], j2 = lc[5 * C4 + ch0 + k], j3 = lc[6 * C4 + ch0 + k],
                      mu2 = lc[7 * C4 + ch0 + k];
          h2[k] = down16<IO>(bn_bwd_dx(j1, g[k], j2, q[k], mu2, j3));
        }
        if (t.live[i]) __builtin_amdgcn_raw_buffer_store_b128(pack8(h2), re, t.voff[i], ks * kRowBytes, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (more) load_b(ks + 1);
    __syncthreads();
    T::mma(lds, acc);
  }
  __syncthreads();  // the epilogue reuses the LDS

  // ---- the LDS image of tail_tile.h with the BNB sums of conv_fwd_kernel's epilogue ----
  T::image(lds, acc, [](int, uint32_t) {});
  __syncthreads();
  constexpr int CPR = T::CPR, RPP = T::RPP, NPASS = T::NPASS, GRP = 4;
  static_assert(NPASS % GRP == 0, "whole groups of passes");
  const int oc = tid % CPR, orow = tid / CPR;
  float ba[8], bb[8], bm[8], s1[8], s2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int ch = oc * 8 + k;
    ba[k] = p.bn_coef[ch];
    bb[k] = p.bn_coef[BN + ch];
    bm[k] = p.bn_mean[ch];
    s1[k] = 0.f;
    s2[k] = 0.f;
  }
#pragma unroll
  for (int g0 = 0; g0 < NPASS; g0 += GRP) {
    uint4 xv[GRP];
#pragma unroll
    for (int q = 0; q < GRP; ++q) {
      const int64_t m = m0 + (g0 + q) * RPP + orow;
      xv[q] = *reinterpret_cast<const uint4*>(p.bnx + (m < p.M ? m : 0) * BN + oc * 8);
    }
#pragma unroll
    for (int q = 0; q < GRP; ++q) {
      const int row = (g0 + q) * RPP + orow;
      const int64_t m = m0 + row;
      if (m < p.M) {
        const uint4 v = *reinterpret_cast<const uint4*>(lds + row * C_STRIDE + oc * 16);
        const uint32_t gu[4] = {v.x, v.y, v.z, v.w};
        const uint32_t xu[4] = {xv[q].x, xv[q].y, xv[q].z, xv[q].w};
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int k = 2 * k2 + h;
            const float g = cunpack<F16V>(gu[k2], h);
            const float x = cunpack<F16V>(xu[k2], h);
            const float dz = __builtin_fmaf(x, ba[k], bb[k]) > 0.0f ? g : 0.0f;
            s1[k] += dz;
            s2[k] = __builtin_fmaf(dz, x - bm[k], s2[k]);
          }
        *reinterpret_cast<uint4*>(p.dx + m * BN + oc * 8) = v;  // (the unmasked gradient, as BNB stores it)
      }
    }
  }
  // threads sharing a channel group: lanes l, l + CPR, ... of a wave, then the four waves through LDS
#pragma unroll
  for (int k = 0; k < 8; ++k) {
#pragma unroll
    for (int off = CPR; off < 64; off <<= 1) {
      s1[k] += __shfl_xor(s1[k], off, 64);
      s2[k] += __shfl_xor(s2[k], off, 64);
    }
  }
  __syncthreads();
  float* bred = reinterpret_cast<float*>(lds);  // [4 waves][2][BN]
  if (lane < CPR) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      bred[(wid * 2) * BN + oc * 8 + k] = s1[k];
      bred[(wid * 2 + 1) * BN + oc * 8 + k] = s2[k];
    }
  }
  __syncthreads();
  if (tid < BN) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      a += bred[(w * 2) * BN + tid];
      b += bred[(w * 2 + 1) * BN + tid];
    }
    p.bp1[(int64_t)tid * p.m_tiles + mt] = a;
    p.bp2[(int64_t)tid * p.m_tiles + mt] = b;
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static size_t tail_conv3_lds(int C4, int C, bool two) {
  return C == 128 ? tc3::lds_bytes<128>(C4, two) : tc3::lds_bytes<64>(C4, two);
}

const char* tail_conv3_bwd_refusal(int64_t M, int64_t C4, int64_t C) {
  if (const char* why = tail_tile_refusal(M, C4, C, "needs 4C % 64 == 0 and 4C >= 64",
                                          "needs C of 64 or 128 (one output-channel tile)"))
    return why;
  if (tail_conv3_lds((int)C4, (int)C, true) > 65536) return "the coefficients do not fit the LDS";
  // only where the unfused backward-data runs the tile this kernel reproduces
  return conv_dgrad_bnb_plain_tile_refusal(M, (int)C, C4);
}

void launch_tail_conv3_bwd(bool f16, TailConv3BwdArgs a, int C, hipStream_t s) {
  if (const char* why = tail_conv3_bwd_refusal(a.M, a.C4, C)) throw std::runtime_error(std::string("tail_conv3_bwd: ") + why);
  const bool two = a.x2 != nullptr;
  if (two && (a.mean2 == nullptr || a.dx_ds == nullptr)) throw std::runtime_error("tail_conv3_bwd: x2 needs mean2 and dx_ds");
  a.j = two ? a.k + 3 * (int64_t)a.C4 : nullptr;
  a.m_tiles = conv_m_tiles(a.M);
  a.rev = kTailReverse;
  const dim3 grid((unsigned)a.m_tiles), block(tail::kThreads);
  const size_t lds = tail_conv3_lds(a.C4, C, two);
  tail_dispatch(f16, C == 128, two, [&](auto h, auto w, auto t) {
    hipLaunchKernelGGL((tail_conv3_bwd_kernel<std::conditional_t<h.value, F16, BF16>, w.value ? 128 : 64, t.value>), grid,
                       block, lds, s, a);
  });
}

}  // namespace dpt
