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
// off): the same wave tiling (4x1 waves at BN = 64, 2x2 at BN = 128), v_mfma_f32_32x32x16 with ks and
// kk ascending, the cvt_pk rounding of the epilogue, the mask fma(x, a, b) > 0 from bn2's input, s1/s2
// summed over a thread's rows in ascending order, shfl_xor CPR..32, waves summed in index order.
// One 128-row tile per block, plain grid, no inter-block communication.
#include <stdexcept>
#include <string>
#include <type_traits>

#include "bn_io.h"
#include "common.h"
#include "kernels.h"
#include "mfma.h"

namespace dpt {

namespace tc3 {
constexpr int BM = 128;
constexpr int BK = 64;
constexpr int kThreads = 256;
constexpr int kRowBytes = BK * 2;
constexpr int A_BYTES = BM * kRowBytes;
constexpr uint32_t kOOB = 0xFFFFFF00u;  // past every descriptor's range: the load returns zeros

__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

// K-loop image (A tile, B tile, coefficients) and the epilogue image share the front of the LDS
template <int BN>
__host__ __device__ constexpr int lds_bytes(int C4, bool two) {
  const int main = A_BYTES + BN * kRowBytes + (two ? 8 : 4) * C4 * 4, epi = BM * (BN * 2 + 16);
  return main > epi ? main : epi;
}
}  // namespace tc3

struct TailConv3BwdArgs {
  const uint16_t* dz = nullptr;    // [M, C4] the tail's masked output gradient
  const uint16_t* x3 = nullptr;    // [M, C4] the tail BatchNorm's input
  const uint16_t* x2 = nullptr;    // [M, C4] the downsample BatchNorm's input (TWO)
  const float* k = nullptr;        // [k1 | k2 | k3], 3 * C4 (the finalize's kbuf)
  const float* mean = nullptr;     // [C4]
  const float* j = nullptr;        // [j1 | j2 | j3] (TWO)
  const float* mean2 = nullptr;    // [C4] (TWO)
  const uint16_t* wt = nullptr;    // [C][C4] conv3's flipped weight
  uint16_t* dx3 = nullptr;         // [M, C4]
  uint16_t* dx_ds = nullptr;       // [M, C4] (TWO)
  const uint16_t* bnx = nullptr;   // [M, C] bn2's input
  const float* bn_mean = nullptr;  // [C]
  const float* bn_coef = nullptr;  // [a | b], 2 * C
  uint16_t* dx = nullptr;          // [M, C] conv3's input gradient
  float* bp1 = nullptr;            // [C][m_tiles]
  float* bp2 = nullptr;
  int64_t M = 0;
  int C4 = 0, m_tiles = 0, rev = 0;
};

// the conversions of IO::load8 / IO::store8, an element at a time
template <typename IO>
struct Cvt16;
template <>
struct Cvt16<BF16> {
  __device__ static float up(uint32_t h) { return bf16_to_f32((uint16_t)h); }
  __device__ static uint32_t down(float v) { return f32_to_bf16(v); }
};
template <>
struct Cvt16<F16> {
  __device__ static float up(uint32_t h) { return f16_to_f32((uint16_t)h); }
  __device__ static uint32_t down(float v) { return F16::to16(v); }
};

template <typename IO, int BN, bool TWO>
__global__ __launch_bounds__(tc3::kThreads, 2) void tail_conv3_bwd_kernel(TailConv3BwdArgs p) {
  using namespace tc3;
  constexpr bool F16V = std::is_same<IO, F16>::value;
  constexpr int WN = BN / 64, WM = 4 / WN, MI = BM / (WM * 32), NI = 2;
  constexpr int B_PER_T = BN * 8 / kThreads;  // weight chunks per thread and K-step
  constexpr int C_STRIDE = BN * 2 + 16;
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* la = lds;
  unsigned char* lb = lds + A_BYTES;
  float* lc = reinterpret_cast<float*>(lds + A_BYTES + BN * kRowBytes);  // [k1 | k2 | k3 | mean | j1 | j2 | j3 | mean2][C4]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int lr = lane & 31, lh = lane >> 5;
  const int mt = p.rev ? p.m_tiles - 1 - (int)blockIdx.x : (int)blockIdx.x;
  const int64_t m0 = (int64_t)mt * BM;
  const int C4 = p.C4, nk = C4 / BK;

  // this thread's chunks: column c (8 channels) of rows rb, rb + 32, rb + 64, rb + 96
  const int c = tid & 7, rb = tid >> 3;
  const uint32_t nbytes = (uint32_t)(p.M * C4 * 2);
  const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)p.dz, 0, (int)nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x3, 0, (int)nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t r2 =
      __builtin_amdgcn_make_buffer_rsrc((void*)(TWO ? p.x2 : p.x3), 0, (int)nbytes, 0x00020000);
  uint32_t voff[4];
  bool live[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + rb + 32 * i;
    live[i] = m < p.M;
    voff[i] = live[i] ? (uint32_t)((m * C4 + c * 8) * 2) : kOOB;
  }
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
  auto aoff = [&](int i, int ks) { return live[i] ? voff[i] + (uint32_t)ks * kRowBytes : kOOB; };
  auto load_g = [&](int i, int ks) { ga[i] = __builtin_amdgcn_raw_buffer_load_b128(rg, aoff(i, ks), 0, 0); };
  auto load_x = [&](int i, int ks) { xa[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, aoff(i, ks), 0, 0); };
  auto load_q = [&](int i, int ks) { qa[i] = __builtin_amdgcn_raw_buffer_load_b128(r2, aoff(i, ks), 0, 0); };
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
  auto unpack = [&](const u32x4& w, float f[8]) {
    const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = Cvt16<IO>::up(k & 1 ? u[k >> 1] >> 16 : u[k >> 1] & 0xffffu);
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

  f32x16_t acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  __syncthreads();  // the coefficients are staged
  for (int ks = 0; ks < nk; ++ks) {
    const bool more = ks + 1 < nk;
    const int ch0 = ks * BK + c * 8;
    u32x4 dv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float g[8], v[8];
      unpack(ga[i], g);
      unpack(xa[i], v);
      // the registers are free again: the next K-step's chunks are in flight from here, while the
      // rest of this K-step is applied, staged and multiplied
      if (more) load_x(i, ks + 1);
      if (more && !TWO) load_g(i, ks + 1);
      uint32_t h[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        // the expression of bn_bwd_apply_kernel / bn_bwd_apply2_kernel (bn_io.h)
        const float k1 = lc[ch0 + k], k2 = lc[C4 + ch0 + k], k3 = lc[2 * C4 + ch0 + k], mu = lc[3 * C4 + ch0 + k];
        h[k] = Cvt16<IO>::down(bn_bwd_dx(k1, g[k], k2, v[k], mu, k3));
      }
      dv[i] = u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
      if (live[i]) __builtin_amdgcn_raw_buffer_store_b128(dv[i], rd, voff[i], ks * kRowBytes, 0);
      else dv[i] = u32x4{0u, 0u, 0u, 0u};  // rows past M are zero rows of the GEMM
    }
    if (ks > 0) __syncthreads();  // every wave has multiplied the previous K-step
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = rb + 32 * i;
      *reinterpret_cast<u32x4*>(la + row * kRowBytes + swz(row, c) * 16) = dv[i];
    }
#pragma unroll
    for (int i = 0; i < B_PER_T; ++i) {
      const int row = rb + 32 * i;
      *reinterpret_cast<u32x4*>(lb + row * kRowBytes + swz(row, c) * 16) = wb[i];
    }
    if constexpr (TWO) {
      // the downsample branch's gradient (the second expression of bn_bwd_apply2_kernel) feeds no GEMM
      // here; a pass of its own after the A and B tiles are staged (their registers are free) that the
      // scheduler may not mix with its neighbours, so that only one BatchNorm's coefficients are live
      // at a time (both, next to the staged tiles: spills at BN = 128)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float g[8], q[8];
        unpack(ga[i], g);
        unpack(qa[i], q);
        if (more) load_g(i, ks + 1);
        if (more) load_q(i, ks + 1);
        uint32_t h2[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float j1 = lc[4 * C4 + ch0 + k], j2 = lc[5 * C4 + ch0 + k], j3 = lc[6 * C4 + ch0 + k],
                      mu2 = lc[7 * C4 + ch0 + k];
          h2[k] = Cvt16<IO>::down(bn_bwd_dx(j1, g[k], j2, q[k], mu2, j3));
        }
        if (live[i])
          __builtin_amdgcn_raw_buffer_store_b128(
              u32x4{h2[0] | (h2[1] << 16), h2[2] | (h2[3] << 16), h2[4] | (h2[5] << 16), h2[6] | (h2[7] << 16)}, re,
              voff[i], ks * kRowBytes, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (more) load_b(ks + 1);
    __syncthreads();
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
  __syncthreads();  // the epilogue reuses the LDS

  // ---- epilogue of conv_fwd_kernel (LDS image, BNB), operation for operation ----
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
      }
    }
  __syncthreads();
  constexpr int CPR = BN / 8, RPP = kThreads / CPR, NPASS = BM / RPP, GRP = 4;
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
  if (C4 < 64 || C4 % 64 != 0) return "needs 4C % 64 == 0 and 4C >= 64";
  if (C != 64 && C != 128) return "needs C of 64 or 128 (one output-channel tile)";
  if (M < 1) return "empty input";
  // 32-bit byte offsets through buffer descriptors, as conv_fwd_kernel (conv_check_offsets)
  if (M * C4 * 2 >= 0xFFFFFF00ll || C * C4 * 2 >= 0x7FFFFFFFll) return "operand tensors beyond 2^31 elements";
  if (tail_conv3_lds((int)C4, (int)C, true) > 65536) return "the coefficients do not fit the LDS";
  // only where the unfused backward-data runs the tile this kernel reproduces
  return conv_dgrad_bnb_plain_tile_refusal(M, (int)C, C4);
}

template <typename IO>
static void tail_conv3_dispatch(const TailConv3BwdArgs& a, int C, bool two, hipStream_t s) {
  const dim3 grid((unsigned)a.m_tiles), block(tc3::kThreads);
  const size_t lds = tail_conv3_lds(a.C4, C, two);
#define DPT_TC3(BN, TWOV) \
  hipLaunchKernelGGL((tail_conv3_bwd_kernel<IO, BN, TWOV>), grid, block, lds, s, a)
  if (C == 128) { if (two) DPT_TC3(128, true); else DPT_TC3(128, false); }
  else { if (two) DPT_TC3(64, true); else DPT_TC3(64, false); }
#undef DPT_TC3
}

// Apply passes walk the rows last-to-first (bn_kernels.hip kBnReverse): the rows the producing
// backward-data wrote last are still in the caches.  The fused kernel takes its M-tiles in the same order.
constexpr int kTail3Reverse = 1;

void launch_tail_conv3_bwd(bool f16, const uint16_t* dz, const uint16_t* x3, const uint16_t* x2, const float* kbuf,
                           const float* mean, const float* mean2, const uint16_t* wt, uint16_t* dx3, uint16_t* dx_ds,
                           const uint16_t* bnx, const float* bn_mean, const float* bn_coef, uint16_t* dx, float* bp1,
                           float* bp2, int64_t M, int C4, int C, hipStream_t s) {
  if (const char* why = tail_conv3_bwd_refusal(M, C4, C)) throw std::runtime_error(std::string("tail_conv3_bwd: ") + why);
  const bool two = x2 != nullptr;
  if (two && (mean2 == nullptr || dx_ds == nullptr)) throw std::runtime_error("tail_conv3_bwd: x2 needs mean2 and dx_ds");
  TailConv3BwdArgs a;
  a.dz = dz; a.x3 = x3; a.x2 = x2; a.k = kbuf; a.mean = mean; a.j = two ? kbuf + 3 * (int64_t)C4 : nullptr;
  a.mean2 = mean2; a.wt = wt; a.dx3 = dx3; a.dx_ds = dx_ds; a.bnx = bnx; a.bn_mean = bn_mean; a.bn_coef = bn_coef;
  a.dx = dx; a.bp1 = bp1; a.bp2 = bp2; a.M = M; a.C4 = C4; a.m_tiles = conv_m_tiles(M); a.rev = kTail3Reverse;
  if (f16) tail_conv3_dispatch<F16>(a, C, two, s);
  else tail_conv3_dispatch<BF16>(a, C, two, s);
}

}  // namespace dpt
