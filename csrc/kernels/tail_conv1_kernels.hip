// Bottleneck tail apply fused into the next block's 1x1 forward conv, for gfx950.
//
// Why: a bottleneck tail writes y = relu(bn3(x3) + identity) with bn_fwd_apply_kernel and the next
// block's conv1 (1x1 / stride 1, 4C -> C channels) reads all of y back.  In ResNet-50's layer1 and
// layer2 at batch 256 y is 411 MB / 205 MB - larger than what stays in the Infinity Cache between the
// two kernels - so the conv's read is a second HBM pass over values that were in registers a moment
// earlier (docs/DESIGN.md §17).  This kernel is the streaming apply pass that also feeds the small
// GEMM: one block forms 128 rows of y a 64-channel K-step at a time, stores them (and the 1-bit
// ReLU mask), and writes the same rounded bits into the LDS A tile of the MFMA loop.
//
// Per K-step and thread: four 16-byte chunks of x3 and of the residual (each re-issued for the next
// K-step as soon as it is unpacked), y with exactly the arithmetic of bn_fwd_apply_kernel (bn_io.h
// rounding), a global store of the y chunk, ds_write_b128 into the XOR-swizzled A tile; the weight
// K-slice is register-staged the same way.  The coefficients [a | b] (and [a2 | b2]) sit in LDS,
// staged once per block; the tile's mask bytes are gathered in LDS and stored as whole rows at the end.
//
// x1, psum and psq are bit-equal to conv_fwd_kernel<128, BN, 1, LDSEPI, STATS>: the same wave tiling
// (4x1 waves at BN = 64, 2x2 at BN = 128), v_mfma_f32_32x32x16 with ks and kk ascending, the cvt_pk
// rounding of the epilogue, per-lane f0 + f1 / fma sums, shfl_xor 32, waves summed in index order.
// One 128-row tile per block, plain grid, no inter-block communication.
#include <stdexcept>
#include <string>
#include <type_traits>

#include "bn_io.h"
#include "common.h"
#include "kernels.h"
#include "mfma.h"

namespace dpt {

namespace tc1 {
constexpr int BM = 128;
constexpr int BK = 64;
constexpr int kThreads = 256;
constexpr int kRowBytes = BK * 2;
constexpr int A_BYTES = BM * kRowBytes;
constexpr uint32_t kOOB = 0xFFFFFF00u;  // past every descriptor's range: the load returns zeros

__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

template <int BN>
__host__ __device__ constexpr int lds_epi() { return BM * (BN * 2 + 16) + 2 * (4 / (BN / 64)) * BN * 4; }
// K-loop image (A tile, B tile, coefficients) and the epilogue image share the front of the LDS
template <int BN>
__host__ __device__ constexpr int lds_main(int Cin, bool aff) {
  const int main = A_BYTES + BN * kRowBytes + (aff ? 4 : 2) * Cin * 4, epi = lds_epi<BN>();
  return main > epi ? main : epi;
}
}  // namespace tc1

struct TailConv1Args {
  const uint16_t* x3 = nullptr;   // [M, Cin] the tail BatchNorm's input
  const uint16_t* r = nullptr;    // [M, Cin] the residual, or (AFF) the downsample BatchNorm's input
  const float* coef = nullptr;    // [a | b], 2 * Cin
  const float* coef2 = nullptr;   // [a2 | b2] (AFF)
  const uint16_t* w = nullptr;    // [Cout][Cin]
  uint16_t* y = nullptr;          // [M, Cin]
  uint8_t* mask = nullptr;        // [M, Cin / 8]
  uint16_t* x1 = nullptr;         // [M, Cout]
  float* psum = nullptr;          // [Cout][m_tiles]
  float* psq = nullptr;
  int64_t M = 0;
  int Cin = 0, m_tiles = 0, rev = 0;
};

// the rounding and the mask test of IO::store8m, an element at a time
template <typename IO>
struct Rnd;
template <>
struct Rnd<BF16> {
  __device__ static float up(uint32_t h) { return bf16_to_f32((uint16_t)h); }
  __device__ static uint32_t down(float v) { return f32_to_bf16(v); }
  __device__ static bool pos(uint32_t h) { return BF16::pos16(h); }
};
template <>
struct Rnd<F16> {
  __device__ static float up(uint32_t h) { return f16_to_f32((uint16_t)h); }
  __device__ static uint32_t down(float v) { return F16::to16(v); }
  __device__ static bool pos(uint32_t h) { return (float)__builtin_bit_cast(_Float16, (uint16_t)h) > 0.0f; }
};

template <typename IO, int BN, bool AFF>
__global__ __launch_bounds__(tc1::kThreads, (BN == 64 && !AFF) ? 3 : 2) void tail_conv1_fwd_kernel(TailConv1Args p) {
  using namespace tc1;
  constexpr bool F16V = std::is_same<IO, F16>::value;
  constexpr int WN = BN / 64, WM = 4 / WN, MI = BM / (WM * 32), NI = 2;
  constexpr int B_PER_T = BN * 8 / kThreads;  // weight chunks per thread and K-step
  constexpr int C_STRIDE = BN * 2 + 16;
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* la = lds;
  unsigned char* lb = lds + A_BYTES;
  float* lc = reinterpret_cast<float*>(lds + A_BYTES + BN * kRowBytes);  // [a | b | a2 | b2][Cin]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int lr = lane & 31, lh = lane >> 5;
  const int mt = p.rev ? p.m_tiles - 1 - (int)blockIdx.x : (int)blockIdx.x;
  const int64_t m0 = (int64_t)mt * BM;
  const int Cin = p.Cin, nk = Cin / BK;
  const int mrow = Cin >> 3;  // mask bytes per row
  unsigned char* lm = lds + lds_main<BN>(Cin, AFF);  // [BM][mrow], behind everything the epilogue reuses

  // this thread's chunks: column c (8 channels) of rows rb, rb + 32, rb + 64, rb + 96
  const int c = tid & 7, rb = tid >> 3;
  const uint32_t nbytes = (uint32_t)(p.M * Cin * 2);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x3, 0, (int)nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)p.r, 0, (int)nbytes, 0x00020000);
  uint32_t voff[4];
  bool live[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + rb + 32 * i;
    live[i] = m < p.M;
    voff[i] = live[i] ? (uint32_t)((m * Cin + c * 8) * 2) : kOOB;
  }
  const uint16_t* wrow[B_PER_T];
#pragma unroll
  for (int i = 0; i < B_PER_T; ++i) wrow[i] = p.w + (int64_t)(rb + 32 * i) * Cin + c * 8;

  u32x4 xa[4], ra[4];
  u32x4 wb[B_PER_T];
  auto load_a = [&](int i, int ks) {
    const uint32_t o = live[i] ? voff[i] + (uint32_t)ks * kRowBytes : kOOB;
    xa[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, o, 0, 0);
    ra[i] = __builtin_amdgcn_raw_buffer_load_b128(rr, o, 0, 0);
  };
  auto load_b = [&](int ks) {
#pragma unroll
    for (int i = 0; i < B_PER_T; ++i) wb[i] = *reinterpret_cast<const u32x4*>(wrow[i] + ks * BK);
  };
#pragma unroll
  for (int i = 0; i < 4; ++i) load_a(i, 0);
  load_b(0);
  for (int i = tid; i < 2 * Cin; i += kThreads) {
    lc[i] = p.coef[i];
    if (AFF) lc[2 * Cin + i] = p.coef2[i];
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
    float a[8], b[8], a2[8], b2[8];
    const int ch0 = ks * BK + c * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      a[k] = lc[ch0 + k];
      b[k] = lc[Cin + ch0 + k];
      a2[k] = AFF ? lc[2 * Cin + ch0 + k] : 0.f;
      b2[k] = AFF ? lc[3 * Cin + ch0 + k] : 0.f;
    }
    u32x4 yv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t xu[4] = {xa[i].x, xa[i].y, xa[i].z, xa[i].w};
      const uint32_t ru[4] = {ra[i].x, ra[i].y, ra[i].z, ra[i].w};
      float v[8], q[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        v[k] = Rnd<IO>::up(k & 1 ? xu[k >> 1] >> 16 : xu[k >> 1] & 0xffffu);
        q[k] = Rnd<IO>::up(k & 1 ? ru[k >> 1] >> 16 : ru[k >> 1] & 0xffffu);
      }
      // the registers are free again: the next K-step's chunk is in flight from here, while the
      // rest of this K-step is applied, staged and multiplied
      if (more) load_a(i, ks + 1);
      uint32_t h[8], msk = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float o = __builtin_fmaf(v[k], a[k], b[k]);  // bn_fwd_apply_kernel, expression for expression
        if (AFF) o += __builtin_fmaf(q[k], a2[k], b2[k]);
        else o += q[k];
        o = o < 0.0f ? 0.0f : o;  // NaN-propagating
        h[k] = Rnd<IO>::down(o);
        msk |= (Rnd<IO>::pos(h[k]) ? 1u : 0u) << k;
      }
      yv[i] = u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
      const int row = rb + 32 * i;
      // the tile's mask bytes are gathered in LDS and stored as whole rows at the end: a byte per
      // row and K-step straight to memory is a partial write of every 32-byte sector, four times
      lm[row * mrow + (ch0 >> 3)] = (uint8_t)msk;
      if (live[i]) *reinterpret_cast<u32x4*>(p.y + (m0 + row) * Cin + ch0) = yv[i];
      else yv[i] = u32x4{0u, 0u, 0u, 0u};  // rows past M are zero rows of the GEMM
    }
    if (ks > 0) __syncthreads();  // every wave has multiplied the previous K-step
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = rb + 32 * i;
      *reinterpret_cast<u32x4*>(la + row * kRowBytes + swz(row, c) * 16) = yv[i];
    }
#pragma unroll
    for (int i = 0; i < B_PER_T; ++i) {
      const int row = rb + 32 * i;
      *reinterpret_cast<u32x4*>(lb + row * kRowBytes + swz(row, c) * 16) = wb[i];
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

  // ---- epilogue of conv_fwd_kernel (LDS image, BN partial sums), operation for operation ----
  float cs[NI], cq[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) { cs[j] = 0.f; cq[j] = 0.f; }
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
        // rows past M hold exact zeros: no effect on the sums
        const float f0 = cunpack<F16V>(u, 0), f1 = cunpack<F16V>(u, 1);
        cs[j] += f0 + f1;
        cq[j] = __builtin_fmaf(f0, f0, __builtin_fmaf(f1, f1, cq[j]));
      }
    }
  float* red = reinterpret_cast<float*>(lds + BM * C_STRIDE);  // [2][WM][BN]
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    cs[j] += __shfl_xor(cs[j], 32, 64);
    cq[j] += __shfl_xor(cq[j], 32, 64);
    if (lh == 0) {
      const int col = wn * 64 + j * 32 + lr;
      red[wm * BN + col] = cs[j];
      red[WM * BN + wm * BN + col] = cq[j];
    }
  }
  __syncthreads();
  if (tid < BN) {
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int w = 0; w < WM; ++w) { s += red[w * BN + tid]; q += red[WM * BN + w * BN + tid]; }
    p.psum[(int64_t)tid * p.m_tiles + mt] = s;
    p.psq[(int64_t)tid * p.m_tiles + mt] = q;
  }
  // the tile's mask rows are one contiguous piece of the mask: 8-byte stores, whole rows only
  for (int j = tid; j < BM * mrow / 8; j += kThreads) {
    if (m0 + (j * 8) / mrow < p.M)
      *reinterpret_cast<uint2*>(p.mask + m0 * mrow + j * 8) = *reinterpret_cast<const uint2*>(lm + j * 8);
  }
  constexpr int CPR = BN / 8, RPP = kThreads / CPR, NPASS = BM / RPP;
  const int oc = tid % CPR, orow = tid / CPR;
#pragma unroll
  for (int g = 0; g < NPASS; ++g) {
    const int row = g * RPP + orow;
    const int64_t m = m0 + row;
    if (m < p.M)
      *reinterpret_cast<uint4*>(p.x1 + m * BN + oc * 8) = *reinterpret_cast<const uint4*>(lds + row * C_STRIDE + oc * 16);
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static size_t tail_conv1_lds(int Cin, int Cout, bool aff) {
  const size_t front = Cout == 128 ? tc1::lds_main<128>(Cin, aff) : tc1::lds_main<64>(Cin, aff);
  return front + (size_t)tc1::BM * (Cin / 8);  // + the tile's mask bytes
}

const char* tail_conv1_refusal(int64_t M, int64_t Cin, int64_t Cout) {
  if (Cin < 64 || Cin % 64 != 0) return "needs Cin % 64 == 0 and Cin >= 64";
  if (Cout != 64 && Cout != 128) return "needs Cout of 64 or 128 (one output-channel tile)";
  if (!bn_supported(Cin)) return "Cin is not a fused-BatchNorm channel count";
  if (M < 1) return "empty input";
  // 32-bit byte offsets through buffer descriptors, as conv_fwd_kernel (conv_check_offsets)
  if (M * Cin * 2 >= 0xFFFFFF00ll || Cout * Cin * 2 >= 0x7FFFFFFFll) return "operand tensors beyond 2^31 elements";
  if (tail_conv1_lds((int)Cin, (int)Cout, true) > 65536) return "the coefficients and the mask tile do not fit the LDS";
  // a conv the split-K policy would split (eagerly or under graph capture) is not fused: its
  // statistics come in another layout and a different summation order
  if (conv_fwd_splits_for(M, (int)Cout, Cin, false) != 1 || conv_fwd_splits_for(M, (int)Cout, Cin, true) != 1)
    return "the split-K policy splits this conv";
  return nullptr;
}

// Apply passes walk the rows last-to-first (bn_kernels.hip kBnReverse): the rows the producing conv
// wrote last are still in the caches.  The fused kernel takes its M-tiles in the same order.
constexpr int kTailReverse = 1;

template <typename IO>
static void tail_conv1_dispatch(const TailConv1Args& a, int Cout, bool aff, hipStream_t s) {
  const dim3 grid((unsigned)a.m_tiles), block(tc1::kThreads);
  const size_t lds = tail_conv1_lds(a.Cin, Cout, aff);
#define DPT_TC1(BN, AFFV) \
  hipLaunchKernelGGL((tail_conv1_fwd_kernel<IO, BN, AFFV>), grid, block, lds, s, a)
  if (Cout == 128) { if (aff) DPT_TC1(128, true); else DPT_TC1(128, false); }
  else { if (aff) DPT_TC1(64, true); else DPT_TC1(64, false); }
#undef DPT_TC1
}

void launch_tail_conv1_fwd(bool f16, const uint16_t* x3, const uint16_t* r, const float* coef, const float* coef2,
                           const uint16_t* w, uint16_t* y, uint8_t* mask, uint16_t* x1, float* psum, float* psq,
                           int64_t M, int Cin, int Cout, hipStream_t s) {
  if (const char* why = tail_conv1_refusal(M, Cin, Cout)) throw std::runtime_error(std::string("tail_conv1_fwd: ") + why);
  TailConv1Args a;
  a.x3 = x3; a.r = r; a.coef = coef; a.coef2 = coef2; a.w = w; a.y = y; a.mask = mask; a.x1 = x1;
  a.psum = psum; a.psq = psq; a.M = M; a.Cin = Cin; a.m_tiles = conv_m_tiles(M); a.rev = kTailReverse;
  if (f16) tail_conv1_dispatch<F16>(a, Cout, coef2 != nullptr, s);
  else tail_conv1_dispatch<BF16>(a, Cout, coef2 != nullptr, s);
}

}  // namespace dpt
