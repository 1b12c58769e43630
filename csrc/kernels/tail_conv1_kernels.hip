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
// x1, psum and psq are bit-equal to conv_fwd_kernel<128, BN, 1, LDSEPI, STATS>: the tile, the MFMA
// order and the rounded LDS image are tail_tile.h's; here, per-lane f0 + f1 / fma sums, shfl_xor 32,
// waves summed in index order.  One 128-row tile per block, plain grid, no inter-block communication.
#include <stdexcept>
#include <string>
#include <type_traits>

#include "bn_io.h"
#include "common.h"
#include "kernels.h"
#include "mfma.h"
#include "tail_tile.h"

namespace dpt {

namespace tc1 {
using namespace tail;

template <int BN>
__host__ __device__ constexpr int lds_epi() { return image_bytes(BN) + 2 * (4 / (BN / 64)) * BN * 4; }
// K-loop image (A tile, B tile, coefficients) and the epilogue image share the front of the LDS
template <int BN>
__host__ __device__ constexpr int lds_main(int Cin, bool aff) {
  const int main = tile_bytes(BN) + (aff ? 4 : 2) * Cin * 4, epi = lds_epi<BN>();
  return main > epi ? main : epi;
}

// the mask test of IO::store8m, an element at a time
template <typename IO>
__device__ __forceinline__ bool pos(uint32_t h) {
  if constexpr (std::is_same<IO, F16>::value) return (float)__builtin_bit_cast(_Float16, (uint16_t)h) > 0.0f;
  else return BF16::pos16(h);
}
}  // namespace tc1

template <typename IO, int BN, bool AFF>
__global__ __launch_bounds__(tail::kThreads, (BN == 64 && !AFF) ? 3 : 2) void tail_conv1_fwd_kernel(TailConv1Args p) {
  using namespace tc1;
  constexpr bool F16V = std::is_same<IO, F16>::value;
  using T = Tile<F16V, BN>;
  constexpr int WN = T::WN, WM = T::WM, NI = T::NI, B_PER_T = T::B_PER_T, C_STRIDE = T::C_STRIDE;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  float* lc = reinterpret_cast<float*>(lds + tile_bytes(BN));  // [a | b | a2 | b2][Cin]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int lr = lane & 31, lh = lane >> 5;
  const int Cin = p.Cin, nk = Cin / BK;
  const Rows t(p.M, Cin, p.m_tiles, p.rev);
  const int mt = t.mt, c = t.c, rb = t.rb;
  const int64_t m0 = t.m0;
  const int mrow = Cin >> 3;  // mask bytes per row
  unsigned char* lm = lds + lds_main<BN>(Cin, AFF);  // [BM][mrow], behind everything the epilogue reuses

  const uint32_t nbytes = (uint32_t)(p.M * Cin * 2);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x3, 0, (int)nbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)p.r, 0, (int)nbytes, 0x00020000);
  const uint16_t* wrow[B_PER_T];
#pragma unroll
  for (int i = 0; i < B_PER_T; ++i) wrow[i] = p.w + (int64_t)(rb + 32 * i) * Cin + c * 8;

  u32x4 xa[4], ra[4];
  u32x4 wb[B_PER_T];
  auto load_a = [&](int i, int ks) {
    const uint32_t o = t.off(i, ks);
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

  typename T::Acc acc;
  T::zero(acc);

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
      float v[8], q[8];
      unpack8<IO>(xa[i], v);
      unpack8<IO>(ra[i], q);
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
        h[k] = down16<IO>(o);
        msk |= (pos<IO>(h[k]) ? 1u : 0u) << k;
      }
      yv[i] = pack8(h);
      const int row = rb + 32 * i;
      // the tile's mask bytes are gathered in LDS and stored as whole rows at the end: a byte per
      // row and K-step straight to memory is a partial write of every 32-byte sector, four times
      lm[row * mrow + (ch0 >> 3)] = (uint8_t)msk;
      if (t.live[i]) *reinterpret_cast<u32x4*>(p.y + (m0 + row) * Cin + ch0) = yv[i];
      else yv[i] = u32x4{0u, 0u, 0u, 0u};  // rows past M are zero rows of the GEMM
    }
    if (ks > 0) __syncthreads();  // every wave has multiplied the previous K-step
    T::stage(lds, yv, wb);
    if (more) load_b(ks + 1);
    __syncthreads();
    T::mma(lds, acc);
  }
  __syncthreads();  // the epilogue reuses the LDS

  // ---- the LDS image of tail_tile.h with the BN partial sums of conv_fwd_kernel's epilogue ----
  float cs[NI], cq[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) { cs[j] = 0.f; cq[j] = 0.f; }
  T::image(lds, acc, [&](int j, uint32_t u) {
    // rows past M hold exact zeros: no effect on the sums
    const float f0 = cunpack<F16V>(u, 0), f1 = cunpack<F16V>(u, 1);
    cs[j] += f0 + f1;
    cq[j] = __builtin_fmaf(f0, f0, __builtin_fmaf(f1, f1, cq[j]));
  });
  float* red = reinterpret_cast<float*>(lds + image_bytes(BN));  // [2][WM][BN]
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
  const int oc = tid % T::CPR, orow = tid / T::CPR;
#pragma unroll
  for (int g = 0; g < T::NPASS; ++g) {
    const int row = g * T::RPP + orow;
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
  return front + (size_t)tail::BM * (Cin / 8);  // + the tile's mask bytes
}

const char* tail_conv1_refusal(int64_t M, int64_t Cin, int64_t Cout) {
  if (const char* why = tail_tile_refusal(M, Cin, Cout, "needs Cin % 64 == 0 and Cin >= 64",
                                          "needs Cout of 64 or 128 (one output-channel tile)"))
    return why;
  if (!bn_supported(Cin)) return "Cin is not a fused-BatchNorm channel count";
  if (tail_conv1_lds((int)Cin, (int)Cout, true) > 65536) return "the coefficients and the mask tile do not fit the LDS";
  // a conv the split-K policy would split (eagerly or under graph capture) is not fused: its
  // statistics come in another layout and a different summation order
  if (conv_fwd_splits_for(M, (int)Cout, Cin, false) != 1 || conv_fwd_splits_for(M, (int)Cout, Cin, true) != 1)
    return "the split-K policy splits this conv";
  return nullptr;
}

void launch_tail_conv1_fwd(bool f16, TailConv1Args a, int Cout, hipStream_t s) {
  if (const char* why = tail_conv1_refusal(a.M, a.Cin, Cout)) throw std::runtime_error(std::string("tail_conv1_fwd: ") + why);
  const bool aff = a.coef2 != nullptr;
  a.m_tiles = conv_m_tiles(a.M);
  a.rev = kTailReverse;
  const dim3 grid((unsigned)a.m_tiles), block(tail::kThreads);
  const size_t lds = tail_conv1_lds(a.Cin, Cout, aff);
  tail_dispatch(f16, Cout == 128, aff, [&](auto h, auto w, auto t) {
    hipLaunchKernelGGL((tail_conv1_fwd_kernel<std::conditional_t<h.value, F16, BF16>, w.value ? 128 : 64, t.value>), grid,
                       block, lds, s, a);
  });
}

}  // namespace dpt
