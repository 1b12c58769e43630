// Patchify convolutions with bias (kernel == stride, no padding) on the gfx950 matrix cores:
// ConvNeXt's 2x2 stride-2 downsamples (C % 32 == 0) and its 4x4 stride-4 stem (C = 3).
//
// With kernel == stride a conv is a plain GEMM whose operand row needs no im2col: in channels_last
// the patch of output pixel m = (n, ho, wo) is k contiguous runs of k*C elements (one per patch
// row r), and a channels_last weight [Cout][r][s][c] has the same (r, s, c) order.  So
//   M = N*Ho*Wo rows (Ho = H / k, Wo = W / k, floor),  K = k*k*C,  Cout columns,
// no halo, no border taps, and backward-data writes every input pixel exactly once.  Operands are
// bf16 or fp16 (F16), accumulation fp32 (v_mfma_f32_32x32x16), element offsets 64-bit.
//
// All three kernels: 256 threads (4 waves), K-steps of 64 reduction elements, operands loaded with
// 16-byte global loads into registers one K-step ahead and written into double-buffered swizzled
// LDS images (mfma.h), one barrier per K-step.
//
// patchconv_fwd_kernel<F16>     y = A W^T + bias.  A workgroup owns 128 rows x 128 columns; a wave
//   owns 32 rows x all columns as 32-column accumulators and skips the accumulators past Cout
//   (Cout = 96: three of four, no MFMA on padding columns).  The MFMA runs transposed (W rows as
//   the A operand) so a lane holds 4 consecutive output channels of one pixel: bias is added in
//   fp32, the values are rounded once, packed, passed through an LDS tile and stored 16 bytes wide.
//   A K-step of 64 lies inside one run (2C % 64 == 0), so the A tile is 128 rows x 128 contiguous
//   bytes.  LDS 2 x (16 + 16) KB.
// patchconv_stem_fwd_kernel<F16, XF32>  the same tile for k = 4, C = 3: the four 12-element runs of
//   a row are gathered into one zero-padded K-step (K = 48 -> 64); an fp32 x is rounded to the
//   operand type on the way (the rounding of autocast's cast kernel).
// patchconv_dgrad_kernel<F16>   dxpatch = dy W (k = 2), reduction over Cout.  W is staged as stored,
//   [Cout][K] rows, and read with the transposing LDS read (tr_frag); the 128 x 128 tile of patch
//   rows is scattered back to its two runs of dx with 16-byte stores.  The workgroups of the first
//   K tile also zero the trailing row / column of an odd H / W: every element of dx is written
//   once, no memset, no atomics.
// patchconv_wgrad_kernel<F16, STEM, XF32>  dW = dy^T A, reduction over M.  Both operands have the
//   reduction index as their row, so both go through the transposing reads.  A workgroup owns
//   128 output channels x 128 (stem: 64) K columns of one slice of the rows, 2 x 2 waves; it
//   writes an fp32 partial [Cout*K + Cout]; the trailing Cout entries, the bias gradient, come
//   from one more MFMA per dy fragment against a fragment of ones in the workgroups of the first
//   K tile.  launch_sum_partials (the stem, one tile and hundreds of slices: launch_colsum_rows) adds
//   the slices in a fixed order: bitwise repeatable.
#include "common.h"
#include "kernels.h"
#include "mfma.h"

namespace dpt {

namespace pc {
constexpr int TM = kPatchconvTM, TN = kPatchconvTN, BK = 64, NT = 256;
constexpr int OPITCH = TN * 2 + 16;  // bytes per row of the epilogue tile

struct Geom {
  int H, W, C, Ho, Wo, Cout, k;
  int M, K;  // N*Ho*Wo, k*k*C
};

// element offset of the first element of row m's patch: pixel (n, ho*k, wo*k)
__device__ __forceinline__ int64_t row_base(int m, const Geom& g) {
  const int hw = g.Ho * g.Wo;
  const int n = m / hw, rem = m - n * hw;
  const int ho = rem / g.Wo, wo = rem - ho * g.Wo;
  return (((int64_t)n * g.H + ho * g.k) * g.W + wo * g.k) * g.C;
}

// offset of patch column kk (in (r, s, c) order) from row_base
__device__ __forceinline__ int64_t col_add(int kk, const Geom& g) {
  const int run = g.k * g.C;
  const int r = kk / run;
  return (int64_t)r * g.W * g.C + (kk - r * run);
}

__device__ __forceinline__ uint4 ld16(const uint16_t* p) { return *reinterpret_cast<const uint4*>(p); }

template <int RB>
__device__ __forceinline__ void put16(unsigned char* img, int row, int ch, uint4 v) {
  *reinterpret_cast<uint4*>(img + row * RB + wg_slot<RB>(row, ch) * 16) = v;
}

template <bool F16>
__device__ __forceinline__ uint32_t pack2(float a, float b) {
  const f32x2_t v = {a, b};
  return cpack<F16>(v);
}

// One 12-element run (4 pixels x 3 channels) of a stem patch as six packed 16-bit pairs.  Rows of
// x start on 16 (fp32) / 8 (16-bit) byte boundaries only when W % 4 == 0 (vec).
template <bool F16, bool XF32>
__device__ __forceinline__ void stem_run(const void* x, int64_t off, bool vec, uint32_t u[6]) {
  if constexpr (XF32) {
    const float* p = static_cast<const float*>(x) + off;
    float f[12];
    if (vec) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const float4 v = reinterpret_cast<const float4*>(p)[q];
        f[4 * q] = v.x; f[4 * q + 1] = v.y; f[4 * q + 2] = v.z; f[4 * q + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 12; ++q) f[q] = p[q];
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) u[q] = pack2<F16>(f[2 * q], f[2 * q + 1]);
  } else {
    const uint16_t* p = static_cast<const uint16_t*>(x) + off;
    if (vec) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const uint2 v = reinterpret_cast<const uint2*>(p)[q];
        u[2 * q] = v.x; u[2 * q + 1] = v.y;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 6; ++q) u[q] = (uint32_t)p[2 * q] | ((uint32_t)p[2 * q + 1] << 16);
    }
  }
}

// the six pairs of run `run` into row `row` of a 128-byte-row image: elements run*12 .. run*12+11
__device__ __forceinline__ void stem_put(unsigned char* img, int row, int run, const uint32_t u[6]) {
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const int e = run * 12 + 2 * q;
    *reinterpret_cast<uint32_t*>(img + row * 128 + wg_slot<128>(row, e >> 3) * 16 + (e & 7) * 2) = u[q];
  }
}

// acc[j] = W tile rows (output channels j*32..+31) x this wave's 32 pixels, one 64-element K-step
template <bool F16>
__device__ __forceinline__ void fwd_mma(const unsigned char* aimg, const unsigned char* wimg, f32x16_t (&acc)[4],
                                        int nj, int wid, int lane) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int s = 0; s < BK / 16; ++s) {
    const bf16x8_t fb = row_frag<128>(aimg, wid * 32 + r, 2 * s + h);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nj) acc[j] = cmfma<F16>(row_frag<128>(wimg, j * 32 + r, 2 * s + h), fb, acc[j]);
  }
}

// Accumulators (rows = tile columns j*32 + .., column = this lane's pixel) + badd -> 16-bit tile
// ot[pixel][column], one rounding.
template <bool F16>
__device__ __forceinline__ void tile_put(unsigned char* ot, const f32x16_t (&acc)[4], int nj, const float* badd,
                                         int wid, int lane) {
  const int pix = wid * 32 + (lane & 31), h = lane >> 5;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j >= nj) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = j * 32 + 8 * q + 4 * h;
      uint2 u;
      u.x = pack2<F16>(acc[j][4 * q] + badd[c], acc[j][4 * q + 1] + badd[c + 1]);
      u.y = pack2<F16>(acc[j][4 * q + 2] + badd[c + 2], acc[j][4 * q + 3] + badd[c + 3]);
      *reinterpret_cast<uint2*>(ot + pix * OPITCH + c * 2) = u;
    }
  }
}

// rows m0.. of the tile -> y[m][n0 + ..], 16 bytes per store
__device__ __forceinline__ void tile_store_rows(const unsigned char* ot, uint16_t* y, int m0, int n0, int ncols,
                                                const Geom& g) {
  for (int i = threadIdx.x; i < TM * (TN / 8); i += NT) {
    const int row = i / (TN / 8), c = i % (TN / 8);
    if (m0 + row < g.M && c * 8 < ncols)
      *reinterpret_cast<uint4*>(y + (int64_t)(m0 + row) * g.Cout + n0 + c * 8) =
          *reinterpret_cast<const uint4*>(ot + row * OPITCH + c * 16);
  }
}

__device__ __forceinline__ void zero_acc(f32x16_t& a) {
#pragma unroll
  for (int e = 0; e < 16; ++e) a[e] = 0.f;
}

__device__ __forceinline__ void load_bias(float* bsh, const void* bias, int bias_kind, int n0, int Cout, bool f16) {
  if (threadIdx.x < TN) {
    const int c = n0 + threadIdx.x;
    float b = 0.f;
    if (bias != nullptr && c < Cout) {
      if (bias_kind == 0) b = static_cast<const float*>(bias)[c];
      else if (f16) b = f16_to_f32(static_cast<const uint16_t*>(bias)[c]);
      else b = bf16_to_f32(static_cast<const uint16_t*>(bias)[c]);
    }
    bsh[threadIdx.x] = b;
  }
}
}  // namespace pc

// ---- forward, k = 2 -----------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(pc::NT, 2) void patchconv_fwd_kernel(const uint16_t* __restrict__ x,
                                                                  const uint16_t* __restrict__ w,
                                                                  const void* __restrict__ bias, int bias_kind,
                                                                  uint16_t* __restrict__ y, pc::Geom g, int ntiles) {
  using namespace pc;
  constexpr int A_BYTES = TM * 128, STAGE = A_BYTES + TN * 128;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];
  __shared__ float bsh[TN];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int mt = blockIdx.x / ntiles, nt = blockIdx.x - mt * ntiles;
  const int m0 = mt * TM, n0 = nt * TN;
  const int ncols = min(TN, g.Cout - n0), nj = ncols / 32;
  load_bias(bsh, bias, bias_kind, n0, g.Cout, F16);

  // this thread's 4 rows (i*32 + tid/8) and 16-byte chunk (tid % 8) of both images
  const int ch = tid & 7, row0 = tid >> 3;
  int64_t abase[4], wbase[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = i * 32 + row0;
    abase[i] = m0 + row < g.M ? row_base(m0 + row, g) : -1;
    wbase[i] = row < ncols ? (int64_t)(n0 + row) * g.K : -1;
  }
  uint4 ra[4], rw[4];
  auto load = [&](int step) {
    const int kk = step * BK + ch * 8;
    const int64_t add = col_add(kk, g);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = abase[i] >= 0 ? ld16(x + abase[i] + add) : make_uint4(0, 0, 0, 0);
      rw[i] = wbase[i] >= 0 ? ld16(w + wbase[i] + kk) : make_uint4(0, 0, 0, 0);
    }
  };
  auto store = [&](int buf) {
    unsigned char* a = lds + buf * STAGE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      put16<128>(a, i * 32 + row0, ch, ra[i]);
      put16<128>(a + A_BYTES, i * 32 + row0, ch, rw[i]);
    }
  };

  f32x16_t acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) zero_acc(acc[j]);
  const int steps = g.K / BK;
  load(0);
  store(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const int cur = s & 1;
    if (s + 1 < steps) load(s + 1);
    fwd_mma<F16>(lds + cur * STAGE, lds + cur * STAGE + A_BYTES, acc, nj, wid, lane);
    if (s + 1 < steps) store(cur ^ 1);
    __syncthreads();
  }
  tile_put<F16>(lds, acc, nj, bsh, wid, lane);
  __syncthreads();
  tile_store_rows(lds, y, m0, n0, ncols, g);
}

// ---- forward, stem (k = 4, C = 3, K = 48 in one zero-padded K-step) ------------------------------
template <bool F16, bool XF32>
__global__ __launch_bounds__(pc::NT, 2) void patchconv_stem_fwd_kernel(const void* __restrict__ x,
                                                                       const uint16_t* __restrict__ w,
                                                                       const void* __restrict__ bias, int bias_kind,
                                                                       uint16_t* __restrict__ y, pc::Geom g,
                                                                       int ntiles) {
  using namespace pc;
  constexpr int A_BYTES = TM * 128;
  __shared__ __attribute__((aligned(16))) unsigned char lds[TM * OPITCH];  // >= A_BYTES + TN * 128
  __shared__ float bsh[TN];
  static_assert(TM * OPITCH >= A_BYTES + TN * 128, "stem: the epilogue tile covers both images");
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int mt = blockIdx.x / ntiles, nt = blockIdx.x - mt * ntiles;
  const int m0 = mt * TM, n0 = nt * TN;
  const int ncols = min(TN, g.Cout - n0), nj = ncols / 32;
  load_bias(bsh, bias, bias_kind, n0, g.Cout, F16);

  const bool vec = (g.W & 3) == 0;
  unsigned char* aimg = lds;
  unsigned char* wimg = lds + A_BYTES;
#pragma unroll
  for (int it = 0; it < 2; ++it) {  // 128 rows x 4 runs: a wave reads one run of 64 consecutive rows
    const int item = it * NT + tid, row = item & (TM - 1), run = item / TM;
    uint32_t u[6] = {0, 0, 0, 0, 0, 0};
    if (m0 + row < g.M) stem_run<F16, XF32>(x, row_base(m0 + row, g) + (int64_t)run * g.W * 3, vec, u);
    stem_put(aimg, row, run, u);
  }
  put16<128>(aimg, tid >> 1, 6 + (tid & 1), make_uint4(0, 0, 0, 0));  // K 48..63 of every row
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = i * 32 + (tid >> 3), ch = tid & 7;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (row < ncols && ch * 8 < g.K) v = ld16(w + (int64_t)(n0 + row) * g.K + ch * 8);
    put16<128>(wimg, row, ch, v);
  }
  __syncthreads();
  f32x16_t acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) zero_acc(acc[j]);
  fwd_mma<F16>(aimg, wimg, acc, nj, wid, lane);
  __syncthreads();
  tile_put<F16>(lds, acc, nj, bsh, wid, lane);
  __syncthreads();
  tile_store_rows(lds, y, m0, n0, ncols, g);
}

// ---- backward-data, k = 2 -----------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(pc::NT, 2) void patchconv_dgrad_kernel(const uint16_t* __restrict__ dy,
                                                                    const uint16_t* __restrict__ w,
                                                                    uint16_t* __restrict__ dx, pc::Geom g, int ktiles) {
  using namespace pc;
  constexpr int A_BYTES = TM * 128, STAGE = A_BYTES + BK * 256;  // dy [128 m][64 co], W [64 co][128 kk]
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];
  __shared__ float zsh[TN];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int mt = blockIdx.x / ktiles, kt = blockIdx.x - mt * ktiles;
  const int m0 = mt * TM, kk0 = kt * TN;
  if (tid < TN) zsh[tid] = 0.f;

  const int ach = tid & 7, arow0 = tid >> 3;    // dy: rows i*32 + tid/8
  const int wch = tid & 15, wrow0 = tid >> 4;   // W: rows i*16 + tid/16
  uint4 ra[4], rw[4];
  auto load = [&](int step) {
    const int co0 = step * BK;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + i * 32 + arow0, co = co0 + i * 16 + wrow0;
      ra[i] = (m < g.M && co0 + ach * 8 < g.Cout) ? ld16(dy + (int64_t)m * g.Cout + co0 + ach * 8)
                                                  : make_uint4(0, 0, 0, 0);
      rw[i] = co < g.Cout ? ld16(w + (int64_t)co * g.K + kk0 + wch * 8) : make_uint4(0, 0, 0, 0);
    }
  };
  auto store = [&](int buf) {
    unsigned char* a = lds + buf * STAGE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      put16<128>(a, i * 32 + arow0, ach, ra[i]);
      put16<256>(a + A_BYTES, i * 16 + wrow0, wch, rw[i]);
    }
  };
  f32x16_t acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) zero_acc(acc[j]);
  const int steps = (g.Cout + BK - 1) / BK;
  load(0);
  store(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const int cur = s & 1;
    if (s + 1 < steps) load(s + 1);
    const unsigned char* a = lds + cur * STAGE;
    const unsigned char* b = a + A_BYTES;
#pragma unroll
    for (int q = 0; q < BK / 16; ++q) {
      const bf16x8_t fb = row_frag<128>(a, wid * 32 + (lane & 31), 2 * q + (lane >> 5));
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = cmfma<F16>(tr_frag<256>(b, q * 16, j * 32, lane), fb, acc[j]);
    }
    if (s + 1 < steps) store(cur ^ 1);
    __syncthreads();
  }
  tile_put<F16>(lds, acc, 4, zsh, wid, lane);
  __syncthreads();
  // each row's 128 patch columns back to their runs of dx
  for (int i = tid; i < TM * (TN / 8); i += NT) {
    const int row = i / (TN / 8), c = i % (TN / 8);
    if (m0 + row < g.M)
      *reinterpret_cast<uint4*>(dx + row_base(m0 + row, g) + col_add(kk0 + c * 8, g)) =
          *reinterpret_cast<const uint4*>(lds + row * OPITCH + c * 16);
  }
  // Pixels that no patch covers (odd H: row H-1, odd W: column W-1) are zero.  Row m owns the up
  // to five of them that touch its patch: (2ho, W-1), (2ho+1, W-1), (H-1, 2wo), (H-1, 2wo+1), (H-1, W-1).
  if (kt == 0 && ((g.H | g.W) & 1)) {
    const int cv = g.C / 8;
    for (int i = tid; i < TM * 5 * cv; i += NT) {
      const int c = i % cv, t = i / cv, e = t % 5, m = m0 + t / 5;
      if (m >= g.M) continue;
      const int hw = g.Ho * g.Wo, n = m / hw, rem = m - n * hw, ho = rem / g.Wo, wo = rem - ho * g.Wo;
      const bool wlast = (g.W & 1) && wo == g.Wo - 1, hlast = (g.H & 1) && ho == g.Ho - 1;
      int ph, pw;
      bool on;
      if (e < 2) { ph = 2 * ho + e; pw = g.W - 1; on = wlast; }
      else if (e < 4) { ph = g.H - 1; pw = 2 * wo + (e - 2); on = hlast; }
      else { ph = g.H - 1; pw = g.W - 1; on = wlast && hlast; }
      if (on)
        *reinterpret_cast<uint4*>(dx + (((int64_t)n * g.H + ph) * g.W + pw) * g.C + c * 8) = make_uint4(0, 0, 0, 0);
    }
  }
}

// ---- backward-weight and bias gradient -------------------------------------------------------------
template <bool F16, bool STEM, bool XF32>
__global__ __launch_bounds__(pc::NT, 2) void patchconv_wgrad_kernel(const uint16_t* __restrict__ dy,
                                                                    const void* __restrict__ xv,
                                                                    float* __restrict__ part, pc::Geom g, int ctiles,
                                                                    int ktiles, int steps_per_slice) {
  using namespace pc;
  constexpr int TK = STEM ? 64 : 128, RBX = TK * 2, NJ = TK / 64;
  constexpr int A_BYTES = BK * 256, STAGE = A_BYTES + BK * RBX;  // dy [64 m][128 co], x [64 m][TK kk]
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];
  const uint16_t* x16 = static_cast<const uint16_t*>(xv);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  int bid = blockIdx.x;
  const int kt = bid % ktiles; bid /= ktiles;
  const int ct = bid % ctiles, sl = bid / ctiles;
  const int co0 = ct * TN, kk0 = kt * TK;
  const int nsteps = (g.M + BK - 1) / BK;
  const int s0 = sl * steps_per_slice, s1 = min(s0 + steps_per_slice, nsteps);

  const int ch = tid & 15, row0 = tid >> 4;  // rows i*16 + tid/16 of both 256-byte-row images
  const bool dy_on = co0 + ch * 8 < g.Cout;
  const int64_t xadd = STEM ? 0 : col_add(kk0 + ch * 8, g);
  const bool vec = (g.W & 3) == 0;
  uint4 ra[4], rx[4];
  uint32_t su[6];
  auto load = [&](int step) {
    const int mb = step * BK;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = mb + i * 16 + row0;
      ra[i] = (m < g.M && dy_on) ? ld16(dy + (int64_t)m * g.Cout + co0 + ch * 8) : make_uint4(0, 0, 0, 0);
      if constexpr (!STEM) rx[i] = m < g.M ? ld16(x16 + row_base(m, g) + xadd) : make_uint4(0, 0, 0, 0);
    }
    if constexpr (STEM) {  // 64 rows x 4 runs: one item per thread
      const int m = mb + (tid & 63), run = tid >> 6;
#pragma unroll
      for (int q = 0; q < 6; ++q) su[q] = 0;
      if (m < g.M) stem_run<F16, XF32>(xv, row_base(m, g) + (int64_t)run * g.W * 3, vec, su);
    }
  };
  auto store = [&](int buf) {
    unsigned char* a = lds + buf * STAGE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      put16<256>(a, i * 16 + row0, ch, ra[i]);
      if constexpr (!STEM) put16<256>(a + A_BYTES, i * 16 + row0, ch, rx[i]);
    }
    if constexpr (STEM) stem_put(a + A_BYTES, tid & 63, tid >> 6, su);
  };

  f32x16_t acc[2][NJ], accb[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    zero_acc(accb[i]);
#pragma unroll
    for (int j = 0; j < NJ; ++j) zero_acc(acc[i][j]);
  }
  // output-channel blocks of this wave that exist, and whether it forms the bias gradient
  bool on[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) on[i] = co0 + wm * 64 + i * 32 < g.Cout;
  const bool dob = kt == 0 && wn == 0;
  const uint16_t one = F16 ? 0x3C00 : 0x3F80;
  i16x8_t ov;
#pragma unroll
  for (int q = 0; q < 8; ++q) ov[q] = (short)one;
  const bf16x8_t ones = __builtin_bit_cast(bf16x8_t, ov);

  if constexpr (STEM) {  // K 48..63 of every row of both buffers stays zero
    if (tid < 128) {
      put16<128>(lds + A_BYTES, tid >> 1, 6 + (tid & 1), make_uint4(0, 0, 0, 0));
      put16<128>(lds + STAGE + A_BYTES, tid >> 1, 6 + (tid & 1), make_uint4(0, 0, 0, 0));
    }
  }
  if (s0 < s1) {
    load(s0);
    store(0);
  }
  __syncthreads();
  for (int s = s0; s < s1; ++s) {
    const int cur = (s - s0) & 1;
    if (s + 1 < s1) load(s + 1);
    const unsigned char* a = lds + cur * STAGE;
    const unsigned char* b = a + A_BYTES;
#pragma unroll
    for (int q = 0; q < BK / 16; ++q) {
      bf16x8_t fa[2], fb[NJ];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = tr_frag<256>(a, q * 16, wm * 64 + i * 32, lane);
#pragma unroll
      for (int j = 0; j < NJ; ++j) fb[j] = tr_frag<RBX>(b, q * 16, wn * (TK / 2) + j * 32, lane);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (!on[i]) continue;
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = cmfma<F16>(fa[i], fb[j], acc[i][j]);
        if (dob) accb[i] = cmfma<F16>(fa[i], ones, accb[i]);
      }
    }
    if (s + 1 < s1) store(cur ^ 1);
    __syncthreads();
  }

  float* out = part + (int64_t)sl * ((int64_t)g.Cout * g.K + g.Cout);
  const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (!on[i]) continue;
    const int cob = co0 + wm * 64 + i * 32;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = kk0 + wn * (TK / 2) + j * 32 + lr;
      if (col >= g.K) continue;  // the stem's padding columns
#pragma unroll
      for (int e = 0; e < 16; ++e)
        out[(int64_t)(cob + (e & 3) + 8 * (e >> 2) + 4 * lh) * g.K + col] = acc[i][j][e];
    }
    if (dob && lr == 0) {
#pragma unroll
      for (int e = 0; e < 16; ++e) out[(int64_t)g.Cout * g.K + cob + (e & 3) + 8 * (e >> 2) + 4 * lh] = accb[i][e];
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------
bool patchconv_supported(int64_t C, int64_t Cout, int64_t k) {
  if (Cout <= 0 || Cout % 32 != 0) return false;
  if (k == 2) return C > 0 && C % 32 == 0;
  return k == 4 && C == 3;
}

static pc::Geom pc_geom(int64_t N, int H, int W, int C, int Cout, int k) {
  pc::Geom g;
  g.H = H; g.W = W; g.C = C; g.Ho = H / k; g.Wo = W / k; g.Cout = Cout; g.k = k;
  g.M = (int)(N * g.Ho * g.Wo);
  g.K = k * k * C;
  return g;
}

void launch_patchconv_fwd(int kind, bool x_f32, const void* x, const uint16_t* w, const void* bias, int bias_kind,
                          uint16_t* y, int64_t N, int H, int W, int C, int Cout, int k, hipStream_t s) {
  const pc::Geom g = pc_geom(N, H, W, C, Cout, k);
  if (g.M == 0) return;
  const int ntiles = (Cout + pc::TN - 1) / pc::TN;
  const dim3 gr((unsigned)(((g.M + pc::TM - 1) / pc::TM) * ntiles)), bl(pc::NT);
  with_bool(kind == 2, [&](auto f16) {
    constexpr bool F16 = decltype(f16)::value;
    if (k == 2) {
      hipLaunchKernelGGL((patchconv_fwd_kernel<F16>), gr, bl, 0, s, static_cast<const uint16_t*>(x), w, bias,
                         bias_kind, y, g, ntiles);
    } else {
      with_bool(x_f32, [&](auto f32) {
        hipLaunchKernelGGL((patchconv_stem_fwd_kernel<F16, decltype(f32)::value>), gr, bl, 0, s, x, w, bias,
                           bias_kind, y, g, ntiles);
      });
    }
  });
}

void launch_patchconv_dgrad(int kind, const uint16_t* dy, const uint16_t* w, uint16_t* dx, int64_t N, int H, int W,
                            int C, int Cout, hipStream_t s) {
  const pc::Geom g = pc_geom(N, H, W, C, Cout, 2);
  if (g.M == 0) return;
  const int ktiles = g.K / pc::TN;  // K = 4C, C % 32 == 0
  const dim3 gr((unsigned)(((g.M + pc::TM - 1) / pc::TM) * ktiles)), bl(pc::NT);
  with_bool(kind == 2, [&](auto f16) {
    hipLaunchKernelGGL((patchconv_dgrad_kernel<decltype(f16)::value>), gr, bl, 0, s, dy, w, dx, g, ktiles);
  });
}

static int pc_wgrad_tiles(int Cout, int C, int k, int* ctiles, int* ktiles) {
  const int tk = k == 4 ? 64 : 128;
  *ctiles = (Cout + pc::TN - 1) / pc::TN;
  *ktiles = (k * k * C + tk - 1) / tk;
  return *ctiles * *ktiles;
}

int patchconv_wgrad_slices(int64_t M, int Cout, int C, int k) {
  int ct, kt;
  const int64_t tiles = pc_wgrad_tiles(Cout, C, k, &ct, &kt);
  const int64_t nsteps = (M + pc::BK - 1) / pc::BK;
  int64_t S = (2 * 256 + tiles - 1) / tiles;  // slices x tiles: about two workgroups per CU
  if (S > nsteps / 4) S = nsteps / 4;         // at least four K-steps per slice
  if (S < 1) S = 1;
  const int64_t sps = (nsteps + S - 1) / S;
  return (int)(sps > 0 ? (nsteps + sps - 1) / sps : 1);  // no empty slice
}

void launch_patchconv_wgrad(int kind, bool x_f32, const uint16_t* dy, const void* x, float* part, int64_t N, int H,
                            int W, int C, int Cout, int k, int S, hipStream_t s) {
  const pc::Geom g = pc_geom(N, H, W, C, Cout, k);
  int ct, kt;
  const int tiles = pc_wgrad_tiles(Cout, C, k, &ct, &kt);
  const int nsteps = (g.M + pc::BK - 1) / pc::BK;
  const int sps = (nsteps + S - 1) / S;
  const dim3 gr((unsigned)(tiles * S)), bl(pc::NT);
  with_bool(kind == 2, [&](auto f16) {
    constexpr bool F16 = decltype(f16)::value;
    if (k == 2) {
      hipLaunchKernelGGL((patchconv_wgrad_kernel<F16, false, false>), gr, bl, 0, s, dy, x, part, g, ct, kt, sps);
    } else {
      with_bool(x_f32, [&](auto f32) {
        hipLaunchKernelGGL((patchconv_wgrad_kernel<F16, true, decltype(f32)::value>), gr, bl, 0, s, dy, x, part, g,
                           ct, kt, sps);
      });
    }
  });
}

}  // namespace dpt
