// Depthwise KxK "same" convolutions (stride 1, pad (K-1)/2, K in {3, 5, 7}) for gfx950:
// forward, backward-data and backward-weight (+ bias gradient) of ConvNeXt's 7x7 conv.
//
// With one input channel per group there is no GEMM and nothing for the matrix cores: each
// output is K*K multiply-adds on its own channel, so the kernels are HBM streams whose design
// question is how the halo moves.  Layout is channels-last, x / y / dy [N, H, W, C] with
// C % 8 == 0: one lane owns 8 channels of one pixel as one 16-byte vector (8 lanes cover a
// 64-channel block, 128 contiguous bytes of a pixel).  Operands are bf16 or fp16 (KIND 1 / 2),
// accumulation fp32, element offsets 64-bit.
//
// Activation type (ACT_F32): the forward's x and the backward-weight's x may be fp32 (the
// residual stream under autocast); each element is rounded to the operand type as it is
// staged into LDS - bit for bit the value autocast's cast kernel would have written - and
// backward-data then writes dx as fp32.  No cast pass, no 16-bit copy of x, no 16-bit dx.
//
// dwconv_kernel<K, KIND, ACT_F32, DGRAD, TH, TW, RUN>  (forward, and backward-data with DGRAD)
//   grid (pixel tiles, N, channel blocks of 64); block = TH * (TW / RUN) pixel lanes x 8
//   channel lanes.  Two geometries: 16x16 pixels with runs of 8 (256 threads) and, for images
//   with an edge <= 8 (ConvNeXt's 7x7 stage, where a 16x16 tile idles four fifths of its
//   lanes), 8x8 pixels with runs of 4 (128 threads).
//   1. Stage: the (TH+K-1) x (TW+K-1) x 64 halo, 16-bit, with 16-byte loads, zeros outside the
//      image and past C.  The row pitch is padded to an odd pixel count so that two lanes on
//      neighbouring rows (one 16-lane LDS pass) fall into different bank halves.  The K*K taps
//      of the channel block (read flipped, w[c][K-1-r][K-1-s], under DGRAD) and the bias go
//      to LDS as fp32, [tap][channel].
//      LDS, K = 7, 16x16: 22 x 23 x 128 B = 64,768 + taps 12,544 + bias 256 = 77,568 B: two
//      blocks per CU of the 160 KB.  8x8: 14 x 15 x 128 + 12,800 = 39,680 B.
//   2. Compute: a lane makes RUN consecutive outputs of one row for its 8 channels.  For each
//      tap row it walks the RUN+K-1 halo vectors of that row once; each vector feeds the up to
//      K outputs of the run that it touches (the window slides through registers).  An LDS
//      element is read K * (RUN+K-1) / RUN times (12.25 at K = 7, RUN = 8) instead of K*K = 49.
//      Registers: RUN x 8 = 64 fp32 accumulators + K x 8 = 56 taps of the current row + one
//      vector.  Order of additions is fixed (r, then s), bias added in fp32, one rounding.
//   Bytes per pass: x once (halo overlap (22/16)^2 = 1.9x is served by L2) and y once.
//
// dwconv_wgrad_kernel<K, KIND, ACT_F32>  (dw and db partials)
//   grid (S pixel slices, channel blocks of 64), 256 threads.  A block walks its slice of the
//   8 x 16 pixel tiles of (n, h, w); per tile it stages the 16-bit x halo (14 x 23 x 128 B at
//   K = 7) and the dy tile (8 x 16 x 128 B): 57,600 B, two blocks per CU.
//   A lane owns 8 channels x one tap ROW r x one share of the tile's rows: lanes are
//   (channel lane 0..7) x (slot 0..SLOTS-1) x (share 0..SHARES-1), SLOTS = 8 (4 at K = 3),
//   slot r < K the tap row, slot K the bias term, SHARES = 32 / SLOTS = 4 (8).  That is K x 8 =
//   56 fp32 accumulators per lane (8 for the bias lanes): all K*K taps in one lane would be 392,
//   far past the register file, and one tap per lane would re-read x and dy K*K times.  Within
//   a row the lane keeps a run of 8 dy vectors in registers and streams the 8+K-1 x vectors
//   past them, the forward's sliding window transposed.
//   After the slice the shares are summed through LDS in a fixed order and the block writes
//   its fp32 partials part[slice][C*K*K + C] (dw as [c][r][s], then db); the colsum_rows kernel
//   (vit_kernels.hip) adds the S slices in a fixed order and casts.  No atomics: two runs
//   agree bit for bit.  S is chosen so that S x channel blocks is about twice the 256 CUs.
//   Bytes per pass: x once, dy once, plus S x C x (K*K+1) x 4 B of partials (4.9 MB at
//   ConvNeXt-T's first stage, batch 128, against 154 MB of x as fp32).
#include "common.h"
#include "kernels.h"

namespace dpt {

constexpr int kDwCB = 64;  // channels per block: 8 lanes x 8 channels

template <int KIND>
__device__ __forceinline__ float dw_h2f(uint32_t h) {
  return KIND == 1 ? bf16_to_f32((uint16_t)h) : f16_to_f32((uint16_t)h);
}
template <int KIND>
__device__ __forceinline__ uint32_t dw_f2h(float f) {
  return KIND == 1 ? (uint32_t)f32_to_bf16(f) : (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f);
}
template <int KIND>
__device__ __forceinline__ void dw_unpack(uint4 q, float v[8]) {
  const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[2 * k] = dw_h2f<KIND>(u[k] & 0xffff);
    v[2 * k + 1] = dw_h2f<KIND>(u[k] >> 16);
  }
}
template <int KIND>
__device__ __forceinline__ uint4 dw_pack(const float v[8]) {
  uint4 q;
  q.x = dw_f2h<KIND>(v[0]) | (dw_f2h<KIND>(v[1]) << 16);
  q.y = dw_f2h<KIND>(v[2]) | (dw_f2h<KIND>(v[3]) << 16);
  q.z = dw_f2h<KIND>(v[4]) | (dw_f2h<KIND>(v[5]) << 16);
  q.w = dw_f2h<KIND>(v[6]) | (dw_f2h<KIND>(v[7]) << 16);
  return q;
}

// 8 channels of one pixel as 16-bit operands: a 16-byte load, or (F32) two of them rounded.
template <int KIND, bool F32>
__device__ __forceinline__ uint4 dw_load8(const void* base, int64_t off) {
  if (!F32) return *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(base) + off);
  const float4* p = reinterpret_cast<const float4*>(static_cast<const float*>(base) + off);
  const float4 a = p[0], b = p[1];
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  return dw_pack<KIND>(v);
}

// Stage rows x cols pixels (pitch in pixels) x 64 channels from image n at (h0, w0) into LDS,
// zeros outside the image and past C.
template <int KIND, bool F32, int NT>
__device__ __forceinline__ void dw_stage(uint4* lds, int rows, int cols, int pitch, const void* src, int64_t n,
                                         int h0, int w0, int c0, int H, int W, int C) {
  for (int i = threadIdx.x; i < rows * cols * 8; i += NT) {
    const int cg = i & 7, pix = i >> 3;
    const int hr = pix / cols, hc = pix - hr * cols;
    const int gh = h0 + hr, gw = w0 + hc, c = c0 + cg * 8;
    uint4 q = make_uint4(0, 0, 0, 0);
    if (gh >= 0 && gh < H && gw >= 0 && gw < W && c < C)
      q = dw_load8<KIND, F32>(src, ((n * H + gh) * W + gw) * (int64_t)C + c);
    lds[(hr * pitch + hc) * 8 + cg] = q;
  }
}

template <int K, int KIND, bool ACT_F32, bool DGRAD, int TH, int TW, int RUN>
__global__ __launch_bounds__(TH*(TW / RUN) * 8) void dwconv_kernel(const void* __restrict__ in,
                                                                   const uint16_t* __restrict__ w,
                                                                   const void* __restrict__ bias, int bias_kind,
                                                                   void* __restrict__ out, int H, int W, int C,
                                                                   int tiles_w) {
  constexpr int NT = TH * (TW / RUN) * 8, P = (K - 1) / 2;
  constexpr int HR = TH + K - 1, HC = TW + K - 1, PITCH = HC | 1;
  constexpr bool IN_F32 = ACT_F32 && !DGRAD, OUT_F32 = ACT_F32 && DGRAD;
  __shared__ uint4 halo[HR * PITCH * 8];
  __shared__ float taps[K * K * kDwCB];
  __shared__ float bsh[kDwCB];

  const int tile = blockIdx.x, th = tile / tiles_w, tw = tile - th * tiles_w;
  const int64_t n = blockIdx.y;
  const int c0 = blockIdx.z * kDwCB, h0 = th * TH, w0 = tw * TW;

  dw_stage<KIND, IN_F32, NT>(halo, HR, HC, PITCH, in, n, h0 - P, w0 - P, c0, H, W, C);
  for (int i = threadIdx.x; i < kDwCB * K * K; i += NT) {
    const int cl = i / (K * K), t = i - cl * (K * K);
    const int c = c0 + cl;
    const float v = c < C ? dw_h2f<KIND>(w[(int64_t)c * (K * K) + t]) : 0.f;
    taps[(DGRAD ? K * K - 1 - t : t) * kDwCB + cl] = v;
  }
  if (threadIdx.x < kDwCB) {
    const int c = c0 + threadIdx.x;
    float b = 0.f;
    if (!DGRAD && bias != nullptr && c < C) {
      if (bias_kind == 0) b = static_cast<const float*>(bias)[c];
      else b = dw_h2f<KIND>(static_cast<const uint16_t*>(bias)[c]);
    }
    bsh[threadIdx.x] = b;
  }
  __syncthreads();

  const int cg = threadIdx.x & 7, pl = threadIdx.x >> 3;
  const int row = pl % TH, q0 = (pl / TH) * RUN;
  float acc[RUN][8];
#pragma unroll
  for (int o = 0; o < RUN; ++o)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[o][c] = 0.f;

#pragma unroll 1
  for (int r = 0; r < K; ++r) {
    float wr[K][8];
#pragma unroll
    for (int s = 0; s < K; ++s) {
      const float4* tp = reinterpret_cast<const float4*>(taps + (r * K + s) * kDwCB + cg * 8);
      const float4 a = tp[0], b = tp[1];
      wr[s][0] = a.x; wr[s][1] = a.y; wr[s][2] = a.z; wr[s][3] = a.w;
      wr[s][4] = b.x; wr[s][5] = b.y; wr[s][6] = b.z; wr[s][7] = b.w;
    }
    const uint4* hp = halo + ((row + r) * PITCH + q0) * 8 + cg;
#pragma unroll
    for (int j = 0; j < RUN + K - 1; ++j) {
      float v[8];
      dw_unpack<KIND>(hp[j * 8], v);
#pragma unroll
      for (int s = 0; s < K; ++s) {
        const int o = j - s;
        if (o >= 0 && o < RUN) {
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[o][c] = fmaf(v[c], wr[s][c], acc[o][c]);
        }
      }
    }
  }

  const int gh = h0 + row, c = c0 + cg * 8;
  if (gh < H && c < C) {
    float b[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) b[k] = bsh[cg * 8 + k];
#pragma unroll
    for (int o = 0; o < RUN; ++o) {
      const int gw = w0 + q0 + o;
      if (gw < W) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = acc[o][k] + b[k];
        const int64_t off = ((n * H + gh) * W + gw) * (int64_t)C + c;
        if (OUT_F32) {
          float4* op = reinterpret_cast<float4*>(static_cast<float*>(out) + off);
          op[0] = make_float4(v[0], v[1], v[2], v[3]);
          op[1] = make_float4(v[4], v[5], v[6], v[7]);
        } else {
          *reinterpret_cast<uint4*>(static_cast<uint16_t*>(out) + off) = dw_pack<KIND>(v);
        }
      }
    }
  }
}

// ---- backward-weight ----------------------------------------------------------------------------
constexpr int kWgTH = 8, kWgTW = 16, kWgRun = 8, kWgNT = 256;

template <int K>
struct WgGeom {
  static constexpr int SLOTS = K + 1 <= 4 ? 4 : 8;
  static constexpr int SHARES = 32 / SLOTS;
  static constexpr int HR = kWgTH + K - 1, HC = kWgTW + K - 1, PITCH = HC | 1;
  static constexpr int STAGE_BYTES = (HR * PITCH + kWgTH * kWgTW) * 8 * 16;
  static constexpr int NOUT = (K * K + 1) * kDwCB;  // per-block outputs: [tap][channel], then bias
  static constexpr int RED_BYTES = SHARES * NOUT * 4;
  static constexpr int LDS_BYTES = STAGE_BYTES > RED_BYTES ? STAGE_BYTES : RED_BYTES;
};

template <int K, int KIND, bool ACT_F32>
__global__ __launch_bounds__(kWgNT) void dwconv_wgrad_kernel(const uint16_t* __restrict__ dy,
                                                             const void* __restrict__ x,
                                                             float* __restrict__ part, int H, int W, int C,
                                                             int tiles_h, int tiles_w, int64_t n_tiles,
                                                             int64_t tiles_per_slice) {
  using G = WgGeom<K>;
  constexpr int P = (K - 1) / 2;
  __shared__ uint4 lds[G::LDS_BYTES / 16];
  uint4* xh = lds;
  uint4* dyt = lds + G::HR * G::PITCH * 8;

  const int c0 = blockIdx.y * kDwCB;
  const int cg = threadIdx.x & 7, slot = (threadIdx.x >> 3) % G::SLOTS, share = (threadIdx.x >> 3) / G::SLOTS;
  float acc[K][8];
#pragma unroll
  for (int s = 0; s < K; ++s)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[s][c] = 0.f;

  const int64_t t_begin = blockIdx.x * tiles_per_slice;
  int64_t t_end = t_begin + tiles_per_slice;
  if (t_end > n_tiles) t_end = n_tiles;
  for (int64_t t = t_begin; t < t_end; ++t) {
    const int64_t n = t / (tiles_h * tiles_w);
    const int rem = (int)(t - n * (tiles_h * tiles_w));
    const int h0 = (rem / tiles_w) * kWgTH, w0 = (rem % tiles_w) * kWgTW;
    __syncthreads();  // the previous tile's readers are done
    dw_stage<KIND, ACT_F32, kWgNT>(xh, G::HR, G::HC, G::PITCH, x, n, h0 - P, w0 - P, c0, H, W, C);
    dw_stage<KIND, false, kWgNT>(dyt, kWgTH, kWgTW, kWgTW, dy, n, h0, w0, c0, H, W, C);
    __syncthreads();
    // slots past K (two of eight at K = 5) only help staging
    for (int row = share; row < kWgTH && slot <= K; row += G::SHARES) {
#pragma unroll
      for (int q0 = 0; q0 < kWgTW; q0 += kWgRun) {
        float g[kWgRun][8];
#pragma unroll
        for (int o = 0; o < kWgRun; ++o) dw_unpack<KIND>(dyt[(row * kWgTW + q0 + o) * 8 + cg], g[o]);
        if (slot == K) {  // bias term: acc[0] is the lane's db
#pragma unroll
          for (int o = 0; o < kWgRun; ++o)
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[0][c] += g[o][c];
        } else {
          const uint4* hp = xh + ((row + slot) * G::PITCH + q0) * 8 + cg;
#pragma unroll
          for (int j = 0; j < kWgRun + K - 1; ++j) {
            float v[8];
            dw_unpack<KIND>(hp[j * 8], v);
#pragma unroll
            for (int s = 0; s < K; ++s) {
              const int o = j - s;
              if (o >= 0 && o < kWgRun) {
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[s][c] = fmaf(v[c], g[o][c], acc[s][c]);
              }
            }
          }
        }
      }
    }
  }

  // Combine the shares in a fixed order: red[share][tap or bias][channel].
  __syncthreads();
  float* red = reinterpret_cast<float*>(lds);
  if (slot < K) {
#pragma unroll
    for (int s = 0; s < K; ++s)
#pragma unroll
      for (int c = 0; c < 8; ++c) red[share * G::NOUT + (slot * K + s) * kDwCB + cg * 8 + c] = acc[s][c];
  } else if (slot == K) {
#pragma unroll
    for (int c = 0; c < 8; ++c) red[share * G::NOUT + K * K * kDwCB + cg * 8 + c] = acc[0][c];
  }
  __syncthreads();
  float* dst = part + (int64_t)blockIdx.x * ((int64_t)C * (K * K + 1));
  for (int i = threadIdx.x; i < G::NOUT; i += kWgNT) {
    float sum = red[i];
#pragma unroll
    for (int q = 1; q < G::SHARES; ++q) sum += red[q * G::NOUT + i];
    const int tap = i / kDwCB, c = c0 + (i % kDwCB);
    if (c < C) {
      if (tap < K * K) dst[(int64_t)c * (K * K) + tap] = sum;
      else dst[(int64_t)C * (K * K) + c] = sum;
    }
  }
}

// ---- launchers ----------------------------------------------------------------------------------
template <int K, int KIND, bool ACT_F32, bool DGRAD>
static void dwconv_launch(const void* in, const uint16_t* w, const void* bias, int bias_kind, void* out, int64_t N, int H,
                   int W, int C, hipStream_t s) {
  const unsigned cb = (unsigned)((C + kDwCB - 1) / kDwCB);
  if (H <= kDwconvSmallTile || W <= kDwconvSmallTile) {
    constexpr int T = kDwconvSmallTile;
    const int tw = (W + T - 1) / T, th = (H + T - 1) / T;
    hipLaunchKernelGGL((dwconv_kernel<K, KIND, ACT_F32, DGRAD, T, T, 4>), dim3((unsigned)(th * tw), (unsigned)N, cb),
                       dim3(T * (T / 4) * 8), 0, s, in, w, bias, bias_kind, out, H, W, C, tw);
  } else {
    constexpr int T = kDwconvTile;
    const int tw = (W + T - 1) / T, th = (H + T - 1) / T;
    hipLaunchKernelGGL((dwconv_kernel<K, KIND, ACT_F32, DGRAD, T, T, 8>), dim3((unsigned)(th * tw), (unsigned)N, cb),
                       dim3(T * (T / 8) * 8), 0, s, in, w, bias, bias_kind, out, H, W, C, tw);
  }
}

template <int K, int KIND>
static void dwconv_launch_k(bool act_f32, bool dgrad, const void* in, const uint16_t* w, const void* bias, int bias_kind,
                     void* out, int64_t N, int H, int W, int C, hipStream_t s) {
  with_bool(act_f32, [&](auto f32) {
    with_bool(dgrad, [&](auto dg) {
      dwconv_launch<K, KIND, decltype(f32)::value, decltype(dg)::value>(in, w, bias, bias_kind, out, N, H, W, C, s);
    });
  });
}

template <int KIND>
static void dwconv_launch_kind(int K, bool act_f32, bool dgrad, const void* in, const uint16_t* w, const void* bias,
                        int bias_kind, void* out, int64_t N, int H, int W, int C, hipStream_t s) {
  if (K == 3) dwconv_launch_k<3, KIND>(act_f32, dgrad, in, w, bias, bias_kind, out, N, H, W, C, s);
  else if (K == 5) dwconv_launch_k<5, KIND>(act_f32, dgrad, in, w, bias, bias_kind, out, N, H, W, C, s);
  else dwconv_launch_k<7, KIND>(act_f32, dgrad, in, w, bias, bias_kind, out, N, H, W, C, s);
}

template <int K, int KIND>
static void dwconv_wgrad_launch(bool act_f32, const uint16_t* dy, const void* x, float* part, int64_t N, int H, int W, int C,
                         int S, hipStream_t s) {
  const int th = (H + kWgTH - 1) / kWgTH, tw = (W + kWgTW - 1) / kWgTW;
  const int64_t nt = N * th * tw, tps = (nt + S - 1) / S;
  const dim3 gr((unsigned)S, (unsigned)((C + kDwCB - 1) / kDwCB));
  with_bool(act_f32, [&](auto f32) {
    hipLaunchKernelGGL((dwconv_wgrad_kernel<K, KIND, decltype(f32)::value>), gr, dim3(kWgNT), 0, s, dy, x, part, H, W,
                       C, th, tw, nt, tps);
  });
}

bool dwconv_supported(int64_t C, int64_t K) { return C > 0 && C % 8 == 0 && (K == 3 || K == 5 || K == 7); }

void launch_dwconv(int kind, int K, bool act_f32, bool dgrad, const void* in, const uint16_t* w, const void* bias,
                   int bias_kind, void* out, int64_t N, int H, int W, int C, hipStream_t s) {
  if (kind == 1) dwconv_launch_kind<1>(K, act_f32, dgrad, in, w, bias, bias_kind, out, N, H, W, C, s);
  else dwconv_launch_kind<2>(K, act_f32, dgrad, in, w, bias, bias_kind, out, N, H, W, C, s);
}

int dwconv_wgrad_slices(int64_t N, int H, int W, int C) {
  const int64_t nt = N * ((H + kWgTH - 1) / kWgTH) * ((W + kWgTW - 1) / kWgTW);
  const int64_t cb = (C + kDwCB - 1) / kDwCB;
  int64_t S = (2 * 256 + cb - 1) / cb;  // slices x channel blocks: about two blocks per CU
  if (S > nt) S = nt;
  if (S < 1) S = 1;
  const int64_t tps = (nt + S - 1) / S;
  return (int)((nt + tps - 1) / tps);  // no empty slice: every row of the partials is written
}

void launch_dwconv_wgrad(int kind, int K, bool act_f32, const uint16_t* dy, const void* x, float* part, int64_t N,
                         int H, int W, int C, int S, hipStream_t s) {
  if (kind == 1) {
    if (K == 3) dwconv_wgrad_launch<3, 1>(act_f32, dy, x, part, N, H, W, C, S, s);
    else if (K == 5) dwconv_wgrad_launch<5, 1>(act_f32, dy, x, part, N, H, W, C, S, s);
    else dwconv_wgrad_launch<7, 1>(act_f32, dy, x, part, N, H, W, C, S, s);
  } else {
    if (K == 3) dwconv_wgrad_launch<3, 2>(act_f32, dy, x, part, N, H, W, C, S, s);
    else if (K == 5) dwconv_wgrad_launch<5, 2>(act_f32, dy, x, part, N, H, W, C, S, s);
    else dwconv_wgrad_launch<7, 2>(act_f32, dy, x, part, N, H, W, C, S, s);
  }
}

}  // namespace dpt
