// Fused multi-head self-attention (forward + backward) for sequences that do not fit on chip
// (ViT-B/16 above 256 px: 290 .. 1025 tokens), gfx950 MFMA.
//
// attn_kernels.hip holds a whole head in LDS and stops at 256 tokens.  Here one side of every
// product stays in a wave's registers and the other side streams through LDS in 128-row chunks,
// so the sequence length is bounded only by the launch (S <= 4096).  The arithmetic is that of
// attn_kernels.hip: bf16 operands, v_mfma_f32_32x32x16_bf16, scores computed transposed (keys x
// queries: a query's keys are one lane's registers plus its xor-32 partner), P and dS rounded to
// bf16 only as MFMA operands, fp32 accumulation, attn_exp2 for every exponential, Q/K/V read
// straight from [B, S, 3, H, 64], context and dQ/dK/dV written straight into their consumers'
// layouts, lse2 [B*H, attn_lse_stride(S)].  No atomics: every output element has one owner.
//
//   forward   workgroup = QB queries of one (image, head), wave = 32 queries (Q in registers);
//             per chunk of KC keys: S^T = K Q^T, running max m and sum l per query (online
//             softmax), o and l rescaled by exp2((m_old - m_new) scale_log2), O^T += V^T P^T.
//   backward  (1) D[q] = rowsum(dO * O) once per (image, head) into a [B*H, stride] scratch;
//             (2) dK / dV: workgroup = QB keys, wave = 32 keys (K, V in registers), Q / dO / lse2 /
//                 D stream in chunks of QC query rows (attn_kernels.hip's phase 1);
//             (3) dQ: workgroup = QB queries, wave = 32 queries, K / V stream in chunks of KC
//                 keys (phase 2).
// Workgroups of one (image, head) are adjacent in the grid (the block index within the head is
// the fast one), so they run together and share that head's K / V (or Q / dO) in L2.
// Padding keys (>= S) exist only in the last chunk and are masked to probability 0 before the
// max (forward) and ahead of the exponential (backward); padding queries are never stored and
// get lse2 = +inf in the backward, so they add nothing to dK / dV.
#include <cmath>

#include "attn_common.h"
#include "common.h"
#include "kernels.h"
#include "mfma.h"

namespace dpt {

namespace attn_stream {
constexpr int NW = 4;         // waves per workgroup
constexpr int QB = NW * 32;   // queries (forward, dQ) or keys (dK / dV) a workgroup owns
constexpr int KC = 128;       // keys per streamed chunk (forward, dQ)
constexpr int QC = 128;       // query rows per streamed chunk (dK / dV)
constexpr int NTH = NW * 64;
constexpr int MAX_S = 4096;
}  // namespace attn_stream

// 16-byte row fragment of a [S, ld] bf16 matrix straight from global memory (rows >= S: zero)
__device__ __forceinline__ bf16x8_t attn_stream_gfrag(const uint16_t* src, int64_t ld, int row, int ch, int S) {
  uint4 v = make_uint4(0, 0, 0, 0);
  if (row < S) v = *reinterpret_cast<const uint4*>(src + (int64_t)row * ld + ch * 8);
  return __builtin_bit_cast(bf16x8_t, v);
}

// 32 queries (this lane's column) x 64 dims (registers of two tiles) -> [.., S, .., 64] rows
__device__ __forceinline__ void attn_stream_store_rows(uint16_t* row, const f32x16_t (&x)[2], float f, int h) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {  // rows d = 32dt + 8g + 4h + 0..3 (registers 4g..4g+3)
      const f32x2_t v0 = {x[dt][4 * g] * f, x[dt][4 * g + 1] * f};
      const f32x2_t v1 = {x[dt][4 * g + 2] * f, x[dt][4 * g + 3] * f};
      uint2 pk;
      pk.x = __builtin_bit_cast(uint32_t, __builtin_convertvector(v0, bf16x2_t));
      pk.y = __builtin_bit_cast(uint32_t, __builtin_convertvector(v1, bf16x2_t));
      *reinterpret_cast<uint2*>(row + dt * 32 + 8 * g + 4 * h) = pk;
    }
}

// grid: (B*H) * nqb workgroups, block = bh * nqb + query block
// (two waves per SIMD: left to itself the compiler takes 274 registers and one)
__global__ __launch_bounds__(attn_stream::NTH, 2) void attn_stream_fwd_kernel(const uint16_t* __restrict__ qkv,
                                                                              uint16_t* __restrict__ ctx,
                                                                              float* __restrict__ lse2, int S, int H,
                                                                              int nqb, int stride, float scale_log2) {
  using namespace attn;
  using namespace attn_stream;
  constexpr int KT = KC / 32;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * KC * RB];
  unsigned char* kimg = lds;
  unsigned char* vimg = lds + KC * RB;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
  const int b = bh / H, hh = bh - b * H;
  const int64_t ld = 3LL * H * D;
  const uint16_t* base = qkv + (int64_t)b * S * ld;
  const uint16_t* kbase = base + (int64_t)(H + hh) * D;
  const uint16_t* vbase = base + (int64_t)(2 * H + hh) * D;
  const int r = lane & 31, h = lane >> 5;
  const int q = qb * QB + w * 32 + r;
  const bool live = qb * QB + w * 32 < S;  // a wave of padding queries only stages and waits

  bf16x8_t qf[4];  // B operand of S^T = K Q^T: Q[q][16s + 8h .. +7]
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = attn_stream_gfrag(base + (int64_t)hh * D, ld, q, 2 * s + h, S);

  float m = -INFINITY, l = 0.f;  // running maximum of the raw scores and sum of exp2, per query
  f32x16_t o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;

  for (int c0 = 0; c0 < S; c0 += KC) {
    if (c0) __syncthreads();  // the previous chunk's reads are done
    attn_stage(kimg, kbase + (int64_t)c0 * ld, ld, S - c0, KC, tid, NTH);
    attn_stage(vimg, vbase + (int64_t)c0 * ld, ld, S - c0, KC, tid, NTH);
    __syncthreads();
    if (!live) continue;
    const int nkt = min(KT, (S - c0 + 31) / 32);  // key tiles with a real key (>= 1: c0 < S)
    f32x16_t sc[KT];
    float mc = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      if (kt < nkt) {
#pragma unroll
        for (int e = 0; e < 16; ++e) sc[kt][e] = 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s) sc[kt] = mfma32(row_frag<RB>(kimg, kt * 32 + r, 2 * s + h), qf[s], sc[kt]);
        if (c0 + (kt + 1) * 32 > S) {  // padding keys: only in the last tile of the last chunk
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int key = c0 + kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (key >= S) sc[kt][e] = -INFINITY;
          }
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) mc = fmaxf(mc, sc[kt][e]);
      }
    }
    mc = fmaxf(mc, __shfl_xor(mc, 32, 64));
    // every chunk holds a real key, so m_new is finite and the first chunk's factor is
    // exp2(-inf) = 0, never exp2(-inf - -inf)
    const float m_new = fmaxf(m, mc);
    const float alpha = attn_exp2((m - m_new) * scale_log2);
    const float ms = m_new * scale_log2;
    m = m_new;
    float lc = 0.f;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      if (kt < nkt) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float pv = attn_exp2(__builtin_fmaf(sc[kt][e], scale_log2, -ms));
          sc[kt][e] = pv;
          lc += pv;
        }
      }
    }
    lc += __shfl_xor(lc, 32, 64);
    l = __builtin_fmaf(l, alpha, lc);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[dt][e] *= alpha;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      if (kt < nkt) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const bf16x8_t pf = acc_frag(sc[kt], s2);
#pragma unroll
          for (int dt = 0; dt < 2; ++dt)
            o[dt] = mfma32(tr_frag<RB, true>(vimg, kt * 32 + 16 * s2, dt * 32, lane), pf, o[dt]);
        }
      }
    }
  }
  if (q < S) {
    attn_stream_store_rows(ctx + ((int64_t)b * S + q) * H * D + hh * D, o, 1.0f / l, h);
    if (h == 0) lse2[(int64_t)bh * stride + q] = m * scale_log2 + log2f(l);
  }
}

// D[q] = sum_d dO * O (fp32, from the bf16 output): 8 lanes per [64]-row, one 16-byte load of
// each operand per lane; rows = B*S*H in memory order, dsum [B*H, stride]
__global__ __launch_bounds__(256) void attn_stream_dsum_kernel(const uint16_t* __restrict__ out,
                                                               const uint16_t* __restrict__ dout,
                                                               float* __restrict__ dsum, int S, int H, int stride,
                                                               int64_t rows) {
  const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
  const int c = threadIdx.x & 7;
  float acc = 0.f;
  if (g < rows) {
    const uint4 a = *reinterpret_cast<const uint4*>(out + g * 64 + c * 8);
    const uint4 d = *reinterpret_cast<const uint4*>(dout + g * 64 + c * 8);
    const uint32_t ua[4] = {a.x, a.y, a.z, a.w}, ud[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      acc = __builtin_fmaf(bf16_to_f32(ua[k] & 0xffff), bf16_to_f32(ud[k] & 0xffff), acc);
      acc = __builtin_fmaf(bf16_to_f32(ua[k] >> 16), bf16_to_f32(ud[k] >> 16), acc);
    }
  }
  acc += __shfl_xor(acc, 1, 64);
  acc += __shfl_xor(acc, 2, 64);
  acc += __shfl_xor(acc, 4, 64);
  if (g < rows && c == 0) {
    const int64_t bs = g / H;
    const int hh = (int)(g - bs * H);
    const int64_t b = bs / S;
    const int s = (int)(bs - b * S);
    dsum[(b * H + hh) * stride + s] = acc;
  }
}

// dK / dV: grid (B*H) * nkb workgroups, block = bh * nkb + key block; wave = 32 keys
__global__ __launch_bounds__(attn_stream::NTH) void attn_stream_dkdv_kernel(
    const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dout, const float* __restrict__ lse2,
    const float* __restrict__ dsum, uint16_t* __restrict__ dqkv, int S, int H, int nkb, int stride,
    float scale_log2, float scale) {
  using namespace attn;
  using namespace attn_stream;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * QC * RB + 2 * QC * 4];
  unsigned char* qimg = lds;
  unsigned char* oimg = lds + QC * RB;  // dO
  float* ls = reinterpret_cast<float*>(lds + 2 * QC * RB);
  float* dd = ls + QC;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int bh = blockIdx.x / nkb, kb = blockIdx.x - bh * nkb;
  const int b = bh / H, hh = bh - b * H;
  const int64_t ld = 3LL * H * D, ldo = (int64_t)H * D;
  const uint16_t* base = qkv + (int64_t)b * S * ld;
  const uint16_t* qbase = base + (int64_t)hh * D;
  const uint16_t* obase = dout + (int64_t)b * S * ldo + hh * D;
  const int r = lane & 31, h = lane >> 5;
  const int k0 = kb * QB + w * 32, key = k0 + r;
  const bool live = k0 < S;  // a wave of padding keys only stages and waits

  bf16x8_t kf[4], vf[4];  // B operands: K[key][d], V[key][d] rows
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    kf[s] = attn_stream_gfrag(base + (int64_t)(H + hh) * D, ld, key, 2 * s + h, S);
    vf[s] = attn_stream_gfrag(base + (int64_t)(2 * H + hh) * D, ld, key, 2 * s + h, S);
  }
  f32x16_t dv[2], dk[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) { dv[dt][e] = 0.f; dk[dt][e] = 0.f; }

  for (int c0 = 0; c0 < S; c0 += QC) {
    if (c0) __syncthreads();
    attn_stage(qimg, qbase + (int64_t)c0 * ld, ld, S - c0, QC, tid, NTH);
    attn_stage(oimg, obase + (int64_t)c0 * ldo, ldo, S - c0, QC, tid, NTH);
    for (int t = tid; t < QC; t += NTH) {  // lse2 (+inf for padding queries: P = 0) and D
      const int qq = c0 + t;
      ls[t] = qq < S ? lse2[(int64_t)bh * stride + qq] : INFINITY;
      dd[t] = qq < S ? dsum[(int64_t)bh * stride + qq] : 0.f;
    }
    __syncthreads();
    if (!live) continue;
    const int nqt = min(QC / 32, (S - c0 + 31) / 32);  // query tiles with a real query
    for (int qt = 0; qt < nqt; ++qt) {
      f32x16_t sc, dp;
#pragma unroll
      for (int e = 0; e < 16; ++e) { sc[e] = 0.f; dp[e] = 0.f; }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sc = mfma32(row_frag<RB>(qimg, qt * 32 + r, 2 * s + h), kf[s], sc);   // S = Q K^T
        dp = mfma32(row_frag<RB>(oimg, qt * 32 + r, 2 * s + h), vf[s], dp);   // dP = dO V^T
      }
      // rows = queries, column = this lane's key: rows (e & 3) of group e >> 2 are 4 consecutive
      // queries, so their lse2 / D values come in one 16-byte LDS read each
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) {
        const int q4 = qt * 32 + 8 * e4 + 4 * h;
        const float4 l4 = *reinterpret_cast<const float4*>(ls + q4);
        const float4 d4 = *reinterpret_cast<const float4*>(dd + q4);
        const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dv4[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int e = 4 * e4 + j;
          const float pv = key < S ? attn_exp2(__builtin_fmaf(sc[e], scale_log2, -lv[j])) : 0.f;
          sc[e] = pv;
          dp[e] = pv * (dp[e] - dv4[j]);
        }
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8_t pa = acc_frag(sc, s2), da = acc_frag(dp, s2);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dv[dt] = mfma32(pa, tr_frag<RB, true>(oimg, qt * 32 + 16 * s2, dt * 32, lane), dv[dt]);  // P^T dO
          dk[dt] = mfma32(da, tr_frag<RB, true>(qimg, qt * 32 + 16 * s2, dt * 32, lane), dk[dt]);  // dS^T Q
        }
      }
    }
  }
  if (!live) return;
  // rows = keys (registers), column = d (lane)
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int kk = k0 + (e & 3) + 8 * (e >> 2) + 4 * h;
      if (kk < S) {
        uint16_t* row = dqkv + ((int64_t)b * S + kk) * ld;
        row[(int64_t)(H + hh) * D + dt * 32 + r] = f32_to_bf16(dk[dt][e] * scale);
        row[(int64_t)(2 * H + hh) * D + dt * 32 + r] = f32_to_bf16(dv[dt][e]);
      }
    }
}

// dQ: grid (B*H) * nqb workgroups, block = bh * nqb + query block; wave = 32 queries
__global__ __launch_bounds__(attn_stream::NTH) void attn_stream_dq_kernel(
    const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dout, const float* __restrict__ lse2,
    const float* __restrict__ dsum, uint16_t* __restrict__ dqkv, int S, int H, int nqb, int stride,
    float scale_log2, float scale) {
  using namespace attn;
  using namespace attn_stream;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * KC * RB];
  unsigned char* kimg = lds;
  unsigned char* vimg = lds + KC * RB;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
  const int b = bh / H, hh = bh - b * H;
  const int64_t ld = 3LL * H * D, ldo = (int64_t)H * D;
  const uint16_t* base = qkv + (int64_t)b * S * ld;
  const uint16_t* kbase = base + (int64_t)(H + hh) * D;
  const uint16_t* vbase = base + (int64_t)(2 * H + hh) * D;
  const int r = lane & 31, h = lane >> 5;
  const int q = qb * QB + w * 32 + r;
  const bool live = qb * QB + w * 32 < S;

  bf16x8_t qf[4], of[4];  // B operands of S^T = K Q^T and dP^T = V dO^T
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qf[s] = attn_stream_gfrag(base + (int64_t)hh * D, ld, q, 2 * s + h, S);
    of[s] = attn_stream_gfrag(dout + (int64_t)b * S * ldo + hh * D, ldo, q, 2 * s + h, S);
  }
  const float lq = q < S ? lse2[(int64_t)bh * stride + q] : INFINITY;
  const float dq0 = q < S ? dsum[(int64_t)bh * stride + q] : 0.f;
  f32x16_t dq[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) dq[dt][e] = 0.f;

  for (int c0 = 0; c0 < S; c0 += KC) {
    if (c0) __syncthreads();
    attn_stage(kimg, kbase + (int64_t)c0 * ld, ld, S - c0, KC, tid, NTH);
    attn_stage(vimg, vbase + (int64_t)c0 * ld, ld, S - c0, KC, tid, NTH);
    __syncthreads();
    if (!live) continue;
    const int nkt = min(KC / 32, (S - c0 + 31) / 32);
    for (int kt = 0; kt < nkt; ++kt) {
      f32x16_t st, dpt;
#pragma unroll
      for (int e = 0; e < 16; ++e) { st[e] = 0.f; dpt[e] = 0.f; }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        st = mfma32(row_frag<RB>(kimg, kt * 32 + r, 2 * s + h), qf[s], st);
        dpt = mfma32(row_frag<RB>(vimg, kt * 32 + r, 2 * s + h), of[s], dpt);
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {  // rows = keys, column = this lane's query
        const int key = c0 + kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        const float pv = key < S ? attn_exp2(__builtin_fmaf(st[e], scale_log2, -lq)) : 0.f;
        st[e] = pv * (dpt[e] - dq0);
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8_t df = acc_frag(st, s2);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
          dq[dt] = mfma32(tr_frag<RB, true>(kimg, kt * 32 + 16 * s2, dt * 32, lane), df, dq[dt]);  // K^T dS^T
      }
    }
  }
  if (q < S) attn_stream_store_rows(dqkv + ((int64_t)b * S + q) * ld + (int64_t)hh * D, dq, scale, h);
}

bool attn_stream_supported(int S, int Dh) { return Dh == attn::D && S >= 1 && S <= attn_stream::MAX_S; }

void attn_stream_tiles(int* queries_per_wg, int* keys_per_chunk, int* query_rows_per_bwd_chunk) {
  *queries_per_wg = attn_stream::QB;
  *keys_per_chunk = attn_stream::KC;
  *query_rows_per_bwd_chunk = attn_stream::QC;
}

void launch_attn_stream_fwd(const uint16_t* qkv, uint16_t* ctx, float* lse2, int B, int S, int H, float scale,
                            hipStream_t st) {
  using namespace attn_stream;
  const int nqb = (S + QB - 1) / QB;
  const float sl2 = scale * 1.4426950408889634f;
  hipLaunchKernelGGL(attn_stream_fwd_kernel, dim3((unsigned)(B * H * nqb)), dim3(NTH), 0, st, qkv, ctx, lse2, S, H,
                     nqb, attn_lse_stride(S), sl2);
}

void launch_attn_stream_bwd(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse2,
                            float* dsum, uint16_t* dqkv, int B, int S, int H, float scale, hipStream_t st) {
  using namespace attn_stream;
  const int nb = (S + QB - 1) / QB, stride = attn_lse_stride(S);
  const float sl2 = scale * 1.4426950408889634f;
  const int64_t rows = (int64_t)B * S * H;
  hipLaunchKernelGGL(attn_stream_dsum_kernel, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, st, out, dout,
                     dsum, S, H, stride, rows);
  const dim3 grid((unsigned)(B * H * nb));
  hipLaunchKernelGGL(attn_stream_dkdv_kernel, grid, dim3(NTH), 0, st, qkv, dout, lse2, dsum, dqkv, S, H, nb, stride,
                     sl2, scale);
  hipLaunchKernelGGL(attn_stream_dq_kernel, grid, dim3(NTH), 0, st, qkv, dout, lse2, dsum, dqkv, S, H, nb, stride,
                     sl2, scale);
}

}  // namespace dpt
