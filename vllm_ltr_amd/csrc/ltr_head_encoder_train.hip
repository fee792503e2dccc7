// Training kernels of the slate encoder of the hidden-state head on gfx950 (DESIGN.md 4.4 "training the encoder").
//
// Reference: train/allrank/models/transformer.py - LayerNorm (:75-97), attention with src_mask (:153-172), wired into the
// model by models/model.py:147-161 and differentiated by autograd in training/train_utils.py:34-45.  The dense layers, the
// column sums, the norm / clip and Adam of a step are the kernels of ltr_head_train.hip; new here:
//   enc_rows_kernel      z_out = z + branch and (mean, 1 / (unbiased std + eps)) per row: the residual add of a sublayer and
//                        the statistics the next norm's tile loads read, one wave per row
//   enc_ln_bwd_kernel    dx of allRank's LayerNorm (the derivative goes through the unbiased std, eps outside the root) plus
//                        the residual branch's gradient, one wave per row
//   enc_attn_fwd_kernel  slate_attn_kernel's design (ltr_head_encoder.hip) on the rectangular [B, S] layout, with the key
//                        mask y_true == pad_value and the per-row log-sum-exp (exp2 domain) as a second output
//   enc_attn_dq_kernel   a workgroup owns 32 queries of one (slate, head), Q and dO hi | lo row-major in LDS, and walks the
//                        slate's key tiles in order, twice: S = Q K^T, P = exp2(S - LSE), dP = dO V^T give first
//                        D = sum_j P o dP per row, then dS = P o (dP - D) and dQ += dS K.  D comes from the very P and dP
//                        that dS is made of - not from sum_d dO o O, which differs from it by the rounding of O - so that a
//                        row with one valid key (P = 1) has dS = 0 exactly, as the softmax of one element has
//   enc_attn_dkv_kernel  a workgroup owns 32 keys, K and V in LDS, and walks the query tiles: S^T = K Q^T, P^T, dV += P^T dO,
//                        dP^T = V dO^T, dS^T = P^T o (dP^T - D), dK += dS^T Q; the products of the swapped operands are
//                        added in the dq kernel's order, so both kernels see the same P and dP
// Both backward kernels: 4 waves as 2 x 2.  For the 32 x 32 tiles S / dP a wave owns one 16 x 16 block and contracts over d_k
// on row-major planes; for the 32 x d_k outputs it owns 16 rows x half of d_k and contracts over the tile's 32 rows, which
// are contiguous in the P / dS tile and in the TRANSPOSED plane of the other operand.  One staging plane pair holds, in turn,
// the row-major and the transposed form of the walked operand, which keeps LDS at 59 KiB for d_k = 128 (no function
// attribute).  Three cross terms lo.hi, hi.lo, hi.hi on v_mfma_f32_16x16x32_f16, small terms first.  dO is scaled by a power
// of two from max|dO| (gradients lie far below fp16's normal range), undone exactly in the epilogue.  Masked keys, rows past
// S and the d_k pad are zero in LDS and have P = 0, so a padded item's dK and dV are exactly 0.  A query row whose slate has
// no valid key gets output 0 and passes no gradient (the reference gives NaN there).
// No atomics, no memset, no allocation; dQ | dK | dV of every row are written exactly once.
#include "ltr_internal.h"

namespace ltr {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int ET_THREADS = 256;
constexpr int ET_BQ = 64;              // forward: query rows of a workgroup
constexpr int ET_R = 32;               // backward: rows of a query tile and of a key tile
constexpr int ET_TLD = ET_R + 8;       // halves per row of a transposed plane and of the P / dS tile
constexpr float LOG2E = 1.44269504088896341f;

__device__ __forceinline__ bool key_valid(const float* __restrict__ y, float pad, size_t row) {
  return y == nullptr || y[row] != pad;
}

__global__ void __launch_bounds__(ET_THREADS) enc_rows_kernel(const float* __restrict__ z, const float* __restrict__ branch,
                                                              float* __restrict__ z_out, int M, int K,
                                                              float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (ET_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= M) return;
  const size_t o = (size_t)r * K;
  float part = 0.f;
  for (int c = lane; c < K; c += 64) {
    float v = z[o + c];
    if (branch) { v += branch[o + c]; z_out[o + c] = v; }
    part += v;
  }
  const float mean = wave_sum(part) / (float)K;
  float sq = 0.f;
  for (int c = lane; c < K; c += 64) {
    const float d = (branch ? z[o + c] + branch[o + c] : z[o + c]) - mean;
    sq += d * d;
  }
  const float sd = sqrtf(wave_sum(sq) / (float)(K - 1));
  if (lane == 0) { stats[2 * (size_t)r] = mean; stats[2 * (size_t)r + 1] = 1.f / (sd + ALLRANK_LN_EPS); }
}

// y = a_2 (x - mean) r + b_2 with r = 1 / (sd + eps), sd^2 = sum (x - mean)^2 / (K - 1).  With g = dy a_2:
// dx_j = r (g_j - mean(g)) - r^2 (sum_i g_i (x_i - mean)) (x_j - mean) / ((K - 1) sd)   (+ resid_j; dx may be resid)
__global__ void __launch_bounds__(ET_THREADS) enc_ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ stats,
                                                                const float* __restrict__ a2, const float* __restrict__ dy,
                                                                const float* resid, float* dx, int M, int K) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (ET_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= M) return;
  const size_t o = (size_t)r * K;
  const float mean = stats[2 * (size_t)r], rinv = stats[2 * (size_t)r + 1];
  float sg = 0.f, sgx = 0.f;
  for (int c = lane; c < K; c += 64) {
    const float g = dy[o + c] * a2[c];
    sg += g;
    sgx += g * (x[o + c] - mean);
  }
  sg = wave_sum(sg) / (float)K;
  sgx = wave_sum(sgx);
  const float sd = 1.f / rinv - ALLRANK_LN_EPS;
  const float coef = sd > 0.f ? rinv * rinv * sgx / ((float)(K - 1) * sd) : 0.f;
  for (int c = lane; c < K; c += 64) {
    const float v = rinv * (dy[o + c] * a2[c] - sg) - coef * (x[o + c] - mean);
    dx[o + c] = resid ? v + resid[o + c] : v;
  }
}

__device__ __forceinline__ f32x4 mfma3(f16x8 ah, f16x8 al, f16x8 bh, f16x8 bl, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc, 0, 0, 0);
}

// Rows [r0, r0 + ROWS) of one head's [n, dk] slice of a row-major tensor (pitch ld floats), times mul, split into hi | lo
// planes: row-major [ROWS][DKP + 8], or TR: transposed [DKP][ROWS + 8].  Rows from n on and the columns dk .. DKP are 0.
template <int DKP, int ROWS, bool TR>
__device__ __forceinline__ void load_tile(const float* __restrict__ src, int ld, int r0, int n, int dk, float mul,
                                          __half* __restrict__ hi, __half* __restrict__ lo) {
  constexpr int TPR = ET_THREADS / ROWS;     // loader threads per row
  const int row = threadIdx.x / TPR;
  const bool ok = r0 + row < n;
#pragma unroll
  for (int i = 0; i < DKP / 4 / TPR; ++i) {
    const int d = 4 * (threadIdx.x % TPR + TPR * i);
    float x[4];                              // d_k is a multiple of 16: a group of four is inside the head or in the pad
    load4<float, true>(src + (size_t)(r0 + row) * ld, d, ok ? dk : 0, x);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      __half h, l;
      split_f16(x[j] * mul, h, l);
      const int off = TR ? (d + j) * (ROWS + 8) + row : row * (DKP + 8) + d + j;
      hi[off] = h;
      lo[off] = l;
    }
  }
}

// A B^T over d for one 16 x 16 block: rows ra .. of A's and rows rb .. of B's row-major planes [.][DKP + 8].  SWAP: the
// terms in the order of the transposed product B A^T
template <int DKP, bool SWAP>
__device__ __forceinline__ f32x4 mma_over_d(const __half* ah, const __half* al, int ra, const __half* bh, const __half* bl,
                                            int rb, int lane) {
  constexpr int LD = DKP + 8;
  const int frow = lane & 15, fk = (lane >> 4) * 8;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < DKP / 32; ++ks) {
    const int oa = (ra + frow) * LD + ks * 32 + fk, ob = (rb + frow) * LD + ks * 32 + fk;
    const f16x8 a_h = *reinterpret_cast<const f16x8*>(ah + oa), a_l = *reinterpret_cast<const f16x8*>(al + oa);
    const f16x8 b_h = *reinterpret_cast<const f16x8*>(bh + ob), b_l = *reinterpret_cast<const f16x8*>(bl + ob);
    if (SWAP) {
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_h, b_l, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_l, b_h, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_h, b_h, acc, 0, 0, 0);
    } else {
      acc = mfma3(a_h, a_l, b_h, b_l, acc);
    }
  }
  return acc;
}

// out[i] += (rows ra .. of the [ET_R][ET_TLD] tile) x (rows rb + 16 i .. of the transposed planes [.][ET_TLD])^T: the
// contraction runs over the tile's 32 columns
template <int NB>
__device__ __forceinline__ void mma_over_rows(const __half* th, const __half* tl, int ra, const __half* xh, const __half* xl,
                                              int rb, int lane, f32x4 out[NB]) {
  const int frow = lane & 15, fk = (lane >> 4) * 8;
  const f16x8 ah = *reinterpret_cast<const f16x8*>(th + (ra + frow) * ET_TLD + fk);
  const f16x8 al = *reinterpret_cast<const f16x8*>(tl + (ra + frow) * ET_TLD + fk);
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int ob = (rb + 16 * i + frow) * ET_TLD + fk;
    out[i] = mfma3(ah, al, *reinterpret_cast<const f16x8*>(xh + ob), *reinterpret_cast<const f16x8*>(xl + ob), out[i]);
  }
}

// the wave's 16 x 16 block in the accumulator layout (rows r0 + e, column c) into the P / dS tile
__device__ __forceinline__ void store_block(const float v[4], int r0, int c, __half* th, __half* tl) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    __half h, l;
    split_f16(v[e], h, l);
    th[(r0 + e) * ET_TLD + c] = h;
    tl[(r0 + e) * ET_TLD + c] = l;
  }
}

struct AttnBwd {
  const float* qkv;     // [B S, 3 dm]
  const float* dO;      // [B S, dm]
  const float* lse;     // [h, B S], exp2 domain
  float* D;             // [h, B S]: sum_j P o dP of the scaled dO, written by the dq kernel for the dkv kernel
  const float* am_do;   // 64 first-stage maxima of |dO|
  const float* y;       // [B S] labels or nullptr: key j is masked when y == pad
  float pad;
  int S, dm, dk;
  float scale;          // 1 / sqrt(d_k)
  float* dqkv;          // [B S, 3 dm]
};

template <int DKP> struct BwdLds {
  static constexpr int RM = ET_R * (DKP + 8);                       // halves of a row-major plane
  static constexpr int X = RM > DKP * ET_TLD ? RM : DKP * ET_TLD;   // the staging plane holds either form
};

template <int DKP>
__global__ void __launch_bounds__(ET_THREADS) enc_attn_dkv_kernel(AttnBwd a) {
  constexpr int NB = DKP / 32;           // 16-column blocks of a wave's half of d_k
  __shared__ __attribute__((aligned(16))) __half s_k[2][BwdLds<DKP>::RM];
  __shared__ __attribute__((aligned(16))) __half s_v[2][BwdLds<DKP>::RM];
  __shared__ __attribute__((aligned(16))) __half s_x[2][BwdLds<DKP>::X];
  __shared__ __attribute__((aligned(16))) __half s_t[2][ET_R * ET_TLD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave >> 1, wc = wave & 1;
  const int crow = 4 * (lane >> 4), ccol = lane & 15;
  const int k0 = blockIdx.x * ET_R, hh = blockIdx.z, S = a.S, dk = a.dk, ld = 3 * a.dm;
  const size_t row0 = (size_t)blockIdx.y * S, hrow = (size_t)hh * gridDim.y * S + row0;
  const float* qb = a.qkv + row0 * ld + hh * dk;
  const float* dob = a.dO + row0 * a.dm + hh * dk;
  const float sdo = split_scale(wave_max(a.am_do[lane])) * 0.015625f;     // max|dO| -> 2^6: dS stays inside fp16's range
  const float qscale = a.scale * LOG2E;

  load_tile<DKP, ET_R, false>(qb + a.dm, ld, k0, S, dk, 1.f, s_k[0], s_k[1]);
  load_tile<DKP, ET_R, false>(qb + 2 * a.dm, ld, k0, S, dk, 1.f, s_v[0], s_v[1]);
  bool kv[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int key = k0 + wr * 16 + crow + e;
    kv[e] = key < S && key_valid(a.y, a.pad, row0 + key);
  }
  f32x4 dK[NB], dV[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) dK[i] = dV[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int q0 = 0; q0 < S; q0 += ET_R) {       // the slate's query tiles, in order
    __syncthreads();                           // the previous tile's readers of s_x and s_t are done
    load_tile<DKP, ET_R, false>(qb, ld, q0, S, dk, qscale, s_x[0], s_x[1]);
    __syncthreads();
    const int q = q0 + wc * 16 + ccol;
    const float lse = q < S ? a.lse[hrow + q] : 0.f, Dq = q < S ? a.D[hrow + q] : 0.f;
    const f32x4 st = mma_over_d<DKP, true>(s_k[0], s_k[1], wr * 16, s_x[0], s_x[1], wc * 16, lane);
    float p[4], ds[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = q < S && kv[e] ? __builtin_amdgcn_exp2f(st[e] - lse) : 0.f;
    store_block(p, wr * 16 + crow, wc * 16 + ccol, s_t[0], s_t[1]);
    __syncthreads();                           // Q's readers are done
    load_tile<DKP, ET_R, false>(dob, a.dm, q0, S, dk, sdo, s_x[0], s_x[1]);
    __syncthreads();
    const f32x4 dp = mma_over_d<DKP, true>(s_v[0], s_v[1], wr * 16, s_x[0], s_x[1], wc * 16, lane);
#pragma unroll
    for (int e = 0; e < 4; ++e) ds[e] = p[e] * (dp[e] - Dq);
    __syncthreads();                           // dO's readers are done
    load_tile<DKP, ET_R, true>(dob, a.dm, q0, S, dk, sdo, s_x[0], s_x[1]);
    __syncthreads();                           // P^T and dO^T are in LDS
    mma_over_rows<NB>(s_t[0], s_t[1], wr * 16, s_x[0], s_x[1], wc * (DKP / 2), lane, dV);
    __syncthreads();                           // their readers are done
    store_block(ds, wr * 16 + crow, wc * 16 + ccol, s_t[0], s_t[1]);
    load_tile<DKP, ET_R, true>(qb, ld, q0, S, dk, 1.f, s_x[0], s_x[1]);
    __syncthreads();
    mma_over_rows<NB>(s_t[0], s_t[1], wr * 16, s_x[0], s_x[1], wc * (DKP / 2), lane, dK);
  }

  const float cv = 1.f / sdo, ck = a.scale * cv;     // 1 / sdo is a power of two: exact
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int key = k0 + wr * 16 + crow + e;
    if (key >= S) continue;
    float* row = a.dqkv + (row0 + key) * ld + hh * dk;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int d = wc * (DKP / 2) + 16 * i + ccol;
      if (d < dk) { row[a.dm + d] = dK[i][e] * ck; row[2 * a.dm + d] = dV[i][e] * cv; }
    }
  }
}

template <int DKP>
__global__ void __launch_bounds__(ET_THREADS) enc_attn_dq_kernel(AttnBwd a) {
  constexpr int NB = DKP / 32;
  __shared__ __attribute__((aligned(16))) __half s_q[2][BwdLds<DKP>::RM];
  __shared__ __attribute__((aligned(16))) __half s_do[2][BwdLds<DKP>::RM];
  __shared__ __attribute__((aligned(16))) __half s_x[2][BwdLds<DKP>::X];
  __shared__ __attribute__((aligned(16))) __half s_t[2][ET_R * ET_TLD];
  __shared__ float s_d[2][ET_R];           // a row's sum over each half of a key tile's columns
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave >> 1, wc = wave & 1;
  const int crow = 4 * (lane >> 4), ccol = lane & 15;
  const int q0 = blockIdx.x * ET_R, hh = blockIdx.z, S = a.S, dk = a.dk, ld = 3 * a.dm;
  const size_t row0 = (size_t)blockIdx.y * S, hrow = (size_t)hh * gridDim.y * S + row0;
  const float* qb = a.qkv + row0 * ld + hh * dk;
  const float sdo = split_scale(wave_max(a.am_do[lane])) * 0.015625f;

  load_tile<DKP, ET_R, false>(qb, ld, q0, S, dk, a.scale * LOG2E, s_q[0], s_q[1]);
  load_tile<DKP, ET_R, false>(a.dO + row0 * a.dm + hh * dk, a.dm, q0, S, dk, sdo, s_do[0], s_do[1]);
  float lse[4], Dq[4];
  bool qv[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int q = q0 + wr * 16 + crow + e;
    qv[e] = q < S;
    lse[e] = qv[e] ? a.lse[hrow + q] : 0.f;
    Dq[e] = 0.f;
  }
  f32x4 dQ[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) dQ[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int pass = 0; pass < 2; ++pass) {       // 0: D, 1: dQ
  float part[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < S; k0 += ET_R) {       // the slate's key tiles, in order
    __syncthreads();                           // the previous tile's readers of s_x and s_t are done
    load_tile<DKP, ET_R, false>(qb + a.dm, ld, k0, S, dk, 1.f, s_x[0], s_x[1]);
    __syncthreads();
    const int key = k0 + wc * 16 + ccol;
    const bool kv = key < S && key_valid(a.y, a.pad, row0 + key);
    const f32x4 st = mma_over_d<DKP, false>(s_q[0], s_q[1], wr * 16, s_x[0], s_x[1], wc * 16, lane);
    float p[4], ds[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = kv && qv[e] ? __builtin_amdgcn_exp2f(st[e] - lse[e]) : 0.f;
    __syncthreads();                           // K's readers are done
    load_tile<DKP, ET_R, false>(qb + 2 * a.dm, ld, k0, S, dk, 1.f, s_x[0], s_x[1]);
    __syncthreads();
    const f32x4 dp = mma_over_d<DKP, false>(s_do[0], s_do[1], wr * 16, s_x[0], s_x[1], wc * 16, lane);
    if (pass == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) part[e] += p[e] * dp[e];
      continue;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) ds[e] = p[e] * (dp[e] - Dq[e]);
    store_block(ds, wr * 16 + crow, wc * 16 + ccol, s_t[0], s_t[1]);
    __syncthreads();                           // V's readers are done
    load_tile<DKP, ET_R, true>(qb + a.dm, ld, k0, S, dk, 1.f, s_x[0], s_x[1]);
    __syncthreads();                           // dS and K^T are in LDS
    mma_over_rows<NB>(s_t[0], s_t[1], wr * 16, s_x[0], s_x[1], wc * (DKP / 2), lane, dQ);
  }
  if (pass == 0) {                             // the 16 column lanes of a row, then the two column halves, in a fixed order
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int w = 8; w > 0; w >>= 1) part[e] += __shfl_xor(part[e], w, 64);
      if (ccol == 0) s_d[wc][wr * 16 + crow + e] = part[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      Dq[e] = s_d[0][wr * 16 + crow + e] + s_d[1][wr * 16 + crow + e];
      if (wc == 0 && ccol == 0 && qv[e]) a.D[hrow + q0 + wr * 16 + crow + e] = Dq[e];
    }
  }
  }

  const float cq = a.scale / sdo;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int q = q0 + wr * 16 + crow + e;
    if (q >= S) continue;
    float* row = a.dqkv + (row0 + q) * ld + hh * dk;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int d = wc * (DKP / 2) + 16 * i + ccol;
      if (d < dk) row[d] = dQ[i][e] * cq;
    }
  }
}

// slate_attn_kernel on slate blockIdx.y = rows [b S, b S + S), with the key mask and the log-sum-exp output.
// DKP: d_k rounded up to 32; BK: keys per tile
template <int DKP, int BK>
__global__ void __launch_bounds__(ET_THREADS) enc_attn_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ y,
                                                                  float pad, int S, int dm, int dk, float qscale,
                                                                  float* __restrict__ out, float* __restrict__ lse) {
  constexpr int KLD = DKP + 8, VLD = BK + 8;
  __shared__ __attribute__((aligned(16))) __half s_k[2][BK * KLD];       // hi, lo
  __shared__ __attribute__((aligned(16))) __half s_v[2][DKP * VLD];      // V^T hi, lo: [d][key]
  __shared__ __attribute__((aligned(16))) __half s_p[4][2][16 * VLD];    // per wave: P hi, lo [query][key]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hh = blockIdx.z;
  const size_t row0 = (size_t)blockIdx.y * S;
  const int ld = 3 * dm;
  const float* qb = qkv + row0 * ld + hh * dk;
  const int frow = lane & 15, fk = (lane >> 4) * 8;
  const int crow = 4 * (lane >> 4), ccol = lane & 15;

  for (int q0 = blockIdx.x * ET_BQ; q0 < S; q0 += gridDim.x * ET_BQ) {
    f16x8 qh[DKP / 32], ql[DKP / 32];
    {
      const int qr = q0 + wave * 16 + frow;
#pragma unroll
      for (int ks = 0; ks < DKP / 32; ++ks) {
        float v[8];
        load4<float, true>(qb + (size_t)qr * ld, ks * 32 + fk, qr < S ? dk : 0, v);
        load4<float, true>(qb + (size_t)qr * ld, ks * 32 + fk + 4, qr < S ? dk : 0, v + 4);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          __half h, l;
          split_f16(v[i] * qscale, h, l);
          qh[ks][i] = __builtin_bit_cast(_Float16, h);
          ql[ks][i] = __builtin_bit_cast(_Float16, l);
        }
      }
    }
    f32x4 o[DKP / 16];
#pragma unroll
    for (int i = 0; i < DKP / 16; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { m[e] = -INFINITY; l[e] = 0.f; }

    for (int k0 = 0; k0 < S; k0 += BK) {
      __syncthreads();                  // the previous tile's readers are done
      load_tile<DKP, BK, false>(qb + dm, ld, k0, S, dk, 1.f, s_k[0], s_k[1]);
      load_tile<DKP, BK, true>(qb + 2 * dm, ld, k0, S, dk, 1.f, s_v[0], s_v[1]);
      __syncthreads();

      bool kv[BK / 16];                 // the lane's key of every 16-key piece is inside the slate and not padded
#pragma unroll
      for (int j = 0; j < BK / 16; ++j) {
        const int key = k0 + j * 16 + ccol;
        kv[j] = key < S && key_valid(y, pad, row0 + key);
      }
      f32x4 sacc[BK / 16];
#pragma unroll
      for (int j = 0; j < BK / 16; ++j) {
        sacc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < DKP / 32; ++ks) {
          const int off = (j * 16 + frow) * KLD + ks * 32 + fk;
          sacc[j] = mfma3(qh[ks], ql[ks], *reinterpret_cast<const f16x8*>(&s_k[0][off]),
                          *reinterpret_cast<const f16x8*>(&s_k[1][off]), sacc[j]);
        }
      }
      // online softmax of the wave's 16 rows: lane (crow + e, ccol) of every 16-key piece
      float alpha[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < BK / 16; ++j) {
          if (!kv[j]) sacc[j][e] = -INFINITY;
          mx = fmaxf(mx, sacc[j][e]);
        }
#pragma unroll
        for (int w = 8; w > 0; w >>= 1) mx = fmaxf(mx, __shfl_xor(mx, w, 64));
        const float mn = fmaxf(m[e], mx);
        const float mu = mn == -INFINITY ? 0.f : mn;      // every key so far is masked: p = 0 and alpha = 0, not NaN
        alpha[e] = __builtin_amdgcn_exp2f(m[e] - mu);
        m[e] = mn;
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < BK / 16; ++j) {
          const float p = __builtin_amdgcn_exp2f(sacc[j][e] - mu);
          sum += p;
          __half ph, pl;
          split_f16(p, ph, pl);
          s_p[wave][0][(crow + e) * VLD + j * 16 + ccol] = ph;
          s_p[wave][1][(crow + e) * VLD + j * 16 + ccol] = pl;
        }
#pragma unroll
        for (int w = 8; w > 0; w >>= 1) sum += __shfl_xor(sum, w, 64);
        l[e] = l[e] * alpha[e] + sum;
      }
#pragma unroll
      for (int i = 0; i < DKP / 16; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) o[i][e] *= alpha[e];
      __syncthreads();                  // P is in LDS
#pragma unroll
      for (int kk = 0; kk < BK / 32; ++kk) {
        const f16x8 ph = *reinterpret_cast<const f16x8*>(&s_p[wave][0][frow * VLD + kk * 32 + fk]);
        const f16x8 pl = *reinterpret_cast<const f16x8*>(&s_p[wave][1][frow * VLD + kk * 32 + fk]);
#pragma unroll
        for (int i = 0; i < DKP / 16; ++i) {
          const int off = (i * 16 + frow) * VLD + kk * 32 + fk;
          o[i] = mfma3(ph, pl, *reinterpret_cast<const f16x8*>(&s_v[0][off]), *reinterpret_cast<const f16x8*>(&s_v[1][off]), o[i]);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int qr = q0 + wave * 16 + crow + e;
      if (qr >= S) continue;
      const float inv = l[e] > 0.f ? 1.f / l[e] : 0.f;      // no valid key: output 0
      float* orow = out + (row0 + qr) * dm + hh * dk;
#pragma unroll
      for (int i = 0; i < DKP / 16; ++i)
        if (i * 16 + ccol < dk) orow[i * 16 + ccol] = o[i][e] * inv;
      if (ccol == 0) lse[(size_t)hh * gridDim.y * S + row0 + qr] = l[e] > 0.f ? m[e] + log2f(l[e]) : 0.f;
    }
  }
}

}  // namespace

int launch_enc_rows(const float* z, const float* branch, float* z_out, int M, int K, float* stats, hipStream_t s) {
  enc_rows_kernel<<<(M + 3) / 4, ET_THREADS, 0, s>>>(z, branch, z_out, M, K, stats);
  LTR_LAUNCH_CHECK();
  return LTR_OK;
}

int launch_enc_ln_bwd(const float* x, const float* stats, const float* a2, const float* dy, const float* resid, float* dx,
                      int M, int K, hipStream_t s) {
  enc_ln_bwd_kernel<<<(M + 3) / 4, ET_THREADS, 0, s>>>(x, stats, a2, dy, resid, dx, M, K);
  LTR_LAUNCH_CHECK();
  return LTR_OK;
}

int launch_enc_attn_fwd(const float* qkv, const float* y, float pad, int B, int S, int dm, int h, float* out, float* lse,
                        hipStream_t s) {
  const int dk = dm / h;
  const float qscale = LOG2E / sqrtf((float)dk);
  const dim3 grid((S + ET_BQ - 1) / ET_BQ, B, h);
  if (dk <= 32) enc_attn_fwd_kernel<32, 64><<<grid, ET_THREADS, 0, s>>>(qkv, y, pad, S, dm, dk, qscale, out, lse);
  else if (dk <= 64) enc_attn_fwd_kernel<64, 64><<<grid, ET_THREADS, 0, s>>>(qkv, y, pad, S, dm, dk, qscale, out, lse);
  else if (dk <= 96) enc_attn_fwd_kernel<96, 32><<<grid, ET_THREADS, 0, s>>>(qkv, y, pad, S, dm, dk, qscale, out, lse);
  else enc_attn_fwd_kernel<128, 32><<<grid, ET_THREADS, 0, s>>>(qkv, y, pad, S, dm, dk, qscale, out, lse);
  LTR_LAUNCH_CHECK();
  return LTR_OK;
}

int launch_enc_attn_bwd(const float* qkv, const float* dO, const float* lse, const float* am_do, const float* y, float pad,
                        int B, int S, int dm, int h, float* D, float* dqkv, hipStream_t s) {
  const int dk = dm / h;
  const AttnBwd a{qkv, dO, lse, D, am_do, y, pad, S, dm, dk, 1.f / sqrtf((float)dk), dqkv};
  const dim3 grid((S + ET_R - 1) / ET_R, B, h);
  if (dk <= 32) { enc_attn_dq_kernel<32><<<grid, ET_THREADS, 0, s>>>(a); enc_attn_dkv_kernel<32><<<grid, ET_THREADS, 0, s>>>(a); }
  else if (dk <= 64) { enc_attn_dq_kernel<64><<<grid, ET_THREADS, 0, s>>>(a); enc_attn_dkv_kernel<64><<<grid, ET_THREADS, 0, s>>>(a); }
  else if (dk <= 96) { enc_attn_dq_kernel<96><<<grid, ET_THREADS, 0, s>>>(a); enc_attn_dkv_kernel<96><<<grid, ET_THREADS, 0, s>>>(a); }
  else { enc_attn_dq_kernel<128><<<grid, ET_THREADS, 0, s>>>(a); enc_attn_dkv_kernel<128><<<grid, ET_THREADS, 0, s>>>(a); }
  LTR_LAUNCH_CHECK();
  return LTR_OK;
}

}  // namespace ltr
