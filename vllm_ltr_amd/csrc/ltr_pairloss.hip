// LambdaLoss on gfx950: allRank's pairwise loss family (train/allrank/models/losses/lambdaLoss.py:23-130 - RankNet, LambdaRank,
// NDCGLoss1 / 2 / 2++ and the two label-difference weighings) and its gradient w.r.t. the predictions, without the five or six
// [B, S, S] tensors the reference builds.  The definition is the one of include/ltr_hip.h (ltr_lambdaloss); in short, per slate:
// the valid items (y_true != pad) are ranked by descending score (equal scores: lower index first), pair (i, j) is selected when
// both ranks are below the cut and label_i > label_j (NDCGLoss1: every pair, the diagonal too), and the loss is
// -sum log(max(max(sigmoid(sigma (s_i - s_j)), eps)^w_ij, eps)) with weights w_ij that are constants of the ranks, labels and gains.
//
// Three launches on the caller's stream, nothing of size [S, S] in memory:
//
//   prepare  one workgroup per slate.  Scores and labels sit in LDS as order-preserving 32-bit keys (0 = padded item); every
//            thread holds up to four items and ranks them BY COUNTING on both keys at once: one broadcast ds_read_b64 of
//            (score key, label key) of item j feeds eight compares.  "Key j is ahead of key i" is kj > ki for j > i and
//            kj >= ki = kj > ki - 1 for j < i; j runs in chunks of 64, and a wave's items of one register slot lie in ONE
//            chunk, so outside that chunk the threshold (ki or ki - 1) is chosen once per chunk and a compare costs v_cmp +
//            v_addc.  The label ranks give the ideal DCG (block sum in a fixed order), the score ranks the per-slate arrays IN
//            RANK ORDER - score, label, gain, 1 / D, original index - and lim = min(cut, valid items).  Items outside the
//            cut and padded items get their zero gradient here.
//   pair     grid (ceil(cut / 64), B): a workgroup owns 64 consecutive ranks.  Lane l of each of its four waves holds row
//            rank r0 + l in registers; the ranked items [0, lim) stream through LDS in tiles of 256 columns as float4 (score,
//            label, gain, 1 / D), wave w takes columns w, w + 4, ... of a tile, and all 64 lanes read the SAME column: a
//            conflict-free broadcast ds_read_b128.  (The NDCGLoss2 table |1/D[d-1] - 1/D[d]| is in LDS too, indexed by
//            |rank_i - rank_j| - consecutive addresses across a wave.)  For every (row, column) BOTH orientations are
//            evaluated, so the row's owner accumulates the row's complete gradient and nobody else touches it; orientation
//            (row, column) alone counts towards the loss and the pair count.  The two orientations share one exp, one log2 and
//            one reciprocal: with z = sigma x and e = exp(-|z|), log2 sigmoid(z) = -(max(-z, 0) log2(e) + log2(1 + e)) - a
//            stable softplus, so a large negative x reaches the eps clamp as a finite logarithm instead of log(0) - and
//            1 - sigmoid(z) = (z >= 0 ? e : 1) / (1 + e).  Both clamps act in the log2 domain.  Four waves -> LDS -> wave 0
//            adds them in wave order, stores the gradient once at the original index (plain store) and reduces loss and count
//            over the 64 rows with a fixed shuffle tree into ONE partial record per workgroup.
//   finish   adds the partials (f64, fixed order), writes the loss and, under `mean`, scales the gradients by 1 / pairs.
//
// No atomics, no memset, no host sync, every dependency is a launch boundary: two calls give identical bits and the call can
// be captured into a graph.  Matrix instructions have no use here (elementwise pair math).
#include "ltr_internal.h"

#include <algorithm>

namespace ltr {
namespace {

constexpr int LL_MAX_S = 4096;          // listMLE's limit
constexpr int LL_MAX_B = 65535;         // grid.y
constexpr int LL_ROWS = 64;             // ranks per pair workgroup
constexpr int LL_THREADS = 256;
constexpr int LL_WAVES = LL_THREADS / WAVE;
constexpr int LL_COLS = 256;            // columns per LDS tile
constexpr int LL_PREP_MAX = 1024;       // threads of the prepare workgroup
constexpr float LL_LOG2E = 1.4426950408889634f;
constexpr float LL_LN2 = 0.6931471805599453f;
constexpr float LL_XCLAMP = 1e8f;

enum { LL_NONE = 0, LL_RANKNET = 1, LL_NDCG1 = 2, LL_NDCG2 = 3, LL_LAMBDARANK = 4, LL_NDCG2PP = 5, LL_GTDIFF = 6, LL_GTDIFF_POW = 7, LL_SCHEMES = 8 };

struct LlPartial {
  double loss;          // sum of the selected terms, log2 domain
  long long pairs;
};

// per-call workspace: five [B, S] arrays in rank order, lim [B], one partial per pair workgroup
struct LlWs {
  float *score, *label, *gain, *inv_d;
  int32_t *index, *lim;
  LlPartial* part;
  size_t bytes;
};
LlWs ll_carve(int B, int S, void* base) {
  char* p = (char*)base;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t q = o; o += align256(bytes); return base ? p + q : nullptr; };
  const size_t n = (size_t)B * S * 4;
  LlWs w;
  w.score = (float*)take(n); w.label = (float*)take(n); w.gain = (float*)take(n); w.inv_d = (float*)take(n);
  w.index = (int32_t*)take(n);
  w.lim = (int32_t*)take((size_t)B * 4);
  w.part = (LlPartial*)take((size_t)B * ((S + LL_ROWS - 1) / LL_ROWS) * sizeof(LlPartial));
  w.bytes = o;
  return w;
}

// f32 -> u32 that orders like the float (-0 == +0), squeezed into [1, 0xfffffffe]: 0 is the padded item, and ki - 1 / the
// compare against 0xffffffff never wrap.  NaNs land at the ends; the index tie-break keeps every rank unique whatever the bits.
__device__ __forceinline__ uint32_t ll_key(float v) {
  uint32_t u = __float_as_uint(v == 0.f ? 0.f : v);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return min(max(u, 1u), 0xfffffffeu);
}

// D[r] = log2(2 + r) in f32, as the reference's torch.log2(1. + pos_idxs.float()) (lambdaLoss.py:68-69)
__device__ __forceinline__ float ll_discount(int r) { return log2f((float)(r + 2)); }

// sum over the workgroup in a fixed order: shuffle tree inside a wave, then the waves in index order.  Every thread gets it.
template <typename T> __device__ __forceinline__ T ll_block_sum(T v, T* red, int n_waves) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();                                 // red may still be read from a previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T t = red[0];
  for (int w = 1; w < n_waves; ++w) t += red[w];
  return t;
}

// ---- prepare ------------------------------------------------------------------------------------------------------------
// one chunk of 64 keys against the NI items of a thread.  MIXED: the chunk holds an item of this wave, j < i is per lane
template <int NI, bool MIXED>
__device__ __forceinline__ void ll_count_chunk(const uint2* __restrict__ key, int j0, int lane, const int (&qm)[NI], int q,
                                               const uint32_t (&ks)[NI], const uint32_t (&kl)[NI], uint32_t (&rs)[NI],
                                               uint32_t (&rl)[NI]) {
  uint32_t ts[NI], tl[NI];
#pragma unroll
  for (int m = 0; m < NI; ++m) {                   // j < i for the whole chunk: "ahead" is kj >= ki
    const uint32_t before = q < qm[m] ? 1u : 0u;
    ts[m] = ks[m] - before; tl[m] = kl[m] - before;
  }
#pragma unroll 8
  for (int jj = 0; jj < 64; ++jj) {                // (a full unroll of 64 keeps every key live: spills at one item per thread)
    const uint2 kj = key[j0 + jj];                 // same address in every lane: broadcast
#pragma unroll
    for (int m = 0; m < NI; ++m) {
      uint32_t a = ts[m], b = tl[m];
      if (MIXED) {
        const uint32_t own = (q == qm[m] && jj < lane) ? 1u : 0u;
        a -= own; b -= own;
      }
      rs[m] += kj.x > a ? 1u : 0u;
      rl[m] += kj.y > b ? 1u : 0u;
    }
  }
}

// NI items per thread, i = t + m * blockDim.x; blockDim.x is a multiple of 64 with NI * blockDim.x >= S
template <int NI>
__global__ __launch_bounds__(LL_PREP_MAX) void ll_prepare_kernel(const float* __restrict__ y_pred, const float* __restrict__ y_true,
                                                                 int S, int kk, float eps, float pad, LlWs ws,
                                                                 float* __restrict__ grad_out) {
  __shared__ uint2 key[LL_MAX_S];                  // (score key, label key); 0 = padded or beyond S
  __shared__ float redf[LL_PREP_MAX / WAVE];
  __shared__ int redi[LL_PREP_MAX / WAVE];
  const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, n_waves = nt >> 6;
  const size_t base = (size_t)blockIdx.x * S;
  float s[NI], l[NI];
  uint32_t ks[NI], kl[NI], rs[NI], rl[NI];
  int qm[NI];
  int valid = 0;
#pragma unroll
  for (int m = 0; m < NI; ++m) {
    const int i = t + m * nt;
    s[m] = 0.f; l[m] = pad; ks[m] = kl[m] = 0; rs[m] = rl[m] = 0;
    qm[m] = i >> 6;
    if (i < S) { s[m] = y_pred[base + i]; l[m] = y_true[base + i]; }
    if (i < S && l[m] != pad) { ks[m] = ll_key(s[m]); kl[m] = ll_key(l[m]); ++valid; }
    if (i < LL_MAX_S) key[i] = make_uint2(ks[m], kl[m]);
  }
  const int n_valid = ll_block_sum<int>(valid, redi, n_waves);     // (its barriers publish key[])
  const int lim = min(kk, n_valid);

  const int n_chunks = (S + 63) >> 6;              // key[] is written up to NI * nt >= 64 * n_chunks
  for (int q = 0; q < n_chunks; ++q) {
    bool mixed = false;
#pragma unroll
    for (int m = 0; m < NI; ++m) mixed |= q == qm[m];              // wave-uniform: qm = wave + m * n_waves
    if (mixed) ll_count_chunk<NI, true>(key, q << 6, lane, qm, q, ks, kl, rs, rl);
    else       ll_count_chunk<NI, false>(key, q << 6, lane, qm, q, ks, kl, rs, rl);
  }

  // ideal DCG over the kk largest labels (lambdaLoss.py:70): label ranks are unique, so every position is summed once
  float dcg = 0.f;
#pragma unroll
  for (int m = 0; m < NI; ++m)
    if (ks[m] != 0 && (int)rl[m] < kk) dcg += (exp2f(fmaxf(l[m], 0.f)) - 1.f) / ll_discount((int)rl[m]);
  const float max_dcg = fmaxf(ll_block_sum<float>(dcg, redf, n_waves), eps);

#pragma unroll
  for (int m = 0; m < NI; ++m) {
    const int i = t + m * nt;
    if (i >= S) continue;
    const int r = (int)rs[m];
    const bool ranked = ks[m] != 0;                // valid items take the ranks 0 .. n_valid - 1, each exactly once
    if (ranked) {
      ws.score[base + r] = s[m];
      ws.label[base + r] = l[m];
      ws.gain[base + r] = (exp2f(fmaxf(l[m], 0.f)) - 1.f) / max_dcg;
      ws.inv_d[base + r] = 1.f / ll_discount(r);
      ws.index[base + r] = i;
    }
    if (grad_out != nullptr && !(ranked && r < lim)) grad_out[base + i] = 0.f;   // no pair kernel row owns this item
  }
  if (t == 0) ws.lim[blockIdx.x] = lim;
}

// ---- pair ---------------------------------------------------------------------------------------------------------------
// One orientation: z = sigma * clamp(x), e = exp(-|z|), l1p = log2(1 + e), r1 = 1 / (1 + e).
//   lq = log2 max(max(sigmoid(z), eps)^w, eps);  g = w (1 - sigmoid(z)), 0 where a clamp is active
__device__ __forceinline__ void ll_orient(float z, float w, float e, float l1p, float r1, float l2eps, bool x_clamped, float& lq,
                                          float& g) {
  const float lp = -(fmaxf(-z, 0.f) * LL_LOG2E + l1p);
  bool cl = x_clamped || lp < l2eps;
  lq = w * fmaxf(lp, l2eps);
  cl = cl || lq < l2eps;
  lq = fmaxf(lq, l2eps);
  g = cl ? 0.f : w * ((z >= 0.f ? e : 1.f) * r1);
}

struct LlArgs {
  int S, kk;
  float sigma, mu, l2eps;
  LlWs ws;
  float* grad_out;      // nullable
  float gscale;         // sigma / (ln 2 | 1)
};

template <int SCHEME>
__global__ __launch_bounds__(LL_THREADS) void ll_pair_kernel(LlArgs a) {
  constexpr bool NEED_DELTA = SCHEME == LL_NDCG2 || SCHEME == LL_NDCG2PP;
  __shared__ float4 col[LL_COLS];
  __shared__ float delta[NEED_DELTA ? LL_MAX_S : 1];
  __shared__ float red_g[LL_WAVES][LL_ROWS], red_l[LL_WAVES][LL_ROWS];
  __shared__ uint32_t red_n[LL_WAVES][LL_ROWS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.y, r0 = blockIdx.x * LL_ROWS;
  const size_t base = (size_t)b * a.S;
  const int lim = a.ws.lim[b];
  LlPartial* part = a.ws.part + (size_t)b * gridDim.x + blockIdx.x;
  if (r0 >= lim) {                                 // (uniform) the cut or the padding left this tile without rows
    if (t == 0) *part = LlPartial{0.0, 0};
    return;
  }
  const int ri = r0 + lane;
  const bool live = ri < lim;
  float si = 0.f, li = 0.f, gi = 0.f, di = 0.f;
  if (live) { si = a.ws.score[base + ri]; li = a.ws.label[base + ri]; gi = a.ws.gain[base + ri]; di = a.ws.inv_d[base + ri]; }
  const float lic = fmaxf(li, 0.f);                // the weights see labels clamped at 0 (lambdaLoss.py:64)
  if (NEED_DELTA) {                                // |1/D[d-1] - 1/D[d]| from the f32 discounts, differenced in f64
    for (int d = t; d < lim; d += LL_THREADS)
      delta[d] = d == 0 ? 0.f : (float)fabs(1.0 / (double)ll_discount(d - 1) - 1.0 / (double)ll_discount(d));
  }

  float acc_g = 0.f, acc_l = 0.f;
  uint32_t acc_n = 0;
  float4 next = make_float4(0.f, 0.f, 0.f, 0.f);
  if (t < lim) next = make_float4(a.ws.score[base + t], a.ws.label[base + t], a.ws.gain[base + t], a.ws.inv_d[base + t]);
  for (int c0 = 0; c0 < lim; c0 += LL_COLS) {
    __syncthreads();                               // the previous tile has been read (first round: delta[] is complete after the next one)
    col[t] = next;
    __syncthreads();
    const int cn = c0 + LL_COLS + t;               // next tile's loads fly while this one is computed
    if (cn < lim) next = make_float4(a.ws.score[base + cn], a.ws.label[base + cn], a.ws.gain[base + cn], a.ws.inv_d[base + cn]);
    const int jcount = min(LL_COLS, lim - c0);
    for (int j = wave; j < jcount; j += LL_WAVES) {
      const float4 c = col[j];                     // same address in every lane: broadcast
      const float sj = c.x, lj = own_reg(c.y), gj = c.z, dj = own_reg(c.w);   // (own_reg: isa_lint.py, high halves of 64-bit pairs)
      const int rj = c0 + j;
      const float x = si - sj;
      const bool x_clamped = fabsf(x) > LL_XCLAMP;
      const float z = a.sigma * fminf(fmaxf(x, -LL_XCLAMP), LL_XCLAMP);
      const float e = __expf(-fabsf(z));
      // log2(1 + e): below 2^-8 the series, whose relative error stays at f32's (1 + e rounds e's low bits away)
      const float l1p = e < 0.00390625f ? e * LL_LOG2E * (1.f - e * (0.5f - e * (1.f / 3.f))) : __log2f(1.f + e);
      const float r1 = 1.f / (1.f + e);
      if (SCHEME == LL_NDCG1) {                    // every pair, both orientations with their own weight; the diagonal gives loss only
        float lq, g_ij, lq2, g_ji;
        ll_orient(z, gi * di, e, l1p, r1, a.l2eps, x_clamped, lq, g_ij);
        ll_orient(-z, gj * dj, e, l1p, r1, a.l2eps, x_clamped, lq2, g_ji);
        acc_l += live ? lq : 0.f;
        acc_n += live ? 1u : 0u;
        acc_g += (live && rj != ri) ? g_ji - g_ij : 0.f;
      } else {                                     // at most one orientation is selected, and the weight is symmetric
        const bool fwd = live && li > lj, bwd = live && lj > li;
        float w = 1.f;
        const float dg = fabsf(gi - gj);
        const int d = abs(ri - rj);
        if (SCHEME == LL_NDCG2) w = delta[NEED_DELTA ? d : 0] * dg;
        if (SCHEME == LL_LAMBDARANK) w = fabsf(di - dj) * dg;
        if (SCHEME == LL_NDCG2PP) w = a.mu * (delta[NEED_DELTA ? d : 0] * dg) + fabsf(di - dj) * dg;
        if (SCHEME == LL_GTDIFF) w = fabsf(lic - fmaxf(lj, 0.f));
        if (SCHEME == LL_GTDIFF_POW) { const float ljc = fmaxf(lj, 0.f); w = fabsf(lic * lic - ljc * ljc); }
        float lq, g;
        ll_orient(fwd ? z : -z, w, e, l1p, r1, a.l2eps, x_clamped, lq, g);
        acc_l += fwd ? lq : 0.f;
        acc_n += fwd ? 1u : 0u;
        acc_g += fwd ? -g : (bwd ? g : 0.f);
      }
    }
  }

  red_g[wave][lane] = acc_g; red_l[wave][lane] = acc_l; red_n[wave][lane] = acc_n;
  __syncthreads();
  if (wave != 0) return;
  float g = red_g[0][lane], l = red_l[0][lane];
  uint32_t n = red_n[0][lane];
#pragma unroll
  for (int w = 1; w < LL_WAVES; ++w) { g += red_g[w][lane]; l += red_l[w][lane]; n += red_n[w][lane]; }
  if (live && a.grad_out != nullptr) {
    const int oi = a.ws.index[base + ri];          // a permutation of the valid items by construction; the bound costs nothing
    if ((unsigned)oi < (unsigned)a.S) a.grad_out[base + oi] = a.gscale * g;
  }
  double ld = (double)l;
  long long nd = (long long)n;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { ld += __shfl_xor(ld, o, 64); nd += __shfl_xor(nd, o, 64); }
  if (lane == 0) *part = LlPartial{ld, nd};
}

// ---- finish -------------------------------------------------------------------------------------------------------------
// loss = -sum of the partials (x ln 2 for the natural logarithm), / pairs under `mean`; every workgroup adds the partials in
// the same order and scales its share of the gradients, workgroup 0 writes the loss.  No selected pair: loss 0, gradients are
// zero already.
__global__ __launch_bounds__(LL_THREADS) void ll_finish_kernel(const LlPartial* __restrict__ part, int n_part, float log_scale,
                                                               int mean, float* __restrict__ loss_out, float* __restrict__ grad,
                                                               size_t n_grad) {
  __shared__ double redd[LL_WAVES];
  __shared__ long long redn[LL_WAVES];
  double l = 0.0;
  long long n = 0;
  for (int i = threadIdx.x; i < n_part; i += LL_THREADS) { l += part[i].loss; n += part[i].pairs; }
  l = ll_block_sum<double>(l, redd, LL_WAVES);
  n = ll_block_sum<long long>(n, redn, LL_WAVES);
  const double inv = mean && n > 0 ? 1.0 / (double)n : 1.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) *loss_out = n > 0 ? (float)(-l * (double)log_scale * inv) : 0.f;
  if (mean && grad != nullptr && n > 0) {
    const float f = (float)inv;
    for (size_t i = (size_t)blockIdx.x * LL_THREADS + threadIdx.x; i < n_grad; i += (size_t)gridDim.x * LL_THREADS) grad[i] *= f;
  }
}

template <int NI> void ll_launch_prepare(int B, int threads, hipStream_t s, const float* y_pred, const float* y_true, int S, int kk,
                                         float eps, float pad, const LlWs& w, float* grad_out) {
  ll_prepare_kernel<NI><<<B, threads, 0, s>>>(y_pred, y_true, S, kk, eps, pad, w, grad_out);
}

template <int SCHEME> void ll_launch_pair(dim3 grid, hipStream_t s, const LlArgs& a) {
  ll_pair_kernel<SCHEME><<<grid, LL_THREADS, 0, s>>>(a);
}

}  // namespace
}  // namespace ltr

using namespace ltr;

extern "C" size_t ltr_lambdaloss_workspace_bytes(int32_t B, int32_t S) {
  if (B <= 0 || S <= 0 || S > LL_MAX_S || B > LL_MAX_B) return 0;
  return ll_carve(B, S, nullptr).bytes;
}

extern "C" int ltr_lambdaloss(const float* y_pred, const float* y_true, int32_t B, int32_t S, const ltr_lambdaloss_config* cfg,
                              float* loss_out, float* grad_out, void* workspace, size_t ws_bytes, void* stream) {
  if (!cfg) { set_error("ltr_lambdaloss: NULL config"); return LTR_E_INVAL; }
  if (B < 0 || S < 0 || S > LL_MAX_S || B > LL_MAX_B) {
    set_error("ltr_lambdaloss: bad slate shape [%d, %d] (S <= %d, B <= %d)", B, S, LL_MAX_S, LL_MAX_B); return LTR_E_INVAL;
  }
  if (cfg->scheme < 0 || cfg->scheme >= LL_SCHEMES) { set_error("ltr_lambdaloss: unknown weighing scheme %d", cfg->scheme); return LTR_E_INVAL; }
  if (cfg->reduction != 0 && cfg->reduction != 1) { set_error("ltr_lambdaloss: reduction %d is neither sum (0) nor mean (1)", cfg->reduction); return LTR_E_INVAL; }
  if (cfg->log_base != 0 && cfg->log_base != 1) { set_error("ltr_lambdaloss: log_base %d is neither binary (0) nor natural (1)", cfg->log_base); return LTR_E_INVAL; }
  if (!(cfg->eps > 0.f) || !(cfg->eps < 1.f)) { set_error("ltr_lambdaloss: eps must lie in (0, 1)"); return LTR_E_INVAL; }
  if (B * S == 0) return LTR_OK;
  if (!y_pred || !y_true || !loss_out || !workspace) { set_error("ltr_lambdaloss: NULL pointer"); return LTR_E_INVAL; }
  const LlWs w = ll_carve(B, S, workspace);
  if (ws_bytes < w.bytes) { set_error("ltr_lambdaloss: workspace of %zu bytes, %zu needed for [%d, %d]", ws_bytes, w.bytes, B, S); return LTR_E_NOMEM; }

  hipStream_t s = (hipStream_t)stream;
  const int kk = cfg->k <= 0 || cfg->k > S ? S : cfg->k;
  const float sigma = cfg->sigma > 0.f ? cfg->sigma : 1.f;
  const int threads = std::min(LL_PREP_MAX, (S + 63) / 64 * 64);
  const int ni = (S + threads - 1) / threads;
  if (ni == 1) ll_launch_prepare<1>(B, threads, s, y_pred, y_true, S, kk, cfg->eps, cfg->pad_value, w, grad_out);
  else if (ni == 2) ll_launch_prepare<2>(B, threads, s, y_pred, y_true, S, kk, cfg->eps, cfg->pad_value, w, grad_out);
  else ll_launch_prepare<4>(B, threads, s, y_pred, y_true, S, kk, cfg->eps, cfg->pad_value, w, grad_out);
  LTR_LAUNCH_CHECK();

  LlArgs a{};
  a.S = S; a.kk = kk; a.sigma = sigma; a.mu = cfg->mu; a.l2eps = log2f(cfg->eps);
  a.ws = w; a.grad_out = grad_out;
  a.gscale = cfg->log_base == 0 ? sigma / LL_LN2 : sigma;
  const int tiles = (kk + LL_ROWS - 1) / LL_ROWS;   // the cut shrinks the grid; tiles beyond the valid items leave at once
  const dim3 grid((unsigned)tiles, (unsigned)B);
  switch (cfg->scheme) {
    case LL_NDCG1: ll_launch_pair<LL_NDCG1>(grid, s, a); break;
    case LL_NDCG2: ll_launch_pair<LL_NDCG2>(grid, s, a); break;
    case LL_LAMBDARANK: ll_launch_pair<LL_LAMBDARANK>(grid, s, a); break;
    case LL_NDCG2PP: ll_launch_pair<LL_NDCG2PP>(grid, s, a); break;
    case LL_GTDIFF: ll_launch_pair<LL_GTDIFF>(grid, s, a); break;
    case LL_GTDIFF_POW: ll_launch_pair<LL_GTDIFF_POW>(grid, s, a); break;
    default: ll_launch_pair<LL_NONE>(grid, s, a);   // none and rankNet_scheme: w = 1
  }
  LTR_LAUNCH_CHECK();

  const size_t n_grad = (size_t)B * S;
  const bool scale = cfg->reduction == 1 && grad_out != nullptr;
  const unsigned fin = scale ? (unsigned)std::min<size_t>(64, (n_grad + 4 * LL_THREADS - 1) / (4 * LL_THREADS)) : 1u;
  ll_finish_kernel<<<fin, LL_THREADS, 0, s>>>(w.part, tiles * B, cfg->log_base == 0 ? 1.f : LL_LN2, cfg->reduction, loss_out,
                                              grad_out, n_grad);
  LTR_LAUNCH_CHECK();
  return LTR_OK;
}
