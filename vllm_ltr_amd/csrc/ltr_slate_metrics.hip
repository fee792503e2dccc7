// Slate metrics on gfx950: NDCG@k, DCG@k and MRR@k of allRank's epoch end (train/allrank/models/metrics.py:65-171 - ndcg, dcg,
// __apply_mask_and_get_true_sorted_by_preds, mrr - averaged over the slates as train/allrank/training/train_utils.py:48-72
// `metric_on_epoch` / `compute_metrics` do).  The definition is the one of include/ltr_hip.h (ltr_slate_metrics); in short, per
// slate of S items: an item whose label is pad_value scores -inf and has label 0; the items are ranked by descending score (equal
// scores: lower index first, -0 == +0, a NaN first); dcg[j] = sum over the first min(ats[j], S) positions of gain(label) / log2(2 + r);
// idcg[j] the same with the items ranked by descending label; ndcg = dcg / idcg, or filler_value where idcg == 0; p = position of
// the first maximum of the labels in score order, v that maximum, mrr[j] = 1 / (p + 1) if p < ats[j], else 0.  The reference's
// batch-wide mask is kept: when the v of ALL slates of the call add up to 0, every mrr of the call is 0 - so a slate without a
// relevant item inside a batch that has some keeps p = 0 and mrr = 1.  The means are f64 sums over the slates, rounded once.
//
// Two launches on the caller's stream:
//
//   rank     ONE sort network serves both orders.  Item e carries a 64-bit key (~image(score) << 32 | e) - image() is the
//            order-preserving integer image of the float, so ascending keys are descending scores with the index as tie-break -
//            and a 32-bit key ~image(label) (equal labels have equal gains: no index).  Both go through the same bitonic network
//            over P = the next power of two >= S; the tail [S, P) holds all-ones keys, which sort last.  Element e = m NT + t
//            lives in register slot m of thread t (NT threads, NI = P / NT slots), so a compare-exchange at distance j is
//              j < 64        a cross-lane move inside the wave (__shfl_xor), no LDS, no barrier
//              j >= NT       two register slots of the same thread
//              64 <= j < NT  the only steps that go through LDS: every thread stores its slots, one barrier, reads its partners
//            - 18 of the 78 steps at P = 4096, none for P <= 256.  Two tiers:
//              S <= 64   wave per slate, four slates per 256-thread workgroup, NI = 1: the slate in one key pair per lane,
//                        the whole kernel without LDS and without a barrier
//              S > 64    workgroup per slate, NT = P / 4 (P = 128: 64 threads, NI = 2), 12 P bytes of dynamic LDS (48 KiB at
//                        the limit, under the 64 KiB a launch gets without a function attribute)
//            After the sort thread t holds positions m NT + t of both orders.  The label of a score position is read back through
//            the index in the key (the wave tier: a cross-lane gather), the label of an ideal position is the inverse image of its
//            key.  The discounted gains of both orders go through ONE inclusive block scan in f64 - shuffle scan in the wave, wave
//            totals through LDS, rows m in order with a carry - and the thread that owns position min(ats[j], S) - 1 keeps the
//            value: every cut-off from one pass, and the f32 result carries the rounding of its terms only.  MRR is one
//            reduction of (label, position) pairs under a total order (larger label, then smaller position).
//            The kernel writes dcg / ndcg of its slate (to the workspace, and to the caller's arrays when given) and (p, v).
//   finish   one workgroup: adds the v of all slates (f64, fixed order), forms mrr from p under the batch-wide rule, and the
//            three means.  Thread t takes slates t, t + 1024, ...; the 1024 partial sums are added by a fixed shuffle tree and
//            then in wave order.
//
// No atomics, no memset, no allocation, no host sync; every dependency is a launch boundary.  Two calls give identical bits, a
// slate's dcg / ndcg do not depend on the other slates of the call, and the call can be captured into a graph.  Matrix
// instructions have no use here (compare-exchange and a scan).
#include "ltr_internal.h"

#include <algorithm>

namespace ltr {
namespace {

constexpr int SM_MAX_S = 4096;          // the limit of ltr_listmle and ltr_lambdaloss
constexpr int SM_MAX_B = 1 << 20;
constexpr int SM_MAX_ATS = 8;
constexpr int SM_WAVE_SLATES = 4;       // slates per workgroup of the wave tier
constexpr int SM_MAX_THREADS = 1024;
constexpr int SM_FIN_THREADS = 1024;
constexpr int SM_FIN_WAVES = SM_FIN_THREADS / WAVE;

// per-call workspace: what finish reads of every slate
struct SmWs {
  float *ndcg, *dcg;      // [B, n_ats]
  float* v;               // [B] the largest label of the slate
  int32_t* p;             // [B] its first position in score order
  size_t bytes;
};
SmWs sm_carve(int B, void* base) {
  char* q = (char*)base;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return base ? q + at : nullptr; };
  SmWs w;
  w.ndcg = (float*)take((size_t)B * SM_MAX_ATS * 4); w.dcg = (float*)take((size_t)B * SM_MAX_ATS * 4);
  w.v = (float*)take((size_t)B * 4); w.p = (int32_t*)take((size_t)B * 4);
  w.bytes = o;
  return w;
}

struct SmArgs {
  const float *y_pred, *y_true;
  int B, S, P;
  int n_ats, gain;
  int cut[SM_MAX_ATS];    // min(ats[j], S)
  float pad, filler;
  float *ndcg_out, *dcg_out;
  SmWs ws;
};

// f32 -> u32 that orders like the float: -0 == +0, a NaN (either sign) above everything
__device__ __forceinline__ uint32_t sm_image(float v) {
  if (v != v) return 0xffffffffu;
  const uint32_t u = __float_as_uint(v == 0.f ? 0.f : v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sm_unimage(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ uint64_t sm_shfl_xor(uint64_t v, int j) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, j, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), j, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ float sm_gain(float label, int gain) { return gain == 0 ? exp2f(label) - 1.f : label; }
__device__ __forceinline__ float sm_discount(int r) { return 1.f / log2f((float)(r + 2)); }
// cut[j] for a per-lane j: selects on constant indices (a dynamic index into the kernel arguments would go through scratch)
__device__ __forceinline__ int sm_pick(const int (&cut)[SM_MAX_ATS], int j) {
  int c = cut[0];
#pragma unroll
  for (int i = 1; i < SM_MAX_ATS; ++i) c = j == i ? cut[i] : c;
  return c;
}

// MRR candidate: the first maximum of the labels in score order.  Total order: larger label, then smaller position; the empty
// candidate (-inf, INT_MAX) loses to every item
struct SmBest {
  float l;
  int r;
};
__device__ __forceinline__ bool sm_beats(const SmBest& a, const SmBest& b) { return a.l > b.l || (a.l == b.l && a.r < b.r); }
__device__ __forceinline__ SmBest sm_wave_best(SmBest a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const SmBest b{__shfl_xor(a.l, o, 64), __shfl_xor(a.r, o, 64)};
    if (sm_beats(b, a)) a = b;
  }
  return a;
}

__device__ __forceinline__ double sm_wave_scan(double v, int lane) {       // inclusive, fixed order
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const double u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// Ascending bitonic sort of x (64-bit) and y (32-bit), each over the P elements e = m NT + t.  lx / ly: P slots of LDS each,
// touched only when NT > 64 (the distances 64 <= j < NT).
template <int NI>
__device__ __forceinline__ void sm_sort(uint64_t (&x)[NI], uint32_t (&y)[NI], int t, int NT, int P, uint64_t* lx, uint32_t* ly) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      uint64_t ox[NI];
      uint32_t oy[NI];
      if (j < WAVE) {
#pragma unroll
        for (int m = 0; m < NI; ++m) { ox[m] = sm_shfl_xor(x[m], j); oy[m] = (uint32_t)__shfl_xor((int)y[m], j, 64); }
      } else if (j >= NT) {
#pragma unroll
        for (int m = 0; m < NI; ++m) { ox[m] = x[m]; oy[m] = y[m]; }
#pragma unroll
        for (int d = 1; d < NI; d <<= 1)
          if (j == d * NT) {
#pragma unroll
            for (int m = 0; m < NI; ++m) { ox[m] = x[m ^ d]; oy[m] = y[m ^ d]; }
          }
      } else {
        if constexpr (NI > 1) {
          __syncthreads();                          // the readers of the previous exchange are done
#pragma unroll
          for (int m = 0; m < NI; ++m) { lx[m * NT + t] = x[m]; ly[m * NT + t] = y[m]; }
          __syncthreads();
#pragma unroll
          for (int m = 0; m < NI; ++m) { ox[m] = lx[(m * NT + t) ^ j]; oy[m] = ly[(m * NT + t) ^ j]; }
        }
      }
#pragma unroll
      for (int m = 0; m < NI; ++m) {
        const int e = m * NT + t;
        const bool keep_min = ((e & j) == 0) == ((e & k) == 0);
        x[m] = keep_min ? (ox[m] < x[m] ? ox[m] : x[m]) : (ox[m] > x[m] ? ox[m] : x[m]);
        y[m] = keep_min ? min(y[m], oy[m]) : max(y[m], oy[m]);
      }
    }
  }
}

// keys of element e of the slate at `base`
__device__ __forceinline__ void sm_load(const SmArgs& a, size_t base, int e, uint64_t& x, uint32_t& y, float& label) {
  x = ~0ull; y = ~0u; label = 0.f;
  if (e < a.S) {
    const float l = a.y_true[base + e];
    const bool padded = l == a.pad;
    const float s = padded ? -INFINITY : a.y_pred[base + e];
    label = padded ? 0.f : l;
    x = ((uint64_t)~sm_image(s) << 32) | (uint32_t)e;
    y = ~sm_image(label);
  }
}

// dcg, ndcg of cut-off j of slate b
__device__ __forceinline__ void sm_store(const SmArgs& a, int b, int j, float dcg, float idcg) {
  const float ndcg = idcg == 0.f ? a.filler : dcg / idcg;
  const size_t o = (size_t)b * a.n_ats + j;
  a.ws.dcg[o] = dcg; a.ws.ndcg[o] = ndcg;
  if (a.dcg_out) a.dcg_out[o] = dcg;
  if (a.ndcg_out) a.ndcg_out[o] = ndcg;
}

// ---- wave tier: S <= 64 -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SM_WAVE_SLATES * WAVE) void slate_metrics_wave_kernel(SmArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * SM_WAVE_SLATES + (threadIdx.x >> 6);
  if (b >= a.B) return;                             // the whole wave: nothing below waits for another wave
  const size_t base = (size_t)b * a.S;
  uint64_t x[1];
  uint32_t y[1];
  float own;
  sm_load(a, base, lane, x[0], y[0], own);
  sm_sort<1>(x, y, lane, WAVE, WAVE, nullptr, nullptr);

  const bool live = lane < a.S;                     // position `lane` of both orders
  const float label = __shfl(own, (int)(uint32_t)x[0] & 63, 64);       // (a tail key gathers lane 63; `live` drops it)
  const float disc = sm_discount(lane);
  const double sd = sm_wave_scan(live ? (double)(sm_gain(label, a.gain) * disc) : 0.0, lane);
  const double si = sm_wave_scan(live ? (double)(sm_gain(sm_unimage(~y[0]), a.gain) * disc) : 0.0, lane);
  const int at = sm_pick(a.cut, lane) - 1;          // lane j < n_ats fetches cut-off j
  const int src = lane < a.n_ats ? at : 0;
  const float dcg = (float)__shfl(sd, src, 64), idcg = (float)__shfl(si, src, 64);
  if (lane < a.n_ats) sm_store(a, b, lane, dcg, idcg);

  const SmBest best = sm_wave_best(live ? SmBest{label, lane} : SmBest{-INFINITY, 0x7fffffff});
  if (lane == 0) { a.ws.v[b] = best.l; a.ws.p[b] = best.r; }
}

// ---- workgroup tier: 64 < S <= 4096 -----------------------------------------------------------------------------------------
template <int NI>
__global__ __launch_bounds__(SM_MAX_THREADS) void slate_metrics_block_kernel(SmArgs a) {
  extern __shared__ uint64_t sm_lds[];              // u64 [P] | u32 [P]
  __shared__ double wtot[2][SM_MAX_THREADS / WAVE][2];
  __shared__ float cut_dcg[SM_MAX_ATS], cut_idcg[SM_MAX_ATS];
  __shared__ SmBest wbest[SM_MAX_THREADS / WAVE];
  const int t = threadIdx.x, NT = blockDim.x, lane = t & 63, w = t >> 6, n_waves = NT >> 6;
  const int b = blockIdx.x;
  const size_t base = (size_t)b * a.S;
  uint64_t* lx = sm_lds;
  uint32_t* ly = (uint32_t*)(sm_lds + a.P);

  uint64_t x[NI];
  uint32_t y[NI];
#pragma unroll
  for (int m = 0; m < NI; ++m) {
    float unused;
    sm_load(a, base, m * NT + t, x[m], y[m], unused);
  }
  sm_sort<NI>(x, y, t, NT, a.P, lx, ly);

  double carry_d = 0.0, carry_i = 0.0;
  SmBest best{-INFINITY, 0x7fffffff};
#pragma unroll
  for (int m = 0; m < NI; ++m) {
    const int r = m * NT + t;                       // position r of both orders
    const bool live = r < a.S;                      // (the S real keys sort in front of the tail: a live position holds an index < S)
    float label = 0.f;
    if (live) {
      const float l = a.y_true[base + (uint32_t)x[m]];
      label = l == a.pad ? 0.f : l;
      const SmBest c{label, r};
      if (sm_beats(c, best)) best = c;
    }
    const float disc = sm_discount(r);
    const double sd = sm_wave_scan(live ? (double)(sm_gain(label, a.gain) * disc) : 0.0, lane);
    const double si = sm_wave_scan(live ? (double)(sm_gain(sm_unimage(~y[m]), a.gain) * disc) : 0.0, lane);
    if (lane == 63) { wtot[m & 1][w][0] = sd; wtot[m & 1][w][1] = si; }
    __syncthreads();                                // (row m + 2 writes this buffer again: behind the barrier of row m + 1)
    double pre_d = carry_d, pre_i = carry_i;
    for (int v = 0; v < n_waves; ++v) {             // same address in every lane: broadcast reads
      const double td = wtot[m & 1][v][0], ti = wtot[m & 1][v][1];
      if (v < w) { pre_d += td; pre_i += ti; }
      carry_d += td; carry_i += ti;
    }
#pragma unroll
    for (int j = 0; j < SM_MAX_ATS; ++j)
      if (j < a.n_ats && r == a.cut[j] - 1) { cut_dcg[j] = (float)(pre_d + sd); cut_idcg[j] = (float)(pre_i + si); }
  }

  best = sm_wave_best(best);
  if (lane == 0) wbest[w] = best;
  __syncthreads();
  if (t < a.n_ats) sm_store(a, b, t, cut_dcg[t], cut_idcg[t]);
  if (t == 0) {
    for (int v = 1; v < n_waves; ++v)
      if (sm_beats(wbest[v], best)) best = wbest[v];
    a.ws.v[b] = best.l; a.ws.p[b] = best.r;
  }
}

// ---- finish ---------------------------------------------------------------------------------------------------------------
// sum over the workgroup in a fixed order: shuffle tree inside a wave, then the waves in index order.  Every thread gets it.
__device__ __forceinline__ double sm_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();                                  // red may still be read from the previous sum
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < SM_FIN_WAVES; ++w) s += red[w];
  return s;
}

struct SmFinArgs {
  SmWs ws;
  int B, n_ats;
  int cut[SM_MAX_ATS];
  float *mrr_out, *mean_out;
};

__global__ __launch_bounds__(SM_FIN_THREADS) void slate_metrics_finish_kernel(SmFinArgs a) {
  __shared__ double red[SM_FIN_WAVES];
  const int t = threadIdx.x;
  double vs = 0.0;
  for (int b = t; b < a.B; b += SM_FIN_THREADS) vs += (double)a.ws.v[b];
  const bool none = sm_block_sum(vs, red) == 0.0;   // metrics.py:166-167: a batch-wide scalar mask

  double acc[3][SM_MAX_ATS];
#pragma unroll
  for (int j = 0; j < SM_MAX_ATS; ++j) acc[0][j] = acc[1][j] = acc[2][j] = 0.0;
  for (int b = t; b < a.B; b += SM_FIN_THREADS) {
    const int p = a.ws.p[b];
    const float rr = 1.f / ((float)p + 1.f);
#pragma unroll
    for (int j = 0; j < SM_MAX_ATS; ++j)
      if (j < a.n_ats) {
        const size_t o = (size_t)b * a.n_ats + j;
        const float mrr = !none && p < a.cut[j] ? rr : 0.f;
        if (a.mrr_out) a.mrr_out[o] = mrr;
        acc[0][j] += (double)a.ws.ndcg[o]; acc[1][j] += (double)a.ws.dcg[o]; acc[2][j] += (double)mrr;
      }
  }
  if (!a.mean_out) return;                          // (uniform)
#pragma unroll
  for (int m = 0; m < 3; ++m)
#pragma unroll
    for (int j = 0; j < SM_MAX_ATS; ++j)
      if (j < a.n_ats) {
        const double s = sm_block_sum(acc[m][j], red);
        if (t == 0) a.mean_out[m * a.n_ats + j] = (float)(s / (double)a.B);
      }
}

}  // namespace
}  // namespace ltr

using namespace ltr;

extern "C" size_t ltr_slate_metrics_workspace_bytes(int32_t B, int32_t S) {
  if (B <= 0 || S <= 0 || S > SM_MAX_S || B > SM_MAX_B) return 0;
  return sm_carve(B, nullptr).bytes;
}

extern "C" int ltr_slate_metrics(const float* y_pred, const float* y_true, int32_t B, int32_t S, const ltr_slate_metrics_config* cfg,
                                 float* ndcg_out, float* dcg_out, float* mrr_out, float* mean_out, void* workspace,
                                 size_t ws_bytes, void* stream) {
  if (!cfg) { set_error("ltr_slate_metrics: NULL config"); return LTR_E_INVAL; }
  if (B < 0 || S < 0 || S > SM_MAX_S || B > SM_MAX_B) {
    set_error("ltr_slate_metrics: bad slate shape [%d, %d] (S <= %d, B <= %d)", B, S, SM_MAX_S, SM_MAX_B); return LTR_E_INVAL;
  }
  if (cfg->n_ats < 1 || cfg->n_ats > SM_MAX_ATS) { set_error("ltr_slate_metrics: n_ats = %d outside [1, %d]", cfg->n_ats, SM_MAX_ATS); return LTR_E_INVAL; }
  for (int j = 0; j < cfg->n_ats; ++j)
    if (cfg->ats[j] < 1) { set_error("ltr_slate_metrics: ats[%d] = %d, a cut-off is at least 1", j, cfg->ats[j]); return LTR_E_INVAL; }
  if (cfg->gain != 0 && cfg->gain != 1) { set_error("ltr_slate_metrics: gain %d is neither 2^label - 1 (0) nor label (1)", cfg->gain); return LTR_E_INVAL; }
  if (B * S == 0) return LTR_OK;
  if (!y_pred || !y_true || !workspace) { set_error("ltr_slate_metrics: NULL pointer"); return LTR_E_INVAL; }
  const SmWs w = sm_carve(B, workspace);
  if (ws_bytes < w.bytes) { set_error("ltr_slate_metrics: workspace of %zu bytes, %zu needed for %d slates", ws_bytes, w.bytes, B); return LTR_E_NOMEM; }

  hipStream_t s = (hipStream_t)stream;
  SmArgs a{};
  a.y_pred = y_pred; a.y_true = y_true; a.B = B; a.S = S;
  a.n_ats = cfg->n_ats; a.gain = cfg->gain; a.pad = cfg->pad_value; a.filler = cfg->filler_value;
  a.ndcg_out = ndcg_out; a.dcg_out = dcg_out; a.ws = w;
  SmFinArgs f{};
  f.ws = w; f.B = B; f.n_ats = cfg->n_ats; f.mrr_out = mrr_out; f.mean_out = mean_out;
  for (int j = 0; j < SM_MAX_ATS; ++j) a.cut[j] = f.cut[j] = j < cfg->n_ats ? std::min(cfg->ats[j], S) : 1;

  if (S <= WAVE) {
    a.P = WAVE;
    slate_metrics_wave_kernel<<<(unsigned)((B + SM_WAVE_SLATES - 1) / SM_WAVE_SLATES), SM_WAVE_SLATES * WAVE, 0, s>>>(a);
  } else {
    int P = 128;
    while (P < S) P <<= 1;
    a.P = P;
    const size_t lds = (size_t)P * 12;              // <= 48 KiB
    if (P == 128) slate_metrics_block_kernel<2><<<(unsigned)B, 64, lds, s>>>(a);
    else slate_metrics_block_kernel<4><<<(unsigned)B, P / 4, lds, s>>>(a);
  }
  LTR_LAUNCH_CHECK();
  if (mrr_out || mean_out) {
    slate_metrics_finish_kernel<<<1, SM_FIN_THREADS, 0, s>>>(f);
    LTR_LAUNCH_CHECK();
  }
  return LTR_OK;
}
