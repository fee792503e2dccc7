// Order agreement of two score vectors on gfx950: the pair counts behind Kendall's tau-b (the reference's training metric,
// train/trainer.py:195: scipy.stats.kendalltau of the test labels against the predictions) and the discordant-pair gaps the
// parity reports quote ("N of 33.5 M pairs differ, every one a near-tie": the queue orders of
// benchmarks/benchmark_throughput_original.py:396-443 compared pair by pair).
//
// For x, y f32 [n], every unordered pair i < j is classified by sx = sign(x_i - x_j), sy = sign(y_i - y_j) under IEEE f32
// comparison (+0 == -0, infinities ordered, a NaN orders with nothing):
//   concordant sx sy > 0 | discordant sx sy < 0 | tie_x sx == 0, sy != 0 | tie_y sx != 0, sy == 0 | tie_xy both 0 |
//   unordered: one of the four values is a NaN
// and over the discordant pairs: max |x_i - x_j|, max |y_i - y_j| (f32), and the lexicographically smallest pair (i, j) that
// attains the first.  tau-b itself is three host flops on these integers (vllm_ltr_amd/metrics.py).
//
// Shape of the work: n (n - 1) / 2 independent compare-and-count steps on 8 n bytes of input - pure VALU work, no memory
// traffic to speak of.  The index range is cut into tiles of 1024; one 256-thread workgroup owns a tile pair (I, J), J >= I (a
// triangular grid of Tn (Tn + 1) / 2 workgroups, J-major so that neighbours share their J tile in L2).  Tile J sits in LDS as
// interleaved (x, y) float2 - 8 KB; in the inner loop every lane reads the SAME address, a conflict-free broadcast
// ds_read_b64 - and every thread holds four elements of tile I in registers, so one LDS read feeds four pairs.  Per pair: six
// compares, the logic that turns them into five 0 / 1 flags, five integer adds into per-thread 32-bit counters (<= 4096 pairs
// per thread and workgroup: no overflow) and the running gap maximum.  What must not count - j <= i on a diagonal tile pair,
// the ragged end of the last tile - is fed in as a NaN x, for which all six compares are false; `unordered` is the number of
// pairs a thread owns (known in closed form) minus the five flags, so real NaNs and masked pairs share one code path.
// Counters go through wave shuffles, then across the four waves through LDS, and the workgroup writes ONE partial record to
// workspace[block]; a second, single-workgroup launch adds the partials and merges the gap candidates under a total order
// (larger gap, then smaller (i, j)).  No atomics, no workgroup waits for another, nothing is cleared beforehand: integer sums
// and a total order make the result independent of scheduling - bit-reproducible - and the two launches can be captured
// into a graph.
#include "ltr_internal.h"

namespace ltr {
namespace {

constexpr int OA_TILE = 1024;
constexpr int OA_THREADS = 256;
constexpr int OA_WAVES = OA_THREADS / WAVE;
constexpr int OA_PER = OA_TILE / OA_THREADS;      // elements of tile I per thread
constexpr int64_t OA_MAXN = 1 << 20;              // 524,800 workgroups, 33.6 MB of partials; (i, j) and the grid stay far inside int32
constexpr int OA_NCNT = 6;

using OaResult = ltr_order_agreement_result;
static_assert(sizeof(OaResult) == 64, "ltr_order_agreement_result is 64 bytes (metrics.py reads it back as such)");

// candidate for "the discordant pair with the largest |x_i - x_j|"; g = -1, i = j = -1: none yet
struct OaGap {
  float g;
  int i, j;
};
// total order of the candidates: larger gap first, then the lexicographically smaller pair
__device__ __forceinline__ bool oa_beats(const OaGap& a, const OaGap& b) {
  return a.g > b.g || (a.g == b.g && (a.i < b.i || (a.i == b.i && a.j < b.j)));
}
__device__ __forceinline__ OaGap oa_shfl_xor(const OaGap& a, int o) {
  return OaGap{__shfl_xor(a.g, o, 64), __shfl_xor(a.i, o, 64), __shfl_xor(a.j, o, 64)};
}

// Tile pair of a linear workgroup id, J-major: b = J (J + 1) / 2 + I with I <= J.  floor(sqrt(2 b)) by bits (integers only)
// is J or J + 1; the loops settle it.
__device__ __forceinline__ void oa_decode(uint32_t b, int& I, int& J) {
  const uint64_t v = 2ull * b;
  uint64_t r = 0;
  for (uint64_t bit = 1u << 15; bit; bit >>= 1) {
    const uint64_t t = r | bit;
    if (t * t <= v) r = t;
  }
  while (r * (r + 1) / 2 > b) --r;
  while ((r + 1) * (r + 2) / 2 <= b) ++r;
  J = (int)r;
  I = (int)(b - r * (r + 1) / 2);
}

// the j loop of one workgroup.  DIAG: I == J, only j > i counts.
template <bool DIAG>
__device__ __forceinline__ void oa_scan(const float2* __restrict__ sj, int jcount, const float (&xi)[OA_PER],
                                        const float (&yi)[OA_PER], const int (&il)[OA_PER], uint32_t (&cnt)[OA_NCNT],
                                        float (&bg)[OA_PER], int (&bj)[OA_PER], float& gap_y) {
  float2 next = sj[0];
  for (int j = 0; j < jcount; ++j) {
    const float2 p = next;                         // same address in every lane: broadcast read,
    next = sj[j + 1];                              // issued one step ahead (sj has a spare slot behind the tile)
    const float pjy = own_reg(p.y);                // (keeps the high half of the 64-bit read out of packed f32 math: isa_lint.py)
#pragma unroll
    for (int k = 0; k < OA_PER; ++k) {
      const float pjx = DIAG ? (j > il[k] ? p.x : __builtin_nanf("")) : p.x;
      const bool gx = xi[k] > pjx, lx = xi[k] < pjx, ex = xi[k] == pjx;
      const bool gy = yi[k] > pjy, ly = yi[k] < pjy, ey = yi[k] == pjy;
      const bool disc = (gx && ly) || (lx && gy);
      cnt[0] += (uint32_t)((gx && gy) || (lx && ly));
      cnt[1] += (uint32_t)disc;
      cnt[2] += (uint32_t)(ex && (gy || ly));
      cnt[3] += (uint32_t)((gx || lx) && ey);
      cnt[4] += (uint32_t)(ex && ey);
      const float g = disc ? fabsf(xi[k] - pjx) : -1.f;
      const bool up = g > bg[k];                   // j ascends: the first maximum is the smallest j of this i
      bg[k] = up ? g : bg[k];
      bj[k] = up ? j : bj[k];
      gap_y = fmaxf(gap_y, disc ? fabsf(yi[k] - pjy) : 0.f);
    }
  }
}

__global__ __launch_bounds__(OA_THREADS) void order_agreement_tile_kernel(const float* __restrict__ x,
                                                                          const float* __restrict__ y, int n,
                                                                          OaResult* __restrict__ part) {
  __shared__ float2 sj[OA_TILE + 1];             // + 1: the scan reads one element ahead
  __shared__ uint32_t red_cnt[OA_WAVES][OA_NCNT];
  __shared__ float red_gy[OA_WAVES];
  __shared__ OaGap red_gap[OA_WAVES];
  const int t = threadIdx.x;
  int I, J;
  oa_decode(blockIdx.x, I, J);
  const int i0 = I * OA_TILE, j0 = J * OA_TILE;
  const int jcount = min(OA_TILE, n - j0);
  const bool diag = I == J;

  float xi[OA_PER], yi[OA_PER];
  int il[OA_PER];
  uint32_t owned = 0;                              // pairs this thread classifies
#pragma unroll
  for (int k = 0; k < OA_PER; ++k) {
    const int l = t + k * OA_THREADS;              // strided: coalesced loads, and i ascends with k
    const int j = j0 + l, i = i0 + l;
    sj[l] = j < n ? make_float2(x[j], y[j]) : make_float2(0.f, 0.f);
    il[k] = l;
    const bool live = i < n;
    xi[k] = live ? x[i] : __builtin_nanf("");      // a NaN x: every compare false, the element counts nowhere
    yi[k] = live ? y[i] : 0.f;
    if (live) owned += (uint32_t)(diag ? max(jcount - 1 - l, 0) : jcount);
  }
  if (t == 0) sj[OA_TILE] = make_float2(0.f, 0.f);
  __syncthreads();

  uint32_t cnt[OA_NCNT] = {0, 0, 0, 0, 0, 0};
  float bg[OA_PER];
  int bj[OA_PER];
#pragma unroll
  for (int k = 0; k < OA_PER; ++k) { bg[k] = -1.f; bj[k] = -1; }
  float gap_y = 0.f;
  if (diag) oa_scan<true>(sj, jcount, xi, yi, il, cnt, bg, bj, gap_y);
  else      oa_scan<false>(sj, jcount, xi, yi, il, cnt, bg, bj, gap_y);
  cnt[5] = owned - (cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[4]);

  OaGap best{-1.f, -1, -1};
#pragma unroll
  for (int k = 0; k < OA_PER; ++k)                 // i ascends with k: strict > keeps the smaller i
    if (bg[k] > best.g) best = OaGap{bg[k], i0 + il[k], j0 + bj[k]};

#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int c = 0; c < OA_NCNT; ++c) cnt[c] += __shfl_xor(cnt[c], o, 64);     // <= 64 x 4096 per wave
    gap_y = fmaxf(gap_y, __shfl_xor(gap_y, o, 64));
    const OaGap other = oa_shfl_xor(best, o);
    if (oa_beats(other, best)) best = other;
  }
  const int w = t >> 6;
  if ((t & 63) == 0) {
#pragma unroll
    for (int c = 0; c < OA_NCNT; ++c) red_cnt[w][c] = cnt[c];
    red_gy[w] = gap_y;
    red_gap[w] = best;
  }
  __syncthreads();
  if (t == 0) {
    for (int v = 1; v < OA_WAVES; ++v) {
      for (int c = 0; c < OA_NCNT; ++c) cnt[c] += red_cnt[v][c];                // <= 2^20 per workgroup
      gap_y = fmaxf(gap_y, red_gy[v]);
      if (oa_beats(red_gap[v], best)) best = red_gap[v];
    }
    OaResult r;
    r.concordant = cnt[0]; r.discordant = cnt[1]; r.tie_x = cnt[2]; r.tie_y = cnt[3]; r.tie_xy = cnt[4]; r.unordered = cnt[5];
    r.max_gap_x = best.g; r.max_gap_y = gap_y; r.gap_i = best.i; r.gap_j = best.j;
    part[blockIdx.x] = r;
  }
}

// sum of the partial records, merge of their gap candidates; n_part == 0 (n < 2) writes the empty result
__global__ __launch_bounds__(OA_THREADS) void order_agreement_final_kernel(const OaResult* __restrict__ part, int n_part,
                                                                           OaResult* __restrict__ out) {
  __shared__ long long red_cnt[OA_WAVES][OA_NCNT];
  __shared__ float red_gy[OA_WAVES];
  __shared__ OaGap red_gap[OA_WAVES];
  const int t = threadIdx.x;
  long long cnt[OA_NCNT] = {0, 0, 0, 0, 0, 0};
  float gap_y = 0.f;
  OaGap best{-1.f, -1, -1};
  for (int b = t; b < n_part; b += OA_THREADS) {
    const OaResult r = part[b];
    cnt[0] += r.concordant; cnt[1] += r.discordant; cnt[2] += r.tie_x; cnt[3] += r.tie_y; cnt[4] += r.tie_xy; cnt[5] += r.unordered;
    gap_y = fmaxf(gap_y, r.max_gap_y);
    const OaGap g{r.max_gap_x, r.gap_i, r.gap_j};
    if (oa_beats(g, best)) best = g;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int c = 0; c < OA_NCNT; ++c) cnt[c] += __shfl_xor(cnt[c], o, 64);
    gap_y = fmaxf(gap_y, __shfl_xor(gap_y, o, 64));
    const OaGap other = oa_shfl_xor(best, o);
    if (oa_beats(other, best)) best = other;
  }
  const int w = t >> 6;
  if ((t & 63) == 0) {
#pragma unroll
    for (int c = 0; c < OA_NCNT; ++c) red_cnt[w][c] = cnt[c];
    red_gy[w] = gap_y;
    red_gap[w] = best;
  }
  __syncthreads();
  if (t == 0) {
    for (int v = 1; v < OA_WAVES; ++v) {
      for (int c = 0; c < OA_NCNT; ++c) cnt[c] += red_cnt[v][c];
      gap_y = fmaxf(gap_y, red_gy[v]);
      if (oa_beats(red_gap[v], best)) best = red_gap[v];
    }
    OaResult r;
    r.concordant = cnt[0]; r.discordant = cnt[1]; r.tie_x = cnt[2]; r.tie_y = cnt[3]; r.tie_xy = cnt[4]; r.unordered = cnt[5];
    const bool any = best.i >= 0;                  // no discordant pair: gaps 0, pair (-1, -1)
    r.max_gap_x = any ? best.g : 0.f; r.max_gap_y = any ? gap_y : 0.f; r.gap_i = best.i; r.gap_j = best.j;
    *out = r;
  }
}

int64_t oa_blocks(int64_t n) {
  if (n < 2) return 0;
  const int64_t tiles = (n + OA_TILE - 1) / OA_TILE;
  return tiles * (tiles + 1) / 2;
}

}  // namespace
}  // namespace ltr

using namespace ltr;

extern "C" size_t ltr_order_agreement_workspace_bytes(int64_t n) {
  if (n < 0 || n > OA_MAXN) return 0;
  return (size_t)oa_blocks(n) * sizeof(OaResult);
}

extern "C" int ltr_order_agreement(const float* x, const float* y, int32_t n, ltr_order_agreement_result* result_out,
                                   void* workspace, size_t ws_bytes, void* stream) {
  if (n < 0 || n > OA_MAXN) { set_error("ltr_order_agreement: n = %d outside [0, %lld]", n, (long long)OA_MAXN); return LTR_E_INVAL; }
  if (!result_out || (n > 0 && (!x || !y))) { set_error("ltr_order_agreement: NULL pointer"); return LTR_E_INVAL; }
  const int64_t blocks = oa_blocks(n);
  const size_t need = (size_t)blocks * sizeof(OaResult);
  if (need && (!workspace || ws_bytes < need)) {
    set_error("ltr_order_agreement: workspace too small (%zu < %zu)", workspace ? ws_bytes : (size_t)0, need);
    return LTR_E_INVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  OaResult* part = (OaResult*)workspace;
  if (blocks) {
    order_agreement_tile_kernel<<<(unsigned)blocks, OA_THREADS, 0, s>>>(x, y, n, part);
    LTR_LAUNCH_CHECK();
  }
  order_agreement_final_kernel<<<1, OA_THREADS, 0, s>>>(part, (int)blocks, result_out);
  LTR_LAUNCH_CHECK();
  return LTR_OK;
}
