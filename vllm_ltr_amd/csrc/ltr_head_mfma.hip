// Hidden-state learning-to-rank head, batched path on the matrix cores of gfx950.
//
// Reference: vllm/model_executor/predictor.py - FCModel (:10-43), OutputLayer (:91-125) - applied to
// (residual + hidden_states).index_select(0, selected_token_indices) in the backbone's own dtype
// (vllm/model_executor/models/opt.py:250-255; the head is built under set_default_torch_dtype(model_config.dtype),
// model_loader/loader.py:234-241).
//
// The row kernel (ltr_head.hip) streams every weight once per row.  Here a workgroup owns a 64-row x 64-output tile of
// one dense layer, so a weight is read once per 64 rows, and the products run on v_mfma_f32_16x16x32_f16 with the
// hi + lo fp16 split of DESIGN.md 2:
//   head_rows_kernel   one wave per selected row: gather, widen f32 / fp16 / bf16, add the residual (rounded once to
//                      the input dtype, as the reference's tensor add), then (mean, rstd) for the input LayerNorm or
//                      the power-of-two split_scale of the row's max|x|.  3 floats per row.
//   head_dense_kernel  Y = act(X W^T + b).  The X tile is fetched in its own dtype, normalised / scaled and split into
//                      hi and lo planes in LDS; the W tile is the checkpoint's fp16 (exact).  K is walked in 64-wide
//                      steps in order, lo product before hi product, f32 accumulators; no split-K, no atomics.  The
//                      epilogue undoes the scale (exact), adds the bias, applies the activation and stores f32 - or, in
//                      the output layer, sums d_output <= 64 values per row in index order (OutputLayer.score).
// Every row's result depends on that row alone: the same instructions in the same order whatever the batch.
#include "ltr_internal.h"

namespace ltr {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int HB_THREADS = 256;
constexpr int HB_BM = 64, HB_BN = 64, HB_BK = 64;   // tile of a workgroup; 4 waves as 2 x 2, 32 x 32 outputs each
constexpr int HB_LD = HB_BK + 8;                    // halves per LDS row: 144 B, the 16-B fragment reads of 8 rows hit 32 different banks
constexpr int HB_PLANE = HB_BM * HB_LD;             // halves per plane (X hi, X lo, W)
constexpr int HB_CLD = HB_BN + 1;                   // floats per row of the output layer's score tile
static_assert(3 * HB_PLANE * 2 >= HB_BM * HB_CLD * 4, "the score tile reuses the operand planes");

// stats[r] = (mean, rstd, 1) with norm, (0, 1, split_scale(max|x|)) without; one wave per row, lanes own groups of four.
// norm == HEAD_NORM_ALLRANK: the encoder's LayerNorm (train/allrank/models/transformer.py:75-97) - unbiased std, eps added
// to std - as (mean, 1 / (std + eps)) in the same two slots, so the dense kernel's loader folds it in like nn.LayerNorm
template <typename T, bool VEC>
__global__ void __launch_bounds__(HB_THREADS) head_rows_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                               const int32_t* __restrict__ row_index, int N, int K,
                                                               int norm, float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (HB_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= N) return;
  const size_t row = row_index ? (size_t)row_index[r] : (size_t)r;
  const T* xr = x + row * K;
  const T* rr = res ? res + row * K : nullptr;
  float o[4], mean = 0.f, rstd = 1.f, scale = 1.f;
  if (norm) {
    float part = 0.f;
    for (int c = lane * 4; c < K; c += 256) { load_x4<T, VEC>(xr, rr, c, K, o); part += (o[0] + o[1]) + (o[2] + o[3]); }
    mean = wave_sum(part) / (float)K;
    float sq = 0.f;
    for (int c = lane * 4; c < K; c += 256) {
      load_x4<T, VEC>(xr, rr, c, K, o);
#pragma unroll
      for (int i = 0; i < 4; ++i) { const float d = c + i < K ? o[i] - mean : 0.f; sq += d * d; }
    }
    rstd = norm == HEAD_NORM_ALLRANK ? 1.f / (sqrtf(wave_sum(sq) / (float)(K - 1)) + ALLRANK_LN_EPS)
                                     : rsqrtf(wave_sum(sq) / (float)K + LN_EPS);
  } else {
    float amax = 0.f;
    for (int c = lane * 4; c < K; c += 256) {
      load_x4<T, VEC>(xr, rr, c, K, o);
      amax = fmaxf(amax, fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fmaxf(fabsf(o[2]), fabsf(o[3]))));
    }
    scale = split_scale(wave_max(amax));
  }
  if (lane == 0) { stats[3 * (size_t)r] = mean; stats[3 * (size_t)r + 1] = rstd; stats[3 * (size_t)r + 2] = scale; }
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(HB_THREADS) head_dense_kernel(DenseArgs a) {
  __shared__ __attribute__((aligned(16))) __half smem[3 * HB_PLANE];
  __shared__ float s_inv[HB_BM];
  __half* s_hi = smem;
  __half* s_lo = smem + HB_PLANE;
  __half* s_w = smem + 2 * HB_PLANE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int m0 = blockIdx.x * HB_BM, n0 = blockIdx.y * HB_BN;
  const int K = a.K;
  const bool norm = a.ln_w != nullptr;

  // loader role: thread -> (tile row tid / 4, 16 consecutive k) of the X tile and of the W tile
  const int lrow = tid >> 2, lk = (tid & 3) * 16;
  const bool xvalid = m0 + lrow < a.N;
  const bool wvalid = n0 + lrow < a.O;
  const size_t srow = xvalid ? (a.row_index ? (size_t)a.row_index[m0 + lrow] : (size_t)(m0 + lrow)) : 0;
  const T* xr = reinterpret_cast<const T*>(a.x) + srow * K;
  const T* rr = a.res ? reinterpret_cast<const T*>(a.res) + srow * K : nullptr;
  const __half* wp = a.w + (size_t)(wvalid ? n0 + lrow : 0) * K;
  float mean = 0.f, rstd = 0.f, scale = 0.f;
  if (xvalid) {
    const float* st = a.stats + 3 * (size_t)(m0 + lrow);
    mean = own_reg(st[0]); rstd = own_reg(st[1]); scale = own_reg(st[2]);
  }
  if (tid < HB_BM) s_inv[tid] = m0 + tid < a.N ? 1.f / a.stats[3 * (size_t)(m0 + tid) + 2] : 0.f;   // power of two: exact

  float fx[16], fg[16], fb[16];
  f16x8 fw[2];
  auto fetch = [&](int k0) {
    const int c = k0 + lk;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (xvalid) load_x4<T, VEC>(xr, rr, c + 4 * i, K, fx + 4 * i);
      else fx[4 * i] = fx[4 * i + 1] = fx[4 * i + 2] = fx[4 * i + 3] = 0.f;
      if (norm) {
        load4<float, VEC>(a.ln_w, c + 4 * i, K, fg + 4 * i);
        load4<float, VEC>(a.ln_b, c + 4 * i, K, fb + 4 * i);
      }
    }
    if (VEC) {
      if (wvalid && c < K) {
        fw[0] = *reinterpret_cast<const f16x8*>(wp + c);
        fw[1] = *reinterpret_cast<const f16x8*>(wp + c + 8);
      } else {
        fw[0] = fw[1] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const __half h = wvalid && c + i < K ? wp[c + i] : __half(0.f);
        fw[i >> 3][i & 7] = __builtin_bit_cast(_Float16, h);
      }
    }
  };
  // normalise / scale, split, and put the fetched pieces into LDS; the K tail (g = b = 0, x = 0) and rows past N become 0
  auto commit = [&]() {
    f16x8 hi[2], lo[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float v = norm ? (fx[i] - mean) * rstd * fg[i] + fb[i] : fx[i] * scale;
      if (!xvalid) v = 0.f;
      __half h, l;
      split_f16(v, h, l);
      hi[i >> 3][i & 7] = __builtin_bit_cast(_Float16, h);
      lo[i >> 3][i & 7] = __builtin_bit_cast(_Float16, l);
    }
    const int off = lrow * HB_LD + lk;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<f16x8*>(s_hi + off + 8 * i) = hi[i];
      *reinterpret_cast<f16x8*>(s_lo + off + 8 * i) = lo[i];
      *reinterpret_cast<f16x8*>(s_w + off + 8 * i) = fw[i];
    }
  };

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int frow = lane & 15, fk = (lane >> 4) * 8;
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += HB_BK) {
    commit();
    __syncthreads();
    if (k0 + HB_BK < K) fetch(k0 + HB_BK);      // in flight under the MFMAs of this step
#pragma unroll
    for (int ks = 0; ks < HB_BK; ks += 32) {
      f16x8 ah[2], al[2], bw[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int ro = (wr * 32 + i * 16 + frow) * HB_LD + ks + fk;
        ah[i] = *reinterpret_cast<const f16x8*>(s_hi + ro);
        al[i] = *reinterpret_cast<const f16x8*>(s_lo + ro);
        bw[i] = *reinterpret_cast<const f16x8*>(s_w + (wc * 32 + i * 16 + frow) * HB_LD + ks + fk);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bw[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bw[j], acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();                            // the planes are free for the next step (and for the score tile)
  }

  // epilogue.  16x16 C layout: col = lane & 15, row = 4 * (lane >> 4) + e
  float* s_c = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int tc = wc * 32 + j * 16 + (lane & 15), gc = n0 + tc;
    const float bj = gc < a.O ? a.bias[gc] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int tr = wr * 32 + i * 16 + 4 * (lane >> 4) + e, gr = m0 + tr;
        const float v = apply_act(acc[i][j][e] * s_inv[tr] + bj, a.act);
        if (a.scores) s_c[tr * HB_CLD + tc] = gc < a.O ? v : 0.f;
        else if (gr < a.N && gc < a.O) {
          const size_t o = (size_t)gr * a.O + gc;
          a.out[o] = a.resid ? a.resid[o] + v : v;      // the element is read and written by this thread alone: resid may be out
        }
      }
  }
  if (a.scores) {     // OutputLayer.score: the sum over d_output runs in index order, as the row kernel's
    __syncthreads();
    if (tid < HB_BM && m0 + tid < a.N) {
      float s = 0.f;
      for (int j = 0; j < a.O; ++j) s += s_c[tid * HB_CLD + j];
      a.scores[m0 + tid] = s;
    }
  }
}

// d_output > HB_BN: the output layer's activations went to the workspace; one thread sums a row in index order
__global__ void __launch_bounds__(HB_THREADS) head_sum_kernel(const float* __restrict__ y, int N, int O,
                                                              float* __restrict__ scores) {
  const int r = blockIdx.x * HB_THREADS + threadIdx.x;
  if (r >= N) return;
  float s = 0.f;
  for (int j = 0; j < O; ++j) s += y[(size_t)r * O + j];
  scores[r] = s;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// widest activation that goes through the workspace: every FC layer's, and the output layer's when it is not reduced in place
int ws_width(const HeadModel* m) {
  int w = 0;
  for (int i = 0; i < m->L.n; ++i)
    if (i < m->L.n - 1 || m->L.out[i] > HB_BN) w = max(w, m->L.out[i]);
  return w;
}

template <typename T, bool VEC> void launch_layer_v(const DenseArgs& a, hipStream_t s) {
  head_rows_kernel<T, VEC><<<(a.N + 3) / 4, HB_THREADS, 0, s>>>((const T*)a.x, (const T*)a.res, a.row_index, a.N, a.K,
                                                               a.ln_w != nullptr ? a.norm_kind : 0, a.stats);
  head_dense_kernel<T, VEC><<<dim3((a.N + HB_BM - 1) / HB_BM, (a.O + HB_BN - 1) / HB_BN), HB_THREADS, 0, s>>>(a);
}

template <typename T> void launch_layer(const DenseArgs& a, hipStream_t s) {
  const bool vec = a.K % 16 == 0 && al16(a.x) && al16(a.res) && al16(a.w) && al16(a.ln_w) && al16(a.ln_b);
  if (vec) launch_layer_v<T, true>(a, s); else launch_layer_v<T, false>(a, s);
}

}  // namespace

int head_ws_width(const HeadModel* m) { return ws_width(m); }

void launch_head_dense(const DenseArgs& a, int x_dtype, hipStream_t s) {
  if (x_dtype == LTR_HID_F32) launch_layer<float>(a, s);
  else if (x_dtype == LTR_HID_F16) launch_layer<__half>(a, s);
  else launch_layer<bf16_t>(a, s);
}

int launch_head_layers(const HeadModel* m, int li0, int li1, const void* x, const void* res, int x_dtype,
                       const int32_t* row_index, const float* ln_w, const float* ln_b, int norm_kind, int N, float* stats,
                       float* const buf[2], float* scores_out, hipStream_t s, const float** cur_out) {
  const float* cur = nullptr;
  for (int li = li0; li < li1; ++li) {
    const bool first = li == li0, last = li == m->L.n - 1;
    DenseArgs a;
    a.x = first ? x : (const void*)cur;
    a.res = first ? res : nullptr;
    a.row_index = first ? row_index : nullptr;
    a.stats = stats;
    a.ln_w = first ? ln_w : nullptr;
    a.ln_b = first ? ln_b : nullptr;
    a.norm_kind = norm_kind;
    a.w = (const __half*)m->L.w[li];
    a.bias = m->L.b[li];
    a.out = buf[li & 1];
    a.scores = last && m->L.out[li] <= HB_BN ? scores_out : nullptr;
    a.N = N; a.K = m->L.in[li]; a.O = m->L.out[li];
    a.act = last ? m->d.output_activation : m->d.activation;
    launch_head_dense(a, first ? x_dtype : LTR_HID_F32, s);
    LTR_LAUNCH_CHECK();
    cur = a.out;
  }
  if (li1 == m->L.n && m->L.out[li1 - 1] > HB_BN) {
    head_sum_kernel<<<(N + HB_THREADS - 1) / HB_THREADS, HB_THREADS, 0, s>>>(cur, N, m->L.out[li1 - 1], scores_out);
    LTR_LAUNCH_CHECK();
  }
  if (cur_out) *cur_out = cur;
  return LTR_OK;
}

}  // namespace ltr

using namespace ltr;

extern "C" {

size_t ltr_head_workspace_bytes(ltr_head_handle h, int32_t N) {
  const HeadModel* m = (const HeadModel*)h;
  if (!m || N <= 0) return 0;
  return align256((size_t)N * 3 * sizeof(float)) + 2 * align256((size_t)N * ws_width(m) * sizeof(float));
}

int ltr_head_score_batched(ltr_head_handle h, const void* hidden, const void* residual, int32_t hidden_dtype,
                           const int32_t* row_index, int32_t N, float* scores_out, void* workspace, size_t ws_bytes,
                           void* stream) {
  if (N < 0) { set_error("ltr_head_score_batched: negative N"); return LTR_E_INVAL; }
  if (hidden_dtype != LTR_HID_F32 && hidden_dtype != LTR_HID_F16 && hidden_dtype != LTR_HID_BF16) {
    set_error("ltr_head_score_batched: bad hidden_dtype %d (LTR_HID_F32 | LTR_HID_F16 | LTR_HID_BF16)", hidden_dtype);
    return LTR_E_INVAL;
  }
  const HeadModel* m = (const HeadModel*)h;
  if (!m) { set_error("ltr_head_score_batched: NULL handle"); return LTR_E_INVAL; }
  if (m->d.weight_dtype != LTR_W_F16) {
    set_error("ltr_head_score_batched: LTR_W_F32 weights are not exact in fp16; use the row path (ltr_head_score)");
    return LTR_E_INVAL;
  }
  if (N == 0) return LTR_OK;
  if (!hidden || !scores_out || !workspace) { set_error("ltr_head_score_batched: NULL argument"); return LTR_E_INVAL; }
  const size_t need = ltr_head_workspace_bytes(h, N);
  if (ws_bytes < need) {
    set_error("ltr_head_score_batched: workspace of %zu bytes, %zu needed for N = %d", ws_bytes, need, N);
    return LTR_E_NOMEM;
  }
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const size_t act_bytes = align256((size_t)N * ws_width(m) * sizeof(float));
  float* stats = (float*)ws;
  float* buf[2] = {(float*)(ws + align256((size_t)N * 3 * sizeof(float))),
                   (float*)(ws + align256((size_t)N * 3 * sizeof(float)) + act_bytes)};
  return launch_head_layers(m, 0, m->L.n, hidden, residual, hidden_dtype, row_index, m->ln_w, m->ln_b, HEAD_NORM_TORCH, N,
                            stats, buf, scores_out, s, nullptr);
}

}  // extern "C"
