// Slate encoder of the hidden-state learning-to-rank head on gfx950 (DESIGN.md 4.4 "slate encoder").
//
// Reference: train/allrank/models/transformer.py - Encoder (:44-72), LayerNorm (:75-97: unbiased std, eps added to std),
// SublayerConnection (:100-122: x + sublayer(norm(x))), EncoderLayer (:125-150), attention (:153-172),
// MultiHeadedAttention (:175-219), PositionwiseFeedForward (:222-243), make_transformer (:246-263) - placed between the FC
// stack and the output layer by train/allrank/models/model.py:28-166 (LTRModel.prepare_for_output, make_model :147-161).
// Scoring only: dropout is the identity; the slates of a call are unpadded row ranges, so there is no padding mask.
//
// Projections, feed-forward and the output layer run on head_dense_kernel (ltr_head_mfma.hip) with allRank's norm folded
// into the tile load and the residual added in the epilogue.  New here:
//   slate_attn_kernel  out = softmax(Q K^T / sqrt(d_k)) V per (slate, head), not causal.  A workgroup of 4 waves owns a tile
//                      of 64 query rows of one (slate, head) - 16 rows per wave, Q fragments (scaled by log2(e) / sqrt(d_k),
//                      split hi + lo) in registers - and walks the slate's keys in tiles of BK: K hi / lo row-major and
//                      V hi / lo TRANSPOSED in LDS (the contraction of P V runs over keys, and an MFMA operand holds 8
//                      consecutive contraction indices).  S = Ql Kh + Qh Kl + Qh Kh and O += Pl Vh + Ph Vl + Ph Vh on
//                      v_mfma_f32_16x16x32_f16, small terms first; the lo x lo terms (2^-22 of the product) are dropped.
//                      Softmax is online in the exp2 domain, running max and sum in f32 per query row; P goes from the
//                      accumulator layout to the operand layout through a per-wave LDS tile.  Keys past the slate's end
//                      are zero in LDS and -inf in S; query rows past it are zero and never stored.  A workgroup strides
//                      over its slate's query tiles, so the grid's x size (from max_slate) is a matter of speed only.
// Everything a slate's rows see is that slate's rows, in an order fixed by the slate's own length: bit-identical whatever
// else is in the call.  No atomics, no memset, no allocation, no function attribute, no wait between workgroups.
#include "ltr_internal.h"

namespace ltr {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int SA_THREADS = 256;
constexpr int SA_BQ = 64;          // query rows of a workgroup: 16 per wave
constexpr int ENC_MAX_BLOCKS = 16;
constexpr int ENC_PER_BLOCK = 12;  // weight pointers per encoder block

struct EncoderBlock {
  const float *n0_a, *n0_b;   // sublayer.0.norm
  const __half* wqkv;         // [3 d_model, d_model]: linears.0 | linears.1 | linears.2
  const float* bqkv;
  const __half* wo;           // linears.3
  const float* bo;
  const float *n1_a, *n1_b;   // sublayer.1.norm
  const __half* w1;           // [d_ff, d_model]
  const float* b1;
  const __half* w2;           // [d_model, d_ff]
  const float* b2;
};

struct HeadEncoder {
  const HeadModel* head;
  ltr_head_encoder_desc d;
  int d_model, d_k;
  EncoderBlock blk[ENC_MAX_BLOCKS];
  const float *fin_a, *fin_b;   // encoder.norm
};

// z[r] = the selected row in f32: (hidden + residual)[row_index[r]], the sum rounded once to T (fc_model = None: the
// encoder's residual stream starts at the rows themselves)
template <typename T>
__global__ void __launch_bounds__(SA_THREADS) enc_gather_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                                const int32_t* __restrict__ row_index, int N, int K,
                                                                float* __restrict__ z) {
  const int groups = (K + 3) / 4;
  const size_t i = (size_t)blockIdx.x * SA_THREADS + threadIdx.x;
  if (i >= (size_t)N * groups) return;
  const int r = (int)(i / groups), c = (int)(i % groups) * 4;
  const size_t row = row_index ? (size_t)row_index[r] : (size_t)r;
  float o[4];
  load_x4<T, false>(x + row * K, res ? res + row * K : nullptr, c, K, o);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (c + j < K) z[(size_t)r * K + c + j] = o[j];
}

__device__ __forceinline__ void split4(const float f[4], f16x4& hi, f16x4& lo) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    __half h, l;
    split_f16(f[i], h, l);
    hi[i] = __builtin_bit_cast(_Float16, h);
    lo[i] = __builtin_bit_cast(_Float16, l);
  }
}

// DKP: d_k rounded up to the MFMA's K of 32 (the pad is zero in registers and LDS); BK: keys per tile
template <int DKP, int BK>
__global__ void __launch_bounds__(SA_THREADS) slate_attn_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ cu,
                                                                int N, int dm, int dk, float qscale,
                                                                float* __restrict__ out) {
  constexpr int KLD = DKP + 8;            // halves per K row: 16-byte fragment reads of 8 rows spread over the banks
  constexpr int VLD = BK + 8;             // halves per row of V^T and of P
  constexpr int TPK = SA_THREADS / BK;    // loader threads per key
  constexpr int LGRP = DKP / 4 / TPK;     // groups of four d per loader thread
  static_assert(DKP % 32 == 0 && BK % 32 == 0 && (DKP / 4) % TPK == 0, "tile shape");
  __shared__ __attribute__((aligned(16))) __half s_k[2][BK * KLD];       // hi, lo
  __shared__ __attribute__((aligned(16))) __half s_v[2][DKP * VLD];      // V^T hi, lo: [d][key]
  __shared__ __attribute__((aligned(16))) __half s_p[4][2][16 * VLD];    // per wave: P hi, lo [query][key]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hh = blockIdx.z;
  int s0 = 0, s1 = N;
  if (cu != nullptr) {      // clamped: a malformed cu_slates reads and writes inside the call's N rows
    s0 = min(max(cu[blockIdx.y], 0), N);
    s1 = min(max(cu[blockIdx.y + 1], s0), N);
  }
  const int len = s1 - s0;
  const int ld = 3 * dm;
  const float* qb = qkv + (size_t)s0 * ld + hh * dk;
  const float* kb = qb + dm;
  const float* vb = qb + 2 * dm;
  const int frow = lane & 15, fk = (lane >> 4) * 8;   // operand fragment: row / column frow, 8 contraction indices from fk
  const int crow = 4 * (lane >> 4), ccol = lane & 15; // accumulator: rows crow + e, column ccol
  const int lkey = tid / TPK, lg = tid % TPK;

  for (int q0 = blockIdx.x * SA_BQ; q0 < len; q0 += gridDim.x * SA_BQ) {
    f16x8 qh[DKP / 32], ql[DKP / 32];
    {
      const int qr = q0 + wave * 16 + frow;
#pragma unroll
      for (int ks = 0; ks < DKP / 32; ++ks) {
        const int d = ks * 32 + fk;
        float a[8];                     // d_k is a multiple of 16: a group of 8 lies inside the head or in the pad (0)
        load4<float, true>(qb + (size_t)qr * ld, d, qr < len ? dk : 0, a);
        load4<float, true>(qb + (size_t)qr * ld, d + 4, qr < len ? dk : 0, a + 4);
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] *= qscale;
        f16x4 h0, l0, h1, l1;
        split4(a, h0, l0);
        split4(a + 4, h1, l1);
        qh[ks] = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
        ql[ks] = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
      }
    }
    f32x4 o[DKP / 16];
#pragma unroll
    for (int i = 0; i < DKP / 16; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { m[e] = -INFINITY; l[e] = 0.f; }

    for (int k0 = 0; k0 < len; k0 += BK) {
      __syncthreads();                  // the previous tile's readers are done
      {
        const int kr = k0 + lkey;
#pragma unroll
        for (int i = 0; i < LGRP; ++i) {
          const int d = 4 * (lg + TPK * i);
          float kx[4], vx[4];           // zero in the pad and past the slate's end
          load4<float, true>(kb + (size_t)kr * ld, d, kr < len ? dk : 0, kx);
          load4<float, true>(vb + (size_t)kr * ld, d, kr < len ? dk : 0, vx);
          f16x4 h4, l4;
          split4(kx, h4, l4);
          *reinterpret_cast<f16x4*>(&s_k[0][lkey * KLD + d]) = h4;
          *reinterpret_cast<f16x4*>(&s_k[1][lkey * KLD + d]) = l4;
          split4(vx, h4, l4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const _Float16 hj = h4[j], lj = l4[j];      // a copy: bit_cast of the element lvalue itself reads element 0
            s_v[0][(d + j) * VLD + lkey] = __builtin_bit_cast(__half, hj);
            s_v[1][(d + j) * VLD + lkey] = __builtin_bit_cast(__half, lj);
          }
        }
      }
      __syncthreads();

      f32x4 sacc[BK / 16];
#pragma unroll
      for (int j = 0; j < BK / 16; ++j) {
        sacc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < DKP / 32; ++ks) {
          const int off = (j * 16 + frow) * KLD + ks * 32 + fk;
          const f16x8 kh = *reinterpret_cast<const f16x8*>(&s_k[0][off]);
          const f16x8 kl = *reinterpret_cast<const f16x8*>(&s_k[1][off]);
          sacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ql[ks], kh, sacc[j], 0, 0, 0);
          sacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qh[ks], kl, sacc[j], 0, 0, 0);
          sacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qh[ks], kh, sacc[j], 0, 0, 0);
        }
      }
      // online softmax of the wave's 16 rows: lane (crow + e, ccol) of every 16-key piece
      float alpha[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < BK / 16; ++j) {
          if (k0 + j * 16 + ccol >= len) sacc[j][e] = -INFINITY;
          mx = fmaxf(mx, sacc[j][e]);
        }
#pragma unroll
        for (int w = 8; w > 0; w >>= 1) mx = fmaxf(mx, __shfl_xor(mx, w, 64));
        const float mn = fmaxf(m[e], mx);     // finite: the first key of a tile is always inside the slate
        alpha[e] = __builtin_amdgcn_exp2f(m[e] - mn);
        m[e] = mn;
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < BK / 16; ++j) {
          const float p = __builtin_amdgcn_exp2f(sacc[j][e] - mn);
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
          const f16x8 vh = *reinterpret_cast<const f16x8*>(&s_v[0][off]);
          const f16x8 vl = *reinterpret_cast<const f16x8*>(&s_v[1][off]);
          o[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pl, vh, o[i], 0, 0, 0);
          o[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ph, vl, o[i], 0, 0, 0);
          o[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ph, vh, o[i], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int qr = q0 + wave * 16 + crow + e;
      if (qr >= len) continue;
      const float inv = 1.f / l[e];
      float* orow = out + (size_t)(s0 + qr) * dm + hh * dk;
#pragma unroll
      for (int i = 0; i < DKP / 16; ++i)
        if (i * 16 + ccol < dk) orow[i * 16 + ccol] = o[i][e] * inv;
    }
  }
}

void launch_slate_attn(const float* qkv, const int32_t* cu, int N, int B, int max_slate, int dm, int h, float* out,
                       hipStream_t s) {
  const int dk = dm / h;
  const float qscale = 1.44269504088896341f / sqrtf((float)dk);
  const dim3 grid((max_slate + SA_BQ - 1) / SA_BQ, B, h);
  if (dk <= 32) slate_attn_kernel<32, 64><<<grid, SA_THREADS, 0, s>>>(qkv, cu, N, dm, dk, qscale, out);
  else if (dk <= 64) slate_attn_kernel<64, 64><<<grid, SA_THREADS, 0, s>>>(qkv, cu, N, dm, dk, qscale, out);
  else if (dk <= 96) slate_attn_kernel<96, 32><<<grid, SA_THREADS, 0, s>>>(qkv, cu, N, dm, dk, qscale, out);
  else slate_attn_kernel<128, 32><<<grid, SA_THREADS, 0, s>>>(qkv, cu, N, dm, dk, qscale, out);
}

size_t enc_act_width(const HeadEncoder* e) { return (size_t)max(head_ws_width(e->head), e->d_model); }

}  // namespace

int launch_enc_gather(const void* x, const void* res, int x_dtype, const int32_t* row_index, int N, int K, float* z,
                      hipStream_t s) {
  const unsigned blocks = (unsigned)(((size_t)N * ((K + 3) / 4) + SA_THREADS - 1) / SA_THREADS);
  if (x_dtype == LTR_HID_F32)
    enc_gather_kernel<float><<<blocks, SA_THREADS, 0, s>>>((const float*)x, (const float*)res, row_index, N, K, z);
  else if (x_dtype == LTR_HID_F16)
    enc_gather_kernel<__half><<<blocks, SA_THREADS, 0, s>>>((const __half*)x, (const __half*)res, row_index, N, K, z);
  else
    enc_gather_kernel<bf16_t><<<blocks, SA_THREADS, 0, s>>>((const bf16_t*)x, (const bf16_t*)res, row_index, N, K, z);
  LTR_LAUNCH_CHECK();
  return LTR_OK;
}

}  // namespace ltr

using namespace ltr;

extern "C" {

int ltr_head_encoder_create(ltr_head_handle head, const ltr_head_encoder_desc* d, const void* const* weights,
                            int32_t n_weights, ltr_head_encoder_handle* out) {
  if (!head || !d || !weights || !out) { set_error("ltr_head_encoder_create: NULL argument"); return LTR_E_INVAL; }
  const HeadModel* m = (const HeadModel*)head;
  const int dm = m->L.in[m->L.n - 1];
  if (m->d.weight_dtype != LTR_W_F16) {
    set_error("ltr_head_encoder_create: LTR_W_F32 weights are not exact in fp16; the encoder needs an LTR_W_F16 head");
    return LTR_E_INVAL;
  }
  if (d->positional_encoding != 0) {
    set_error("ltr_head_encoder_create: positional_encoding is not built (a queue has no item order to encode)");
    return LTR_E_INVAL;
  }
  if (d->n_blocks < 1 || d->n_blocks > ENC_MAX_BLOCKS || d->d_ff < 1 || d->d_ff > 65536 || d->h < 1) {
    set_error("ltr_head_encoder_create: bad shape (N=%d d_ff=%d h=%d)", d->n_blocks, d->d_ff, d->h);
    return LTR_E_INVAL;
  }
  if (dm < 2) { set_error("ltr_head_encoder_create: d_model = %d: the unbiased std of one value does not exist", dm); return LTR_E_INVAL; }
  if (dm % d->h != 0) { set_error("ltr_head_encoder_create: h = %d does not divide d_model = %d", d->h, dm); return LTR_E_INVAL; }
  const int dk = dm / d->h;
  if (dk % 16 != 0 || dk > 128) {
    set_error("ltr_head_encoder_create: d_k = %d (a multiple of 16 up to 128)", dk);
    return LTR_E_INVAL;
  }
  const int want = ENC_PER_BLOCK * d->n_blocks + 2;
  if (n_weights != want) { set_error("ltr_head_encoder_create: %d weight pointers, expected %d", n_weights, want); return LTR_E_INVAL; }
  for (int i = 0; i < want; ++i)
    if (!weights[i]) { set_error("ltr_head_encoder_create: weight pointer %d is NULL", i); return LTR_E_INVAL; }
  HeadEncoder* e = new HeadEncoder();
  e->head = m; e->d = *d; e->d_model = dm; e->d_k = dk;
  for (int b = 0; b < d->n_blocks; ++b) {
    const void* const* w = weights + ENC_PER_BLOCK * b;
    EncoderBlock& k = e->blk[b];
    k.n0_a = (const float*)w[0]; k.n0_b = (const float*)w[1];
    k.wqkv = (const __half*)w[2]; k.bqkv = (const float*)w[3];
    k.wo = (const __half*)w[4]; k.bo = (const float*)w[5];
    k.n1_a = (const float*)w[6]; k.n1_b = (const float*)w[7];
    k.w1 = (const __half*)w[8]; k.b1 = (const float*)w[9];
    k.w2 = (const __half*)w[10]; k.b2 = (const float*)w[11];
  }
  e->fin_a = (const float*)weights[want - 2];
  e->fin_b = (const float*)weights[want - 1];
  *out = (ltr_head_encoder_handle)e;
  return LTR_OK;
}

int ltr_head_encoder_destroy(ltr_head_encoder_handle enc) { delete (HeadEncoder*)enc; return LTR_OK; }

size_t ltr_head_encoder_workspace_bytes(ltr_head_encoder_handle enc, int32_t N) {
  const HeadEncoder* e = (const HeadEncoder*)enc;
  if (!e || N <= 0) return 0;
  const size_t n = (size_t)N, f = sizeof(float);
  return align256(n * 3 * f) + 2 * align256(n * enc_act_width(e) * f) + align256(n * 3 * e->d_model * f) +
         align256(n * e->d_model * f) + align256(n * e->d.d_ff * f);
}

int ltr_head_encoder_score(ltr_head_encoder_handle enc, const void* hidden, const void* residual, int32_t hidden_dtype,
                           const int32_t* row_index, int32_t N, const int32_t* cu_slates, int32_t B, int32_t max_slate,
                           float* scores_out, void* workspace, size_t ws_bytes, void* stream) {
  const HeadEncoder* e = (const HeadEncoder*)enc;
  if (!e) { set_error("ltr_head_encoder_score: NULL handle"); return LTR_E_INVAL; }
  if (N < 0 || B < 0 || B > 65535) { set_error("ltr_head_encoder_score: bad N = %d or B = %d (0 .. 65535 slates)", N, B); return LTR_E_INVAL; }
  if (hidden_dtype != LTR_HID_F32 && hidden_dtype != LTR_HID_F16 && hidden_dtype != LTR_HID_BF16) {
    set_error("ltr_head_encoder_score: bad hidden_dtype %d (LTR_HID_F32 | LTR_HID_F16 | LTR_HID_BF16)", hidden_dtype);
    return LTR_E_INVAL;
  }
  if (!cu_slates && B != 1) { set_error("ltr_head_encoder_score: cu_slates is NULL and B = %d (NULL: one slate of N rows)", B); return LTR_E_INVAL; }
  if (N == 0) return LTR_OK;
  if (B < 1) { set_error("ltr_head_encoder_score: %d rows in no slate", N); return LTR_E_INVAL; }
  if (!hidden || !scores_out || !workspace) { set_error("ltr_head_encoder_score: NULL argument"); return LTR_E_INVAL; }
  const size_t need = ltr_head_encoder_workspace_bytes(enc, N);
  if (ws_bytes < need) {
    set_error("ltr_head_encoder_score: workspace of %zu bytes, %zu needed for N = %d", ws_bytes, need, N);
    return LTR_E_NOMEM;
  }
  if (max_slate < 1 || max_slate > N) max_slate = N;
  const HeadModel* m = e->head;
  const int dm = e->d_model, n_fc = m->L.n - 1;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const size_t f = sizeof(float), n = (size_t)N;
  float* stats = (float*)ws; ws += align256(n * 3 * f);
  float* buf[2];
  buf[0] = (float*)ws; ws += align256(n * enc_act_width(e) * f);
  buf[1] = (float*)ws; ws += align256(n * enc_act_width(e) * f);
  float* qkv = (float*)ws; ws += align256(n * 3 * dm * f);
  float* att = (float*)ws; ws += align256(n * dm * f);
  float* ff = (float*)ws;

  // 1. z = FC(x): the residual stream, in buf[(n_fc + 1) & 1] - not where the output layer may write
  float* z = buf[(n_fc + 1) & 1];
  if (n_fc > 0) {
    const int rc = launch_head_layers(m, 0, n_fc, hidden, residual, hidden_dtype, row_index, m->ln_w, m->ln_b,
                                      HEAD_NORM_TORCH, N, stats, buf, nullptr, s, nullptr);
    if (rc != LTR_OK) return rc;
  } else {
    const int rc = launch_enc_gather(hidden, residual, hidden_dtype, row_index, N, dm, z, s);
    if (rc != LTR_OK) return rc;
  }
  // 2. the blocks (EncoderLayer.forward, transformer.py:142-150)
  auto dense = [&](const float* x, const float* na, const float* nb, const __half* w, const float* bias, int K, int O,
                   int act, const float* resid, float* out) {
    DenseArgs a;
    a.x = x; a.res = nullptr; a.row_index = nullptr; a.stats = stats;
    a.ln_w = na; a.ln_b = nb; a.norm_kind = HEAD_NORM_ALLRANK;
    a.w = w; a.bias = bias; a.resid = resid; a.out = out; a.scores = nullptr;
    a.N = N; a.K = K; a.O = O; a.act = act;
    launch_head_dense(a, LTR_HID_F32, s);
  };
  for (int b = 0; b < e->d.n_blocks; ++b) {
    const EncoderBlock& k = e->blk[b];
    dense(z, k.n0_a, k.n0_b, k.wqkv, k.bqkv, dm, 3 * dm, ACT_NONE, nullptr, qkv);
    LTR_LAUNCH_CHECK();
    launch_slate_attn(qkv, cu_slates, N, B, max_slate, dm, e->d.h, att, s);
    LTR_LAUNCH_CHECK();
    dense(att, nullptr, nullptr, k.wo, k.bo, dm, dm, ACT_NONE, z, z);
    LTR_LAUNCH_CHECK();
    dense(z, k.n1_a, k.n1_b, k.w1, k.b1, dm, e->d.d_ff, ACT_RELU, nullptr, ff);
    LTR_LAUNCH_CHECK();
    dense(ff, nullptr, nullptr, k.w2, k.b2, e->d.d_ff, dm, ACT_NONE, z, z);
    LTR_LAUNCH_CHECK();
  }
  // 3. encoder.norm folded into the output layer's tile load, then OutputLayer.score
  return launch_head_layers(m, n_fc, n_fc + 1, z, nullptr, LTR_HID_F32, nullptr, e->fin_a, e->fin_b, HEAD_NORM_ALLRANK, N,
                            stats, buf, scores_out, s, nullptr);
}

}  // extern "C"
