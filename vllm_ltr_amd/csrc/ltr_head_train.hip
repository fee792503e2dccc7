// Training of the hidden-state learning-to-rank head on the matrix cores of gfx950 (DESIGN.md 4.4 "training").
//
// Reference: the head is vllm/model_executor/predictor.py (:126-145 only Xavier-initialises it), the encoder-less copy of
// allRank's FCModel / OutputLayer / LTRModel (train/allrank/models/model.py:28-166); allRank's loop trains those classes
// (train/allrank/training/train_utils.py:34-45: loss, backward, clip_grad_norm_, opt.step).  ltr_head_train_step is one
// such step on M = B * S selected rows of stored hidden states.
//
// Precision.  Parameters, gradients and Adam moments are f32.  Every product is split x split: both operands are scaled by
// a power of two taken from max|.| of their tensor (split_scale; the maximum by a two-stage reduction whose second stage
// is a wave_max in the consumer), split into fp16 hi + lo, and multiplied on v_mfma_f32_16x16x32_f16 as lo.hi, hi.lo and
// hi.hi (lo.lo is 2^-22 relative and dropped), f32 accumulation in a fixed K order; the epilogue undoes the scales exactly.
// The input LayerNorm's output is O(1) and is split unscaled, as the scoring path does.
//
// Kernels (all 256 threads = 4 waves as 2 x 2, a workgroup owns a 64 x 64 output tile, LDS planes of 64 x 72 halves so
// that the 16-byte fragment reads of 8 rows hit 32 different banks; tails are zero-filled in LDS, any width runs):
//   ht_rows_kernel      (mean, rstd) or max|x| per selected row of the first layer's input, which is never materialised
//   ht_gemm_img_kernel  C[m, n] = sum_k X[m, k] Img[n, k].  X is fetched by the forward's tile loader (gather through
//                       row_index, widen f32 / fp16 / bf16, residual added and rounded once, LayerNorm from the row
//                       statistics) or is a plain f32 workspace tensor; Img is a library-kept hi | lo image.
//                       forward:  Img = W [out, in];  epilogue adds the bias and stores Z and A = act(Z)
//                       dX:       Img = W^T [in, out] (so the contraction over outputs is contiguous for both fragments);
//                                 epilogue multiplies by act'(Z_{l-1}) and stores dZ_{l-1}
//   ht_gemm_dw_kernel   dW[o, i] = sum_m dZ[m, o] X[m, i]: the contraction is the slow dimension of both operands; the
//                       row-major 64 x 64 tiles are loaded coalesced (a thread owns two rows x 8 columns), scaled and
//                       split in registers and written TRANSPOSED (one 32-bit store per row pair) into the planes.
//                       Layers with fewer than HT_DW_WIDE output tiles cut M into parts of HT_DW_PART rows - constants,
//                       not functions of the grid or the device - and write partials that are added in part order.
//   column sums         bias / LayerNorm gradients: f64 partials per HT_CS_PART rows, then a sum in part order
//   norm, clip          sum of squares per fixed chunk, then one thread adds the chunks in order (clip_grad_norm_)
//   ht_adam_tile_kernel torch.optim.Adam on a 64 x 64 tile of a matrix + the refreshed hi | lo images of W and, through an
//                       LDS transpose, of W^T; vectors use the element-wise form
// With an encoder (ltr_head_train_create_encoder) the same kernels run its five dense layers per block - allRank's norm
// rides on the tile loader's (x - mean) rstd g + b with rstd = 1 / (std + eps) - around the attention and norm kernels of
// ltr_head_encoder_train.hip.
// No atomics, no memset, no allocation in a step, no waiting between workgroups: every dependency is a launch boundary.
// A step cannot be captured into a graph as it stands: Adam's bias corrections are host-side arguments.
#include "ltr_internal.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <type_traits>
#include <vector>

namespace ltr {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int HT_THREADS = 256;
constexpr int HT_TILE = 64;
constexpr int HT_LD = HT_TILE + 8;            // halves per LDS row: 144 B
constexpr int HT_PLANE = HT_TILE * HT_LD;     // halves per plane
constexpr int HT_AMAX_NB = 64;                // first-stage maxima per tensor
constexpr int HT_DW_PART = 512;               // rows per part of a narrow layer's weight gradient
constexpr int HT_DW_WIDE = 256;               // output tiles from which a layer walks all of M in one part
constexpr int HT_CS_PART = 256;               // rows per part of a column sum
constexpr int HT_SQ_NB = 256;                 // chunks of the sum of squares
constexpr int HT_MAX_LAYERS = 9;              // 8 FC layers + the output layer
constexpr int HT_MAX_ROWS = 1 << 22;
constexpr int HT_ENC_BLOCKS = 16;             // most encoder blocks (ltr_head_encoder_create)
constexpr int HT_ENC_PER_BLOCK = 12;          // tensors per encoder block: norm 0, QKV, W_o, norm 1, w_1, w_2 as (a, b) / (W, b)
constexpr int HT_MAX_MATS = HT_MAX_LAYERS + 4 * HT_ENC_BLOCKS;

// derivative of apply_act at pre-activation z (ReLU: 0 at 0, as torch)
__device__ __forceinline__ float act_grad(float z, int act) {
  switch (act) {
    case ACT_RELU: return z > 0.f ? 1.f : 0.f;
    case ACT_SIGMOID: { const float s = 1.f / (1.f + expf(-z)); return s * (1.f - s); }
    case ACT_TANH: { const float t = tanhf(z); return 1.f - t * t; }
    case ACT_GELU: return 0.5f * (1.f + erff(z * 0.70710678118654752f)) + z * 0.3989422804014327f * expf(-0.5f * z * z);
    case ACT_SILU: { const float s = 1.f / (1.f + expf(-z)); return s * (1.f + z * (1.f - s)); }
    default: return 1.f;
  }
}

// second stage of the two-stage max + the power-of-two scale; every lane of the wave calls it.  nullptr: 1 (LayerNorm output)
__device__ __forceinline__ float tensor_scale(const float* __restrict__ part) {
  return part ? split_scale(wave_max(part[threadIdx.x & 63])) : 1.f;
}
static_assert(HT_AMAX_NB == 64, "tensor_scale reads one first-stage maximum per lane");

// A row-major operand [rows, K]: the first layer's input (x of T, gathered, + residual, LayerNorm'd) or a plain f32 tensor
struct XSrc {
  const void* x;
  const void* res;            // same dtype and shape as x, or nullptr
  const int32_t* row_index;   // or nullptr
  const float* stats;         // [M][2] (mean, rstd) of ht_rows_kernel; read when ln_w is set
  const float* ln_w;          // [K]; non-null: LayerNorm on load
  const float* ln_b;
  const float* amax;          // HT_AMAX_NB first-stage maxima of the tensor, or nullptr: scale 1
  int K;
  int vec;                    // K % 16 == 0 and 16-byte aligned bases: groups of four are one aligned load
};

template <typename T> __device__ __forceinline__ void xload4(const XSrc& s, const T* xr, const T* rr, int c, float o[4]) {
  if (s.vec) load_x4<T, true>(xr, rr, c, s.K, o); else load_x4<T, false>(xr, rr, c, s.K, o);
}
__device__ __forceinline__ void fload4(const float* p, int c, int K, int vec, float o[4]) {
  if (vec) load4<float, true>(p, c, K, o); else load4<float, false>(p, c, K, o);
}
template <typename T> __device__ __forceinline__ const T* xrow(const void* base, size_t row, int K) {
  return base ? reinterpret_cast<const T*>(base) + row * (size_t)K : nullptr;
}

// stats[r] = (mean, rstd) with norm, rowmax[r] = max|x| without; one wave per row (the arithmetic of head_rows_kernel)
template <typename T>
__global__ void __launch_bounds__(HT_THREADS) ht_rows_kernel(XSrc s, int M, float* __restrict__ stats, float* __restrict__ rowmax) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (HT_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= M) return;
  const size_t row = s.row_index ? (size_t)s.row_index[r] : (size_t)r;
  const int K = s.K;
  const T* xr = xrow<T>(s.x, row, K);
  const T* rr = xrow<T>(s.res, row, K);
  float o[4], mean = 0.f, rstd = 1.f, amax = 0.f;
  if (s.ln_w) {
    float part = 0.f;
    for (int c = lane * 4; c < K; c += 256) { xload4<T>(s, xr, rr, c, o); part += (o[0] + o[1]) + (o[2] + o[3]); }
    mean = wave_sum(part) / (float)K;
    float sq = 0.f;
    for (int c = lane * 4; c < K; c += 256) {
      xload4<T>(s, xr, rr, c, o);
#pragma unroll
      for (int i = 0; i < 4; ++i) { const float d = c + i < K ? o[i] - mean : 0.f; sq += d * d; }
    }
    rstd = rsqrtf(wave_sum(sq) / (float)K + LN_EPS);
  } else {
    for (int c = lane * 4; c < K; c += 256) {
      xload4<T>(s, xr, rr, c, o);
      amax = fmaxf(amax, fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fmaxf(fabsf(o[2]), fabsf(o[3]))));
    }
    amax = wave_max(amax);
  }
  if (lane == 0) { stats[2 * (size_t)r] = mean; stats[2 * (size_t)r + 1] = rstd; rowmax[r] = amax; }
}

// first stage of max|x|: workgroup b owns the b-th of HT_AMAX_NB equal chunks and always writes part[b]
__global__ void __launch_bounds__(HT_THREADS) ht_amax_kernel(const float* __restrict__ x, size_t n, float* __restrict__ part) {
  __shared__ float sm[4];
  const size_t chunk = (n + HT_AMAX_NB - 1) / HT_AMAX_NB;
  const size_t beg = (size_t)blockIdx.x * chunk, end = beg + chunk < n ? beg + chunk : n;
  float m = 0.f;
  for (size_t i = beg + threadIdx.x; i < end; i += HT_THREADS) m = fmaxf(m, fabsf(x[i]));
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
}

// the 3-product split MFMA step over one 64-wide slice of the contraction held in the four planes
__device__ __forceinline__ void mma_tile(const __half* s_ah, const __half* s_al, const __half* s_bh, const __half* s_bl,
                                         int wr, int wc, int lane, f32x4 acc[2][2]) {
  const int frow = lane & 15, fk = (lane >> 4) * 8;
#pragma unroll
  for (int ks = 0; ks < HT_TILE; ks += 32) {
    f16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int ra = (wr * 32 + i * 16 + frow) * HT_LD + ks + fk;
      const int rb = (wc * 32 + i * 16 + frow) * HT_LD + ks + fk;
      ah[i] = *reinterpret_cast<const f16x8*>(s_ah + ra);
      al[i] = *reinterpret_cast<const f16x8*>(s_al + ra);
      bh[i] = *reinterpret_cast<const f16x8*>(s_bh + rb);
      bl[i] = *reinterpret_cast<const f16x8*>(s_bl + rb);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
      }
  }
}

enum { HT_MODE_FWD = 0, HT_MODE_DX = 1 };
struct ImgArgs {
  XSrc a;                  // [M, K]
  const __half* img;       // hi plane [ceil64(N)][ld], zero-padded; lo plane at img + plane
  size_t plane;
  int ld;                  // ceil64(K)
  const float* img_amax;   // first-stage maxima the image was scaled by
  const float* bias;       // forward: [N]
  float* Z;                // forward: [M, N] pre-activation
  float* A;                // forward: [M, N] act(Z)
  const float* Zprev;      // dX: [M, N] pre-activation whose act' multiplies the product, or nullptr
  float* out;              // dX: [M, N]
  int M, N, K, act, mode;
};

template <typename T>
__global__ void __launch_bounds__(HT_THREADS) ht_gemm_img_kernel(ImgArgs g) {
  __shared__ __attribute__((aligned(16))) __half smem[4 * HT_PLANE];
  __half* s_ah = smem;
  __half* s_al = smem + HT_PLANE;
  __half* s_bh = smem + 2 * HT_PLANE;
  __half* s_bl = smem + 3 * HT_PLANE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int m0 = blockIdx.x * HT_TILE, n0 = blockIdx.y * HT_TILE;
  const int K = g.K;
  const bool norm = g.a.ln_w != nullptr;
  const float sa = tensor_scale(g.a.amax), sb = tensor_scale(g.img_amax);

  // loader role: thread -> (tile row tid / 4, 16 consecutive k) of the X tile and of the image tile
  const int lrow = tid >> 2, lk = (tid & 3) * 16;
  const bool xvalid = m0 + lrow < g.M;
  const size_t srow = xvalid ? (g.a.row_index ? (size_t)g.a.row_index[m0 + lrow] : (size_t)(m0 + lrow)) : 0;
  const T* xr = xrow<T>(g.a.x, srow, K);
  const T* rr = xrow<T>(g.a.res, srow, K);
  const __half* ip = g.img + (size_t)(n0 + lrow) * g.ld;      // the image has ceil64(N) rows of ceil64(K) halves
  float mean = 0.f, rstd = 0.f;
  if (xvalid && norm) { mean = own_reg(g.a.stats[2 * (size_t)(m0 + lrow)]); rstd = own_reg(g.a.stats[2 * (size_t)(m0 + lrow) + 1]); }

  float fx[16], fg[16], fb[16];
  f16x8 fh[2], fl[2];
  auto fetch = [&](int k0) {
    const int c = k0 + lk;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (xvalid) xload4<T>(g.a, xr, rr, c + 4 * i, fx + 4 * i);
      else fx[4 * i] = fx[4 * i + 1] = fx[4 * i + 2] = fx[4 * i + 3] = 0.f;
      if (norm) {
        fload4(g.a.ln_w, c + 4 * i, K, g.a.vec, fg + 4 * i);
        fload4(g.a.ln_b, c + 4 * i, K, g.a.vec, fb + 4 * i);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      fh[i] = *reinterpret_cast<const f16x8*>(ip + c + 8 * i);
      fl[i] = *reinterpret_cast<const f16x8*>(ip + g.plane + c + 8 * i);
    }
  };
  // normalise / scale, split, and put the fetched pieces into LDS; the K tail (g = b = 0, x = 0) and rows past M become 0
  auto commit = [&]() {
    f16x8 hi[2], lo[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float v = norm ? (fx[i] - mean) * rstd * fg[i] + fb[i] : fx[i] * sa;
      if (!xvalid) v = 0.f;
      __half h, l;
      split_f16(v, h, l);
      hi[i >> 3][i & 7] = __builtin_bit_cast(_Float16, h);
      lo[i >> 3][i & 7] = __builtin_bit_cast(_Float16, l);
    }
    const int off = lrow * HT_LD + lk;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<f16x8*>(s_ah + off + 8 * i) = hi[i];
      *reinterpret_cast<f16x8*>(s_al + off + 8 * i) = lo[i];
      *reinterpret_cast<f16x8*>(s_bh + off + 8 * i) = fh[i];
      *reinterpret_cast<f16x8*>(s_bl + off + 8 * i) = fl[i];
    }
  };

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += HT_TILE) {
    commit();
    __syncthreads();
    if (k0 + HT_TILE < K) fetch(k0 + HT_TILE);      // in flight under the MFMAs of this step
    mma_tile(s_ah, s_al, s_bh, s_bl, wr, wc, lane, acc);
    __syncthreads();
  }

  // epilogue.  16x16 C layout: col = lane & 15, row = 4 * (lane >> 4) + e.  1 / scale is a power of two: exact
  const float inva = 1.f / sa, invb = 1.f / sb;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int gc = n0 + wc * 32 + j * 16 + (lane & 15);
    if (gc >= g.N) continue;
    const float bj = g.mode == HT_MODE_FWD ? g.bias[gc] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int gr = m0 + wr * 32 + i * 16 + 4 * (lane >> 4) + e;
        if (gr >= g.M) continue;
        const size_t o = (size_t)gr * g.N + gc;
        const float v = acc[i][j][e] * inva * invb;
        if (g.mode == HT_MODE_FWD) {
          const float z = v + bj;
          g.Z[o] = z;
          g.A[o] = apply_act(z, g.act);
        } else {
          g.out[o] = g.Zprev ? v * act_grad(g.Zprev[o], g.act) : v;
        }
      }
  }
}

struct DwArgs {
  XSrc a;          // dZ [M, O], plain f32
  XSrc b;          // X [M, K]
  float* out;      // [parts][O][K]
  int M, O, K, part_rows;
};

template <typename T>
__global__ void __launch_bounds__(HT_THREADS) ht_gemm_dw_kernel(DwArgs g) {
  __shared__ __attribute__((aligned(16))) __half smem[4 * HT_PLANE];
  __half* s_ah = smem;
  __half* s_al = smem + HT_PLANE;
  __half* s_bh = smem + 2 * HT_PLANE;
  __half* s_bl = smem + 3 * HT_PLANE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int o0 = blockIdx.x * HT_TILE, i0 = blockIdx.y * HT_TILE;
  const int m_beg = blockIdx.z * g.part_rows, m_end = min(g.M, m_beg + g.part_rows);
  const bool norm = g.b.ln_w != nullptr;
  const float sa = tensor_scale(g.a.amax), sb = tensor_scale(g.b.amax);

  // loader role: thread -> (rows 2 pr and 2 pr + 1 of the 64-row slice, 8 consecutive columns) of both tiles
  const int pr = tid >> 3, ca = o0 + (tid & 7) * 8, cb = i0 + (tid & 7) * 8;
  float lg[8], lb[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) lg[i] = lb[i] = 0.f;
  if (norm) {
    fload4(g.b.ln_w, cb, g.K, g.b.vec, lg); fload4(g.b.ln_w, cb + 4, g.K, g.b.vec, lg + 4);
    fload4(g.b.ln_b, cb, g.K, g.b.vec, lb); fload4(g.b.ln_b, cb + 4, g.K, g.b.vec, lb + 4);
  }
  float fa[2][8], fx[2][8], mean[2], rstd[2];
  bool valid[2];
  auto fetch = [&](int m0) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int gm = m0 + 2 * pr + r;
      valid[r] = gm < m_end;
      mean[r] = 0.f; rstd[r] = 0.f;
      if (valid[r]) {
        const float* ar = reinterpret_cast<const float*>(g.a.x) + (size_t)gm * g.O;
        fload4(ar, ca, g.O, g.a.vec, fa[r]); fload4(ar, ca + 4, g.O, g.a.vec, fa[r] + 4);
        const size_t srow = g.b.row_index ? (size_t)g.b.row_index[gm] : (size_t)gm;
        const T* xr = xrow<T>(g.b.x, srow, g.K);
        const T* rr = xrow<T>(g.b.res, srow, g.K);
        xload4<T>(g.b, xr, rr, cb, fx[r]); xload4<T>(g.b, xr, rr, cb + 4, fx[r] + 4);
        if (norm) { mean[r] = own_reg(g.b.stats[2 * (size_t)gm]); rstd[r] = own_reg(g.b.stats[2 * (size_t)gm + 1]); }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) fa[r][i] = fx[r][i] = 0.f;
      }
    }
  };
  // scale, split and write TRANSPOSED: plane row = column of the tile, plane column = row of the slice; one 32-bit store
  // holds the two rows of a thread.  Columns past the width (x = g = b = 0) and rows past the part become 0
  auto pack = [](__half a, __half b) { return (uint32_t)__half_as_ushort(a) | ((uint32_t)__half_as_ushort(b) << 16); };
  auto commit = [&]() {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      __half h[2], l[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) split_f16(fa[r][i] * sa, h[r], l[r]);
      const int off = ((tid & 7) * 8 + i) * HT_LD + 2 * pr;
      *reinterpret_cast<uint32_t*>(s_ah + off) = pack(h[0], h[1]);
      *reinterpret_cast<uint32_t*>(s_al + off) = pack(l[0], l[1]);
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        float v = norm ? (fx[r][i] - mean[r]) * rstd[r] * lg[i] + lb[i] : fx[r][i] * sb;
        if (!valid[r]) v = 0.f;
        split_f16(v, h[r], l[r]);
      }
      *reinterpret_cast<uint32_t*>(s_bh + off) = pack(h[0], h[1]);
      *reinterpret_cast<uint32_t*>(s_bl + off) = pack(l[0], l[1]);
    }
  };

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  fetch(m_beg);
  for (int m0 = m_beg; m0 < m_end; m0 += HT_TILE) {      // the rows of the part, in order
    commit();
    __syncthreads();
    if (m0 + HT_TILE < m_end) fetch(m0 + HT_TILE);
    mma_tile(s_ah, s_al, s_bh, s_bl, wr, wc, lane, acc);
    __syncthreads();
  }

  const float inva = 1.f / sa, invb = 1.f / sb;
  float* out = g.out + (size_t)blockIdx.z * g.O * g.K;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int gi = i0 + wc * 32 + j * 16 + (lane & 15);
    if (gi >= g.K) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int go = o0 + wr * 32 + i * 16 + 4 * (lane >> 4) + e;
        if (go < g.O) out[(size_t)go * g.K + gi] = acc[i][j][e] * inva * invb;
      }
  }
}

// partial[p][c] = sum over the rows of part p of x[r][c], rows in a fixed order (4 row lanes, combined in lane order).
// Column sums accumulate in f64: under a shift-invariant loss (listMLE, neuralNDCG) the output bias's gradient is the sum of
// dLoss/dscore, which cancels to the rounding residue of its terms - an f32 sum would return its own rounding instead.
__global__ void __launch_bounds__(HT_THREADS) ht_colsum_kernel(const float* __restrict__ x, int M, int C, double* __restrict__ partial) {
  __shared__ double sm[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
  const int beg = blockIdx.y * HT_CS_PART, end = min(M, beg + HT_CS_PART);
  double s = 0.0;
  if (col < C)
    for (int r = beg + rl; r < end; r += 4) s += (double)x[(size_t)r * C + col];
  sm[rl][threadIdx.x & 63] = s;
  __syncthreads();
  if (rl == 0 && col < C) partial[(size_t)blockIdx.y * C + col] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}

// the same for d gamma = sum_rows g (x - mean) rstd, x rebuilt from the first layer's source
template <typename T>
__global__ void __launch_bounds__(HT_THREADS) ht_lnw_kernel(XSrc s, const float* __restrict__ gr, int M, double* __restrict__ partial) {
  __shared__ double sm[4][64];
  const int C = s.K;
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
  const int beg = blockIdx.y * HT_CS_PART, end = min(M, beg + HT_CS_PART);
  double acc = 0.0;
  if (col < C)
    for (int r = beg + rl; r < end; r += 4) {
      const size_t row = s.row_index ? (size_t)s.row_index[r] : (size_t)r;
      float x = widen<T>(reinterpret_cast<const T*>(s.x)[row * C + col]);
      if (s.res) x = round_to<T>(x + widen<T>(reinterpret_cast<const T*>(s.res)[row * C + col]));
      acc += (double)(gr[(size_t)r * C + col] * ((x - s.stats[2 * (size_t)r]) * s.stats[2 * (size_t)r + 1]));
    }
  sm[rl][threadIdx.x & 63] = acc;
  __syncthreads();
  if (rl == 0 && col < C) partial[(size_t)blockIdx.y * C + col] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}

// out[c] = sum_p partial[p][c] in part order, rounded once to f32
__global__ void __launch_bounds__(HT_THREADS) ht_colparts_sum_kernel(const double* __restrict__ partial, int parts, int C, float* __restrict__ out) {
  const int c = blockIdx.x * HT_THREADS + threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (int p = 0; p < parts; ++p) s += partial[(size_t)p * C + c];
  out[c] = (float)s;
}

// out[c] = sum_j W[j][c] v[j] in f64, j in order.  The encoder's final norm feeds the output layer linearly, so its d b_2 =
// sum_rows dZ_o W_o is W_o^T applied to the output bias's gradient, whose f64 column sum keeps what a shift-invariant loss
// leaves of it; the column sum of the rounded rows dZ_o W_o would return their rounding instead (see ht_colsum_kernel)
__global__ void __launch_bounds__(HT_THREADS) ht_matvec_t_kernel(const float* __restrict__ W, const float* __restrict__ v, int O, int K,
                                                               float* __restrict__ out) {
  const int c = blockIdx.x * HT_THREADS + threadIdx.x;
  if (c >= K) return;
  double s = 0.0;
  for (int j = 0; j < O; ++j) s += (double)W[(size_t)j * K + c] * (double)v[j];
  out[c] = (float)s;
}

// out[i] = sum_p partial[p][i] in part order (the weight-gradient parts of a narrow layer)
__global__ void __launch_bounds__(HT_THREADS) ht_parts_sum_kernel(const float* __restrict__ partial, int parts, size_t n, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * HT_THREADS + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int p = 0; p < parts; ++p) s += partial[(size_t)p * n + i];
  out[i] = s;
}

// OutputLayer.score: the sum over d_output in index order
__global__ void __launch_bounds__(HT_THREADS) ht_score_kernel(const float* __restrict__ a, int M, int O, float* __restrict__ scores,
                                                            float* __restrict__ scores_out) {
  const int r = blockIdx.x * HT_THREADS + threadIdx.x;
  if (r >= M) return;
  float s = 0.f;
  for (int j = 0; j < O; ++j) s += a[(size_t)r * O + j];
  scores[r] = s;
  if (scores_out) scores_out[r] = s;
}

// dZ_o[r][j] = dscore[r] act'(Z_o[r][j])
__global__ void __launch_bounds__(HT_THREADS) ht_out_grad_kernel(const float* __restrict__ dscore, const float* __restrict__ z, size_t n,
                                                               int O, int act, float* __restrict__ dz) {
  const size_t i = (size_t)blockIdx.x * HT_THREADS + threadIdx.x;
  if (i < n) dz[i] = dscore[i / O] * act_grad(z[i], act);
}

// torch MSELoss: mean over all n scores, nothing masked; single workgroup, fixed order
__global__ void __launch_bounds__(HT_THREADS) ht_mse_kernel(const float* __restrict__ o, const float* __restrict__ y, int n,
                                                          float* __restrict__ loss, float* __restrict__ dl) {
  __shared__ float red[HT_THREADS];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += HT_THREADS) { const float d = o[i] - y[i]; s += d * d; dl[i] = 2.f * d / (float)n; }
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) { float t = 0.f; for (int k = 0; k < HT_THREADS; ++k) t += red[k]; *loss = t / (float)n; }
}

// clip_grad_norm_, stage 1: the sum of squares of the b-th of HT_SQ_NB equal chunks of the gradient buffer (pads are 0)
__global__ void __launch_bounds__(HT_THREADS) ht_sumsq_kernel(const float* __restrict__ gbuf, size_t n, float* __restrict__ part) {
  __shared__ float sm[4];
  const size_t chunk = (n + HT_SQ_NB - 1) / HT_SQ_NB;
  const size_t beg = (size_t)blockIdx.x * chunk, end = beg + chunk < n ? beg + chunk : n;
  float s = 0.f;
  for (size_t i = beg + threadIdx.x; i < end; i += HT_THREADS) { const float v = gbuf[i]; s += v * v; }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((sm[0] + sm[1]) + sm[2]) + sm[3];
}
// stage 2: slots[0] = norm, slots[1] = min(1, clip / (norm + 1e-6)) (1 when clipping is off)
__global__ void __launch_bounds__(64) ht_norm_kernel(const float* __restrict__ part, float clip, float* __restrict__ slots,
                                                     float* __restrict__ norm_out) {
  if (threadIdx.x != 0) return;
  float s = 0.f;
  for (int i = 0; i < HT_SQ_NB; ++i) s += part[i];
  const float norm = sqrtf(s);
  slots[0] = norm;
  slots[1] = clip > 0.f ? fminf(1.f, clip / (norm + 1e-6f)) : 1.f;
  if (norm_out) *norm_out = norm;
}
__global__ void __launch_bounds__(HT_THREADS) ht_scale_kernel(float* __restrict__ gbuf, size_t n, const float* __restrict__ coef) {
  const size_t i = (size_t)blockIdx.x * HT_THREADS + threadIdx.x;
  if (i < n) gbuf[i] *= *coef;
}
__global__ void __launch_bounds__(HT_THREADS) ht_zero_kernel(float* __restrict__ p, size_t n) {
  const size_t i = (size_t)blockIdx.x * HT_THREADS + threadIdx.x;
  if (i < n) p[i] = 0.f;
}

// torch.optim.Adam with L2 decay and bias correction (the formula of adam_kernel, ltr_trainer.hip)
struct AdamArgs { float lr, b1, b2, eps, wd, bc1, bc2; };
__device__ __forceinline__ float adam_update(float* p, const float* g, float* m, float* v, size_t i, const AdamArgs& h) {
  const float pi = p[i];
  const float gi = g[i] + h.wd * pi;
  const float mi = h.b1 * m[i] + (1.f - h.b1) * gi;
  const float vi = h.b2 * v[i] + (1.f - h.b2) * gi * gi;
  m[i] = mi; v[i] = vi;
  const float pn = pi - h.lr * (mi / h.bc1) / (sqrtf(vi) / sqrtf(h.bc2) + h.eps);
  p[i] = pn;
  return pn;
}
__global__ void __launch_bounds__(HT_THREADS) ht_adam_vec_kernel(float* p, const float* g, float* m, float* v, size_t n, AdamArgs h) {
  const size_t i = (size_t)blockIdx.x * HT_THREADS + threadIdx.x;
  if (i < n) adam_update(p, g, m, v, i, h);
}

// A workgroup owns the 64 x 64 tile (o0, k0) of W [O, K]: Adam on its elements (update != 0), then the tile of the image
// [ceil64(O)][ceil64(K)] (hi | lo planes of W * scale, zeros outside W) and, transposed through LDS, of the image of W^T.
// The scale comes from max|W| taken BEFORE the update (wamax): one step moves a weight by ~lr, far inside fp16's range.
__global__ void __launch_bounds__(HT_THREADS) ht_adam_tile_kernel(float* P, const float* G, float* M1, float* V1, int O, int K,
                                                                AdamArgs h, int update, const float* __restrict__ wamax,
                                                                __half* __restrict__ img, __half* __restrict__ imgT) {
  __shared__ __attribute__((aligned(16))) __half t_hi[HT_PLANE];
  __shared__ __attribute__((aligned(16))) __half t_lo[HT_PLANE];
  const int tid = threadIdx.x;
  const int Op = (int)gridDim.y * HT_TILE, Kp = (int)gridDim.x * HT_TILE;
  const int k0 = blockIdx.x * HT_TILE, o0 = blockIdx.y * HT_TILE;
  const int lrow = tid >> 2, lk = (tid & 3) * 16;
  const float sc = tensor_scale(wamax);
  const int o = o0 + lrow;
  f16x8 hi[2], lo[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int k = k0 + lk + i;
    float w = 0.f;
    if (o < O && k < K) {
      const size_t idx = (size_t)o * K + k;
      w = update ? adam_update(P, G, M1, V1, idx, h) : P[idx];
    }
    __half hh, ll;
    split_f16(w * sc, hh, ll);
    hi[i >> 3][i & 7] = __builtin_bit_cast(_Float16, hh);
    lo[i >> 3][i & 7] = __builtin_bit_cast(_Float16, ll);
  }
  const size_t plane = (size_t)Op * Kp;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    *reinterpret_cast<f16x8*>(img + (size_t)o * Kp + k0 + lk + 8 * i) = hi[i];
    *reinterpret_cast<f16x8*>(img + plane + (size_t)o * Kp + k0 + lk + 8 * i) = lo[i];
    *reinterpret_cast<f16x8*>(t_hi + lrow * HT_LD + lk + 8 * i) = hi[i];
    *reinterpret_cast<f16x8*>(t_lo + lrow * HT_LD + lk + 8 * i) = lo[i];
  }
  __syncthreads();
  // transposed role: thread -> (k row tid / 4, 16 consecutive o)
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    hi[i >> 3][i & 7] = __builtin_bit_cast(_Float16, t_hi[(lk + i) * HT_LD + lrow]);
    lo[i >> 3][i & 7] = __builtin_bit_cast(_Float16, t_lo[(lk + i) * HT_LD + lrow]);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    *reinterpret_cast<f16x8*>(imgT + (size_t)(k0 + lrow) * Op + o0 + lk + 8 * i) = hi[i];
    *reinterpret_cast<f16x8*>(imgT + plane + (size_t)(k0 + lrow) * Op + o0 + lk + 8 * i) = lo[i];
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct DevGuard {
  int prev = -1; bool sw = false;
  explicit DevGuard(int dev) { if (hipGetDevice(&prev) == hipSuccess && prev != dev) sw = hipSetDevice(dev) == hipSuccess; }
  ~DevGuard() { if (sw) (void)hipSetDevice(prev); }
};

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }
inline int ceil64(int n) { return (n + 63) / 64 * 64; }
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline unsigned blocks(size_t n) { return (unsigned)((n + HT_THREADS - 1) / HT_THREADS); }

}  // namespace
}  // namespace ltr

using namespace ltr;

struct ltr_head_trainer {
  ltr_head_desc d;
  ltr_head_train_config cfg;
  int device = 0;
  int n = 0;                          // dense layers including the output layer
  ltr_head_encoder_desc enc{};        // n_blocks == 0: no encoder
  int dm = 0;                         // d_model: the output layer's input width
  int nm = 0;                         // matrices: the n dense layers, then QKV, W_o, w_1, w_2 of every encoder block
  int in[HT_MAX_MATS], out[HT_MAX_MATS];
  int mt[HT_MAX_MATS];                // tensor index of a matrix; its bias follows it
  std::vector<size_t> off, cnt;       // tensor index space of the create call: ln_w, ln_b, (W, b) per layer, then the encoder's
  std::vector<int> mat_of;            // matrix of a tensor, or -1
  size_t total = 0;
  float *P = nullptr, *G = nullptr, *M1 = nullptr, *V1 = nullptr;
  __half* img[HT_MAX_MATS] = {};      // hi | lo planes of W  [ceil64(out)][ceil64(in)]
  __half* imgT[HT_MAX_MATS] = {};     // hi | lo planes of W^T [ceil64(in)][ceil64(out)]
  float* wamax = nullptr;             // [nm][HT_AMAX_NB] first-stage maxima the images were scaled by
  long adam_step = 0;
  int enc_tensor(int b, int i) const { return 2 + 2 * n + HT_ENC_PER_BLOCK * b + i; }   // b == n_blocks: the final norm
  ~ltr_head_trainer() {
    (void)hipFree(P); (void)hipFree(G); (void)hipFree(M1); (void)hipFree(V1); (void)hipFree(wamax);
    for (int i = 0; i < HT_MAX_MATS; ++i) { (void)hipFree(img[i]); (void)hipFree(imgT[i]); }
  }
};

namespace ltr {
namespace {

int dw_parts(const ltr_head_trainer* t, int l, int M) {
  const int tiles = (t->out[l] + 63) / 64 * ((t->in[l] + 63) / 64);
  return tiles >= HT_DW_WIDE ? 1 : (M + HT_DW_PART - 1) / HT_DW_PART;
}

struct EncWs { float *qkv, *att, *lse, *zmid, *st1, *Z1, *A1; };     // what a block's backward reads again
struct HtWs {
  float *stats, *rowmax, *scores, *dscore, *row_loss, *amax, *dw_part, *sq_part, *slots;
  double* cs_part;
  float *Z[HT_MAX_LAYERS], *A[HT_MAX_LAYERS], *dz[3];
  EncWs e[HT_ENC_BLOCKS];
  float *ez[HT_ENC_BLOCKS + 1], *est[HT_ENC_BLOCKS + 1];   // residual stream entering block b (b == n_blocks: leaving the last) and its row statistics
  float *etmp, *eD;                                        // a sublayer's branch output [M, d_model]; D of the attention backward [h, M]
  void* ndcg; size_t ndcg_bytes;
  size_t bytes;
};
HtWs carve(const ltr_head_trainer* t, int B, int S, void* base) {
  const size_t M = (size_t)B * S;
  char* p = (char*)base;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t q = o; o += up256(bytes); return (float*)(base ? p + q : nullptr); };
  HtWs w;
  w.stats = take(M * 2 * 4); w.rowmax = take(M * 4); w.scores = take(M * 4); w.dscore = take(M * 4);
  w.row_loss = take((size_t)std::max(B, 1) * 4);
  w.amax = take((size_t)(2 * t->nm + 2) * HT_AMAX_NB * 4);
  size_t maxw = t->d.input_norm ? t->d.n_features : 1, dwp = 1;
  for (int l = 0; l < t->nm; ++l) {
    if (l < t->n) { w.Z[l] = take(M * t->out[l] * 4); w.A[l] = take(M * t->out[l] * 4); }
    maxw = std::max<size_t>(maxw, t->out[l]);
    const int parts = dw_parts(t, l, (int)M);
    if (parts > 1) dwp = std::max(dwp, (size_t)parts * t->out[l] * t->in[l]);
  }
  const int nb = t->enc.n_blocks;
  const size_t dm = t->dm;
  if (nb) maxw = std::max(maxw, dm);
  for (int b = 0; b < nb; ++b) {
    EncWs& e = w.e[b];
    e.qkv = take(M * 3 * dm * 4); e.att = take(M * dm * 4); e.lse = take(M * t->enc.h * 4);
    e.zmid = take(M * dm * 4); e.st1 = take(M * 2 * 4);
    e.Z1 = take(M * t->enc.d_ff * 4); e.A1 = take(M * t->enc.d_ff * 4);
  }
  for (int b = 0; nb && b <= nb; ++b) {
    w.ez[b] = b == 0 && t->n > 1 ? w.A[t->n - 2] : take(M * dm * 4);
    w.est[b] = take(M * 2 * 4);
  }
  w.etmp = take(nb ? M * dm * 4 : 0); w.eD = take(nb ? M * t->enc.h * 4 : 0);
  w.dz[0] = take(M * maxw * 4); w.dz[1] = take(M * maxw * 4); w.dz[2] = take(nb ? M * maxw * 4 : 0);
  w.cs_part = (double*)take((M + HT_CS_PART - 1) / HT_CS_PART * maxw * 8);
  w.dw_part = take(dwp * 4);
  w.sq_part = take(HT_SQ_NB * 4);
  w.slots = take(64);
  w.ndcg_bytes = t->cfg.loss == LTR_LOSS_NEURALNDCG ? ltr_neuralndcg_workspace_bytes(B, S)
                 : t->cfg.loss == LTR_HEAD_LOSS_LAMBDA ? ltr_lambdaloss_workspace_bytes(B, S) : 0;
  w.ndcg = take(w.ndcg_bytes);
  w.bytes = o;
  return w;
}

template <typename T> constexpr int hid_of() { return sizeof(T) == 4 ? LTR_HID_F32 : std::is_same<T, __half>::value ? LTR_HID_F16 : LTR_HID_BF16; }

XSrc plain_src(const float* x, int K, const float* amax) {
  XSrc s{};
  s.x = x; s.amax = amax; s.K = K; s.vec = K % 16 == 0 && al16(x);
  return s;
}

// the matrix of layer l: max|W| (first stage), then Adam and / or the image refresh
int refresh_matrix(ltr_head_trainer* t, int l, const AdamArgs& a, int update, hipStream_t s) {
  const size_t off = t->off[t->mt[l]];
  float* am = t->wamax + (size_t)l * HT_AMAX_NB;
  ht_amax_kernel<<<HT_AMAX_NB, HT_THREADS, 0, s>>>(t->P + off, t->cnt[t->mt[l]], am);
  LTR_LAUNCH_CHECK();
  ht_adam_tile_kernel<<<dim3(ceil64(t->in[l]) / 64, ceil64(t->out[l]) / 64), HT_THREADS, 0, s>>>(
      t->P + off, t->G + off, t->M1 + off, t->V1 + off, t->out[l], t->in[l], a, update, am, t->img[l], t->imgT[l]);
  LTR_LAUNCH_CHECK();
  return LTR_OK;
}

template <typename T>
int run_step(ltr_head_trainer* t, XSrc x0, int B, int S, const float* y_true, const int32_t* shuffle, int apply_update,
             float* loss_out, float* scores_out, float* grad_norm_out, const HtWs& w, hipStream_t s) {
  const int M = B * S, n = t->n, nm = t->nm, nb = t->enc.n_blocks, dm = t->dm;
  const bool norm = t->d.input_norm != 0;
  float* am_x0 = w.amax;
  // first-stage maxima: of A[l] (dense layer l's output), for an encoder matrix of its own plain input; of dZ at matrix l's output
  auto am_A = [&](int l) { return w.amax + (size_t)(1 + l) * HT_AMAX_NB; };
  auto am_dz = [&](int l) { return w.amax + (size_t)(1 + nm + l) * HT_AMAX_NB; };
  float* am_do = w.amax + (size_t)(1 + 2 * nm) * HT_AMAX_NB;
  const unsigned mt = (unsigned)((M + 63) / 64), cparts = (unsigned)((M + HT_CS_PART - 1) / HT_CS_PART);
  const float* mask = t->cfg.loss == LTR_HEAD_LOSS_GIVEN ? nullptr : y_true;      // allRank's src_mask: y_true == pad_value
  int rc = LTR_OK;

  auto amax = [&](const float* x, size_t cnt, float* part) -> int {
    ht_amax_kernel<<<HT_AMAX_NB, HT_THREADS, 0, s>>>(x, cnt, part);
    LTR_LAUNCH_CHECK();
    return LTR_OK;
  };
  // Z = a W_l^T + b_l, A = act(Z); `first`: a is the call's rows (of T)
  auto forward = [&](int l, const XSrc& a, float* Z, float* A, int act, bool first) -> int {
    ImgArgs g{};
    g.a = a;
    g.img = t->img[l]; g.ld = ceil64(t->in[l]); g.plane = (size_t)ceil64(t->out[l]) * g.ld;
    g.img_amax = t->wamax + (size_t)l * HT_AMAX_NB;
    g.bias = t->P + t->off[t->mt[l] + 1];
    g.Z = Z; g.A = A;
    g.M = M; g.N = t->out[l]; g.K = t->in[l];
    g.act = act;
    g.mode = HT_MODE_FWD;
    const dim3 grid(mt, (unsigned)(ceil64(g.N) / 64));
    if (first) ht_gemm_img_kernel<T><<<grid, HT_THREADS, 0, s>>>(g);
    else ht_gemm_img_kernel<float><<<grid, HT_THREADS, 0, s>>>(g);
    LTR_LAUNCH_CHECK();
    return LTR_OK;
  };
  // a row-major f32 tensor under allRank's LayerNorm, applied on load from the statistics of enc_rows_kernel
  auto normed = [&](const float* z, const float* stats, int tensor) {
    XSrc a = plain_src(z, dm, nullptr);
    a.stats = stats; a.ln_w = t->P + t->off[tensor]; a.ln_b = t->P + t->off[tensor + 1];
    return a;
  };

  // ---- forward
  x0.stats = w.stats;
  ht_rows_kernel<T><<<(M + 3) / 4, HT_THREADS, 0, s>>>(x0, M, w.stats, w.rowmax);
  LTR_LAUNCH_CHECK();
  if (!norm) {
    if ((rc = amax(w.rowmax, (size_t)M, am_x0))) return rc;
    x0.amax = am_x0;
  }
  auto dense_src = [&](int l) { return l == 0 ? x0 : plain_src(w.A[l - 1], t->in[l], am_A(l - 1)); };
  for (int l = 0; l < (nb ? n - 1 : n); ++l) {
    if ((rc = forward(l, dense_src(l), w.Z[l], w.A[l], l == n - 1 ? t->d.output_activation : t->d.activation, l == 0))) return rc;
    if (l < n - 1 && (rc = amax(w.A[l], (size_t)M * t->out[l], am_A(l)))) return rc;
  }
  if (nb) {       // Encoder.forward (transformer.py:44-72): per block z += W_o MHA(norm(z)); z += w_2 relu(w_1 norm(z)); then norm
    if (n == 1 && (rc = launch_enc_gather(x0.x, x0.res, hid_of<T>(), x0.row_index, M, dm, w.ez[0], s))) return rc;
    if ((rc = launch_enc_rows(w.ez[0], nullptr, nullptr, M, dm, w.est[0], s))) return rc;
    for (int b = 0; b < nb; ++b) {
      const EncWs& e = w.e[b];
      const int m0 = n + 4 * b;
      if ((rc = forward(m0, normed(w.ez[b], w.est[b], t->enc_tensor(b, 0)), e.qkv, e.qkv, ACT_NONE, false))) return rc;
      if ((rc = launch_enc_attn_fwd(e.qkv, mask, t->cfg.pad_value, B, S, dm, t->enc.h, e.att, e.lse, s))) return rc;
      if ((rc = amax(e.att, (size_t)M * dm, am_A(m0 + 1)))) return rc;
      if ((rc = forward(m0 + 1, plain_src(e.att, dm, am_A(m0 + 1)), w.etmp, w.etmp, ACT_NONE, false))) return rc;
      if ((rc = launch_enc_rows(w.ez[b], w.etmp, e.zmid, M, dm, e.st1, s))) return rc;
      if ((rc = forward(m0 + 2, normed(e.zmid, e.st1, t->enc_tensor(b, 6)), e.Z1, e.A1, ACT_RELU, false))) return rc;
      if ((rc = amax(e.A1, (size_t)M * t->enc.d_ff, am_A(m0 + 3)))) return rc;
      if ((rc = forward(m0 + 3, plain_src(e.A1, t->enc.d_ff, am_A(m0 + 3)), w.etmp, w.etmp, ACT_NONE, false))) return rc;
      if ((rc = launch_enc_rows(e.zmid, w.etmp, w.ez[b + 1], M, dm, w.est[b + 1], s))) return rc;
    }
    if ((rc = forward(n - 1, normed(w.ez[nb], w.est[nb], t->enc_tensor(nb, 0)), w.Z[n - 1], w.A[n - 1], t->d.output_activation, false))) return rc;
  }
  const int dout = t->out[n - 1];
  ht_score_kernel<<<blocks(M), HT_THREADS, 0, s>>>(w.A[n - 1], M, dout, w.scores, scores_out);
  LTR_LAUNCH_CHECK();

  // ---- loss on the [B, S] scores -> dLoss / dscore
  const float* dscore = w.dscore;
  switch (t->cfg.loss) {
    case LTR_LOSS_LISTMLE:
      rc = ltr_listmle(w.scores, y_true, shuffle, B, S, t->cfg.listmle_eps, t->cfg.pad_value, loss_out, w.row_loss, w.dscore, s);
      break;
    case LTR_LOSS_NEURALNDCG:
      rc = ltr_neuralndcg(w.scores, y_true, B, S, 1.f, 0, t->cfg.pad_value, loss_out, w.row_loss, w.dscore, w.ndcg, w.ndcg_bytes, s);
      break;
    case LTR_HEAD_LOSS_LAMBDA:
      rc = ltr_lambdaloss(w.scores, y_true, B, S, &t->cfg.lambda, loss_out, w.dscore, w.ndcg, w.ndcg_bytes, s);
      break;
    case LTR_LOSS_MSE:
      ht_mse_kernel<<<1, HT_THREADS, 0, s>>>(w.scores, y_true, M, loss_out, w.dscore);
      LTR_LAUNCH_CHECK();
      break;
    default: dscore = y_true;     // LTR_HEAD_LOSS_GIVEN
  }
  if (rc) return rc;

  // ---- backward
  ht_out_grad_kernel<<<blocks((size_t)M * dout), HT_THREADS, 0, s>>>(dscore, w.Z[n - 1], (size_t)M * dout, dout,
                                                                    t->d.output_activation, w.dz[(n - 1) & 1]);
  LTR_LAUNCH_CHECK();
  // the bias and weight gradients of matrix l from dZ [M, out] at its output and from its input
  auto param_grads = [&](int l, const float* dz, const XSrc& in, bool first) -> int {
    const int O = t->out[l], K = t->in[l];
    float* gw = t->G + t->off[t->mt[l]];
    ht_amax_kernel<<<HT_AMAX_NB, HT_THREADS, 0, s>>>(dz, (size_t)M * O, am_dz(l));
    LTR_LAUNCH_CHECK();
    ht_colsum_kernel<<<dim3((unsigned)((O + 63) / 64), cparts), HT_THREADS, 0, s>>>(dz, M, O, w.cs_part);
    LTR_LAUNCH_CHECK();
    ht_colparts_sum_kernel<<<blocks(O), HT_THREADS, 0, s>>>(w.cs_part, (int)cparts, O, t->G + t->off[t->mt[l] + 1]);
    LTR_LAUNCH_CHECK();
    const int parts = dw_parts(t, l, M);
    DwArgs dw{};
    dw.a = plain_src(dz, O, am_dz(l));
    dw.b = in;
    dw.out = parts > 1 ? w.dw_part : gw;
    dw.M = M; dw.O = O; dw.K = K; dw.part_rows = parts > 1 ? HT_DW_PART : M;
    const dim3 grid((unsigned)((O + 63) / 64), (unsigned)((K + 63) / 64), (unsigned)parts);
    if (first) ht_gemm_dw_kernel<T><<<grid, HT_THREADS, 0, s>>>(dw);
    else ht_gemm_dw_kernel<float><<<grid, HT_THREADS, 0, s>>>(dw);
    LTR_LAUNCH_CHECK();
    if (parts > 1) {
      ht_parts_sum_kernel<<<blocks((size_t)O * K), HT_THREADS, 0, s>>>(w.dw_part, parts, (size_t)O * K, gw);
      LTR_LAUNCH_CHECK();
    }
    return LTR_OK;
  };
  // out = dZ W_l, times act'(Zprev) where Zprev is given; after param_grads(l, dz)
  auto input_grad = [&](int l, const float* dz, const float* Zprev, int act, float* out) -> int {
    const int O = t->out[l], K = t->in[l];
    ImgArgs g{};
    g.a = plain_src(dz, O, am_dz(l));
    g.img = t->imgT[l]; g.ld = ceil64(O); g.plane = (size_t)ceil64(K) * g.ld;
    g.img_amax = t->wamax + (size_t)l * HT_AMAX_NB;
    g.Zprev = Zprev;
    g.out = out;
    g.M = M; g.N = K; g.K = O; g.act = act; g.mode = HT_MODE_DX;
    ht_gemm_img_kernel<float><<<dim3(mt, (unsigned)(ceil64(K) / 64)), HT_THREADS, 0, s>>>(g);
    LTR_LAUNCH_CHECK();
    return LTR_OK;
  };
  // a LayerNorm's d beta = column sums of g and d gamma = column sums of g * xhat, g the gradient at its output
  auto norm_grads = [&](const XSrc& in, const float* g, int tensor, bool first) -> int {
    const int K = in.K;
    const dim3 cg((unsigned)((K + 63) / 64), cparts);
    if (tensor == t->enc_tensor(nb, 0) && nb) {      // the encoder's final norm
      const int ot = t->mt[n - 1];
      ht_matvec_t_kernel<<<blocks(K), HT_THREADS, 0, s>>>(t->P + t->off[ot], t->G + t->off[ot + 1], dout, K, t->G + t->off[tensor + 1]);
    } else {
      ht_colsum_kernel<<<cg, HT_THREADS, 0, s>>>(g, M, K, w.cs_part);
      LTR_LAUNCH_CHECK();
      ht_colparts_sum_kernel<<<blocks(K), HT_THREADS, 0, s>>>(w.cs_part, (int)cparts, K, t->G + t->off[tensor + 1]);
    }
    LTR_LAUNCH_CHECK();
    if (first) ht_lnw_kernel<T><<<cg, HT_THREADS, 0, s>>>(in, g, M, w.cs_part);
    else ht_lnw_kernel<float><<<cg, HT_THREADS, 0, s>>>(in, g, M, w.cs_part);
    LTR_LAUNCH_CHECK();
    ht_colparts_sum_kernel<<<blocks(K), HT_THREADS, 0, s>>>(w.cs_part, (int)cparts, K, t->G + t->off[tensor]);
    LTR_LAUNCH_CHECK();
    return LTR_OK;
  };

  if (nb) {
    // the output layer reads norm(z); R = dz[2] carries the gradient at the residual stream down the blocks, dz[0] and dz[1]
    // hold in turn dZ_1 / dO / the gradient at a norm's output and dQ|dK|dV
    float *R = w.dz[2], *t0 = w.dz[0], *t1 = w.dz[1];
    const float* dzo = w.dz[(n - 1) & 1];
    float* dy = w.dz[n & 1];
    XSrc in = normed(w.ez[nb], w.est[nb], t->enc_tensor(nb, 0));
    if ((rc = param_grads(n - 1, dzo, in, false))) return rc;
    if ((rc = input_grad(n - 1, dzo, nullptr, ACT_NONE, dy))) return rc;
    if ((rc = norm_grads(in, dy, t->enc_tensor(nb, 0), false))) return rc;
    if ((rc = launch_enc_ln_bwd(w.ez[nb], w.est[nb], in.ln_w, dy, nullptr, R, M, dm, s))) return rc;
    for (int b = nb - 1; b >= 0; --b) {
      const EncWs& e = w.e[b];
      const int m0 = n + 4 * b;
      // z_out = z_mid + w_2 relu(w_1 norm(z_mid))
      if ((rc = param_grads(m0 + 3, R, plain_src(e.A1, t->enc.d_ff, am_A(m0 + 3)), false))) return rc;
      if ((rc = input_grad(m0 + 3, R, e.Z1, ACT_RELU, t0))) return rc;
      in = normed(e.zmid, e.st1, t->enc_tensor(b, 6));
      if ((rc = param_grads(m0 + 2, t0, in, false))) return rc;
      if ((rc = input_grad(m0 + 2, t0, nullptr, ACT_NONE, t1))) return rc;
      if ((rc = norm_grads(in, t1, t->enc_tensor(b, 6), false))) return rc;
      if ((rc = launch_enc_ln_bwd(e.zmid, e.st1, in.ln_w, t1, R, R, M, dm, s))) return rc;
      // z_mid = z + W_o MHA(norm(z))
      if ((rc = param_grads(m0 + 1, R, plain_src(e.att, dm, am_A(m0 + 1)), false))) return rc;
      if ((rc = input_grad(m0 + 1, R, nullptr, ACT_NONE, t0))) return rc;
      if ((rc = amax(t0, (size_t)M * dm, am_do))) return rc;
      if ((rc = launch_enc_attn_bwd(e.qkv, t0, e.lse, am_do, mask, t->cfg.pad_value, B, S, dm, t->enc.h, w.eD, t1, s))) return rc;
      in = normed(w.ez[b], w.est[b], t->enc_tensor(b, 0));
      if ((rc = param_grads(m0, t1, in, false))) return rc;
      if ((rc = input_grad(m0, t1, nullptr, ACT_NONE, t0))) return rc;
      if ((rc = norm_grads(in, t0, t->enc_tensor(b, 0), false))) return rc;
      if ((rc = launch_enc_ln_bwd(w.ez[b], w.est[b], in.ln_w, t0, R, R, M, dm, s))) return rc;
    }
    if (n > 1) {      // R is the gradient at A_{n-2}: dZ_{n-2} = R act'(Z_{n-2})
      ht_out_grad_kernel<<<blocks((size_t)M * dm), HT_THREADS, 0, s>>>(R, w.Z[n - 2], (size_t)M * dm, 1, t->d.activation, w.dz[(n - 2) & 1]);
      LTR_LAUNCH_CHECK();
    }
  }
  for (int l = nb ? n - 2 : n - 1; l >= 0; --l) {
    float* dz = w.dz[l & 1];
    if ((rc = param_grads(l, dz, dense_src(l), l == 0))) return rc;
    if (l == 0 && !norm) break;
    // dA_{l-1} = dZ_l W_l, times act'(Z_{l-1}); layer 0: the gradient at the LayerNorm output
    if ((rc = input_grad(l, dz, l > 0 ? w.Z[l - 1] : nullptr, t->d.activation, w.dz[(l + 1) & 1]))) return rc;
    if (l == 0 && (rc = norm_grads(x0, w.dz[1], 0, true))) return rc;
  }

  // ---- clip_grad_norm_ (train_utils.py:40-41)
  ht_sumsq_kernel<<<HT_SQ_NB, HT_THREADS, 0, s>>>(t->G, t->total, w.sq_part);
  LTR_LAUNCH_CHECK();
  ht_norm_kernel<<<1, 64, 0, s>>>(w.sq_part, t->cfg.clip_norm, w.slots, grad_norm_out);
  LTR_LAUNCH_CHECK();
  if (t->cfg.clip_norm > 0.f) {
    ht_scale_kernel<<<blocks(t->total), HT_THREADS, 0, s>>>(t->G, t->total, w.slots + 1);
    LTR_LAUNCH_CHECK();
  }
  if (!apply_update) return LTR_OK;

  // ---- opt.step(): torch.optim.Adam; a gradient-only call advances neither the moments nor t
  t->adam_step += 1;
  const double b1 = t->cfg.beta1, b2 = t->cfg.beta2;
  const AdamArgs a{t->cfg.lr, t->cfg.beta1, t->cfg.beta2, t->cfg.eps, t->cfg.weight_decay,
                   (float)(1.0 - std::pow(b1, (double)t->adam_step)), (float)(1.0 - std::pow(b2, (double)t->adam_step))};
  for (size_t i = 0; i < t->cnt.size(); ++i) {
    if (!t->cnt[i]) continue;
    if (t->mat_of[i] >= 0) { if ((rc = refresh_matrix(t, t->mat_of[i], a, 1, s))) return rc; continue; }
    const size_t o = t->off[i];
    ht_adam_vec_kernel<<<blocks(t->cnt[i]), HT_THREADS, 0, s>>>(t->P + o, t->G + o, t->M1 + o, t->V1 + o, t->cnt[i], a);
    LTR_LAUNCH_CHECK();
  }
  return LTR_OK;
}

}  // namespace
}  // namespace ltr

extern "C" {

// both create calls; enc == nullptr: no encoder
static int create_trainer(const ltr_head_desc* d, const ltr_head_encoder_desc* enc, const void* const* weights, int32_t n_weights,
                          const ltr_head_train_config* cfg, void* stream, ltr_head_train_handle* out) {
  if (!d || !weights || !cfg || !out) { set_error("ltr_head_train_create: NULL argument"); return LTR_E_INVAL; }
  if (d->n_fc < 0 || d->n_fc > 8 || d->n_features < 1 || d->n_features > 8192 || d->d_output < 1 || d->d_output > 8192) {
    set_error("ltr_head_train_create: bad shape (n_fc=%d n_features=%d d_output=%d)", d->n_fc, d->n_features, d->d_output);
    return LTR_E_INVAL;
  }
  if (d->weight_dtype != LTR_W_F32) { set_error("ltr_head_train_create: the master weights are f32 (weight_dtype must be LTR_W_F32)"); return LTR_E_INVAL; }
  if (d->activation < LTR_ACT_NONE || d->activation > LTR_ACT_SILU || d->output_activation < LTR_ACT_NONE || d->output_activation > LTR_ACT_SILU) {
    set_error("ltr_head_train_create: unknown activation"); return LTR_E_INVAL;
  }
  if (cfg->loss != LTR_LOSS_LISTMLE && cfg->loss != LTR_LOSS_MSE && cfg->loss != LTR_LOSS_NEURALNDCG && cfg->loss != LTR_HEAD_LOSS_GIVEN &&
      cfg->loss != LTR_HEAD_LOSS_LAMBDA) {
    set_error("ltr_head_train_create: loss %d is not listMLE, MSE, neuralNDCG, LTR_HEAD_LOSS_GIVEN or LTR_HEAD_LOSS_LAMBDA", cfg->loss); return LTR_E_INVAL;
  }
  if (cfg->loss == LTR_HEAD_LOSS_LAMBDA) {         // the checks of ltr_lambdaloss, made once (an empty slate touches nothing)
    const int rc = ltr_lambdaloss(nullptr, nullptr, 0, 0, &cfg->lambda, nullptr, nullptr, nullptr, 0, nullptr);
    if (rc) return rc;
  }
  const int dm = d->n_fc ? d->fc_sizes[d->n_fc - 1] : d->n_features, n_head = 2 + 2 * (d->n_fc + 1);
  if (enc) {      // the checks of ltr_head_encoder_create
    if (enc->positional_encoding != 0) { set_error("ltr_head_train_create_encoder: positional_encoding is not built"); return LTR_E_INVAL; }
    if (enc->n_blocks < 1 || enc->n_blocks > HT_ENC_BLOCKS || enc->d_ff < 1 || enc->d_ff > 65536 || enc->h < 1) {
      set_error("ltr_head_train_create_encoder: bad shape (N=%d d_ff=%d h=%d)", enc->n_blocks, enc->d_ff, enc->h); return LTR_E_INVAL;
    }
    if (dm < 2 || dm % enc->h != 0 || dm / enc->h % 16 != 0 || dm / enc->h > 128) {
      set_error("ltr_head_train_create_encoder: d_model = %d, h = %d: d_k must be a multiple of 16 up to 128", dm, enc->h); return LTR_E_INVAL;
    }
    if (d->n_fc == 0 && d->input_norm) { set_error("ltr_head_train_create_encoder: an input norm needs an FC layer"); return LTR_E_INVAL; }
  }
  const int want = n_head + (enc ? HT_ENC_PER_BLOCK * enc->n_blocks + 2 : 0);
  if (n_weights != want) { set_error("ltr_head_train_create: %d weight pointers, expected %d", n_weights, want); return LTR_E_INVAL; }
  for (int i = 0; i < d->n_fc; ++i)
    if (d->fc_sizes[i] < 1 || d->fc_sizes[i] > 8192) { set_error("ltr_head_train_create: layer %d: bad size %d", i, d->fc_sizes[i]); return LTR_E_INVAL; }
  for (int i = d->input_norm ? 0 : 2; i < want; ++i)
    if (!weights[i]) { set_error("ltr_head_train_create: weight pointer %d is NULL", i); return LTR_E_INVAL; }
  ltr_head_trainer* t = new (std::nothrow) ltr_head_trainer();
  if (!t) { set_error("ltr_head_train_create: out of host memory"); return LTR_E_NOMEM; }
  t->d = *d; t->cfg = *cfg; t->n = d->n_fc + 1;
  t->off.resize(want); t->cnt.resize(want);
  int in = d->n_features;
  t->cnt[0] = t->cnt[1] = d->input_norm ? (size_t)d->n_features : 0;
  for (int l = 0; l < t->n; ++l) {
    const int o = l < d->n_fc ? d->fc_sizes[l] : d->d_output;
    t->in[l] = in; t->out[l] = o;
    t->cnt[2 + 2 * l] = (size_t)o * in; t->cnt[3 + 2 * l] = (size_t)o;
    t->mt[l] = 2 + 2 * l;
    in = o;
  }
  t->nm = t->n; t->dm = dm;
  if (enc) {
    t->enc = *enc;
    const int io[4][2] = {{dm, 3 * dm}, {dm, dm}, {dm, enc->d_ff}, {enc->d_ff, dm}};      // QKV, W_o, w_1, w_2
    const int at[4] = {2, 4, 8, 10};
    for (int b = 0; b <= enc->n_blocks; ++b)
      for (int i = 0; i < (b < enc->n_blocks ? HT_ENC_PER_BLOCK : 2); ++i) t->cnt[t->enc_tensor(b, i)] = (size_t)dm;   // norms; the rest below
    for (int b = 0; b < enc->n_blocks; ++b)
      for (int i = 0; i < 4; ++i) {
        const int l = t->nm++, ti = t->enc_tensor(b, at[i]);
        t->in[l] = io[i][0]; t->out[l] = io[i][1]; t->mt[l] = ti;
        t->cnt[ti] = (size_t)io[i][0] * io[i][1]; t->cnt[ti + 1] = (size_t)io[i][1];
      }
  }
  t->mat_of.assign(want, -1);
  for (int l = 0; l < t->nm; ++l) t->mat_of[t->mt[l]] = l;
  size_t total = 0;
  for (int i = 0; i < want; ++i) { t->off[i] = total; total += (t->cnt[i] + 63) / 64 * 64; }
  t->total = total;
  {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, weights[2]) != hipSuccess) {
      (void)hipGetLastError(); delete t; set_error("ltr_head_train_create: weight pointers must be device memory"); return LTR_E_INVAL;
    }
    t->device = attr.device;
  }
  DevGuard guard(t->device);
  hipStream_t s = (hipStream_t)stream;
  bool ok = hipMalloc((void**)&t->P, total * 4) == hipSuccess && hipMalloc((void**)&t->G, total * 4) == hipSuccess &&
            hipMalloc((void**)&t->M1, total * 4) == hipSuccess && hipMalloc((void**)&t->V1, total * 4) == hipSuccess &&
            hipMalloc((void**)&t->wamax, (size_t)t->nm * HT_AMAX_NB * 4) == hipSuccess;
  for (int l = 0; ok && l < t->nm; ++l) {
    const size_t halves = (size_t)2 * ceil64(t->out[l]) * ceil64(t->in[l]);
    ok = hipMalloc((void**)&t->img[l], halves * 2) == hipSuccess && hipMalloc((void**)&t->imgT[l], halves * 2) == hipSuccess;
  }
  if (!ok) { (void)hipGetLastError(); delete t; set_error("ltr_head_train_create: cannot allocate %zu parameters x 4 buffers and the images", total); return LTR_E_NOMEM; }
  float* bufs[4] = {t->P, t->G, t->M1, t->V1};
  for (float* b : bufs) ht_zero_kernel<<<blocks(total), HT_THREADS, 0, s>>>(b, total);
  for (int i = 0; i < want; ++i)
    if (t->cnt[i] && hipMemcpyAsync(t->P + t->off[i], weights[i], t->cnt[i] * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) {
      delete t; set_error("ltr_head_train_create: copying weight %d failed", i); return LTR_E_HIP;
    }
  for (int l = 0; l < t->nm; ++l) {
    const int rc = refresh_matrix(t, l, AdamArgs{}, 0, s);
    if (rc) { delete t; return rc; }
  }
  if (hipStreamSynchronize(s) != hipSuccess) { delete t; set_error("ltr_head_train_create: building the images failed"); return LTR_E_HIP; }
  *out = t;
  return LTR_OK;
}

int ltr_head_train_create(const ltr_head_desc* d, const void* const* weights, int32_t n_weights,
                          const ltr_head_train_config* cfg, void* stream, ltr_head_train_handle* out) {
  return create_trainer(d, nullptr, weights, n_weights, cfg, stream, out);
}

int ltr_head_train_create_encoder(const ltr_head_desc* d, const ltr_head_encoder_desc* enc, const void* const* weights,
                                  int32_t n_weights, const ltr_head_train_config* cfg, void* stream, ltr_head_train_handle* out) {
  if (!enc) { set_error("ltr_head_train_create_encoder: NULL argument"); return LTR_E_INVAL; }
  return create_trainer(d, enc, weights, n_weights, cfg, stream, out);
}

int ltr_head_train_destroy(ltr_head_train_handle h) {
  if (h) { DevGuard guard(h->device); delete h; }
  return LTR_OK;
}

size_t ltr_head_train_workspace_bytes(ltr_head_train_handle h, int32_t B, int32_t S) {
  if (!h || B <= 0 || S <= 0 || (int64_t)B * S > HT_MAX_ROWS) return 0;
  return carve(h, B, S, nullptr).bytes;
}

int ltr_head_train_step(ltr_head_train_handle h, const void* hidden, const void* residual, int32_t hidden_dtype,
                        const int32_t* row_index, int32_t B, int32_t S, const float* y_true, const int32_t* shuffle,
                        int32_t apply_update, float* loss_out, float* scores_out, float* grad_norm_out, void* workspace,
                        size_t ws_bytes, void* stream) {
  if (!h) { set_error("ltr_head_train_step: NULL handle"); return LTR_E_INVAL; }
  if (B < 0 || S < 0 || (int64_t)B * S > HT_MAX_ROWS) { set_error("ltr_head_train_step: bad slate shape [%d, %d] (at most %d rows)", B, S, HT_MAX_ROWS); return LTR_E_INVAL; }
  if (hidden_dtype != LTR_HID_F32 && hidden_dtype != LTR_HID_F16 && hidden_dtype != LTR_HID_BF16) {
    set_error("ltr_head_train_step: bad hidden_dtype %d (LTR_HID_F32 | LTR_HID_F16 | LTR_HID_BF16)", hidden_dtype);
    return LTR_E_INVAL;
  }
  if (B * S == 0) return LTR_OK;
  if (h->enc.n_blocks && B > 65535) { set_error("ltr_head_train_step: the encoder takes at most 65535 slates (B = %d)", B); return LTR_E_INVAL; }
  const int loss = h->cfg.loss;
  if (!hidden || !y_true || !workspace || (loss != LTR_HEAD_LOSS_GIVEN && !loss_out)) { set_error("ltr_head_train_step: NULL argument"); return LTR_E_INVAL; }
  if (loss == LTR_LOSS_LISTMLE && (!shuffle || S > 4096)) { set_error("ltr_head_train_step: listMLE needs the shuffle permutation and S <= 4096"); return LTR_E_INVAL; }
  if (loss == LTR_HEAD_LOSS_LAMBDA && (S > 4096 || ltr_lambdaloss_workspace_bytes(B, S) == 0)) {
    set_error("ltr_head_train_step: LambdaLoss takes slates of at most 4096 items and 65535 slates ([%d, %d])", B, S); return LTR_E_INVAL;
  }
  if (loss == LTR_LOSS_NEURALNDCG && (S < 2 || S > 1024 || ltr_neuralndcg_workspace_bytes(B, S) == 0)) {
    set_error("ltr_head_train_step: neuralNDCG takes slates of 2..1024 items (S = %d)", S); return LTR_E_INVAL;
  }
  const HtWs w = carve(h, B, S, workspace);
  if (ws_bytes < w.bytes) { set_error("ltr_head_train_step: workspace of %zu bytes, %zu needed for [%d, %d]", ws_bytes, w.bytes, B, S); return LTR_E_NOMEM; }
  DevGuard guard(h->device);
  XSrc x0{};
  x0.x = hidden; x0.res = residual; x0.row_index = row_index;
  x0.ln_w = h->d.input_norm ? h->P + h->off[0] : nullptr;
  x0.ln_b = h->d.input_norm ? h->P + h->off[1] : nullptr;
  x0.K = h->d.n_features;
  x0.vec = x0.K % 16 == 0 && al16(hidden) && al16(residual);
  hipStream_t s = (hipStream_t)stream;
  if (hidden_dtype == LTR_HID_F32) return run_step<float>(h, x0, B, S, y_true, shuffle, apply_update, loss_out, scores_out, grad_norm_out, w, s);
  if (hidden_dtype == LTR_HID_F16) return run_step<__half>(h, x0, B, S, y_true, shuffle, apply_update, loss_out, scores_out, grad_norm_out, w, s);
  return run_step<bf16_t>(h, x0, B, S, y_true, shuffle, apply_update, loss_out, scores_out, grad_norm_out, w, s);
}

int ltr_head_train_read(ltr_head_train_handle h, int32_t index, int32_t what, float* dst, size_t capacity, size_t* count_out,
                        void* stream) {
  if (!h || index < 0 || index >= (int)h->off.size() || !count_out || (what != 0 && what != 1)) {
    set_error("ltr_head_train_read: bad argument"); return LTR_E_INVAL;
  }
  *count_out = h->cnt[index];
  if (!dst || h->cnt[index] == 0) return LTR_OK;           // size query / absent tensor
  if (capacity < h->cnt[index]) { set_error("ltr_head_train_read: %zu floats do not fit %zu", h->cnt[index], capacity); return LTR_E_NOMEM; }
  DevGuard guard(h->device);
  const float* src = (what == 0 ? h->P : h->G) + h->off[index];
  LTR_HIP_CHECK(hipMemcpyAsync(dst, src, h->cnt[index] * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return LTR_OK;
}

}  // extern "C"
