// Supervised criteria on [pixels][K] f32 logits (K = classes, 1..16) against int64 labels in [0, K):
//   KL_div(weight=w, reduction=mean | sum | none)(softmax(logits), one_hot(labels))   contrastyou/losses/kl.py:94-125
//   DiceLoss(ignore_index, smooth, p, reduction)(softmax(logits), one_hot(labels))    contrastyou/losses/dice_loss.py:46-105
// The family of cy_head_loss.hip / cy_pixel_reg.hip: every kernel reads its logits once, one thread per pixel,
// grid-stride, softmax in registers; sums leave a block as f64 partials and a one-block finalize launch adds them in a
// fixed order (no atomics: two runs give the same bits); every backward is one launch that recomputes the softmax.
// K = 2, 4, 8 are compiled with K known; any other K takes the run-time form.
//
// Weighted KL.  l_pix = -w[y] log((p_y + eps) / (1 + eps)); the other classes add exactly 0 (their target is 0).
//   dz_k = G w[y] (-p_y / (p_y + eps)) (delta_ky - p_k),  G = gscale / denom (scalar forms) or dmap[pix] (map forms).
//
// Soft Dice, per image n and class c:  A = sum_pix p_c [y = c],  B = sum_pix p_c^P,  T = #{pix: y = c} (t^P = t for a
// one-hot target),  num = A + smooth,  den = B + T + smooth,  L_nc = 1 - num / den (no factor 2: dice_loss.py:57-60).
//   loss = (1/K) sum_{c != ignore} red_n L_nc;  the divisor K counts the ignored class (dice_loss.py:105).
//   g_c = dloss/dp_c = (G_n r / K) (-[y = c] / den + num P p_c^(P-1) / den^2), 0 for c = ignore;  r = 1/N (mean) or 1;
//   dz_k = p_k (g_k - sum_j p_j g_j).
// A forward block never spans two images: the grid is N x blocks-per-image.
#include "cy_common.h"
#include "cy_pixel_loss.h"
#include "cy_reduce.h"

namespace {

enum { RED_MEAN = 0, RED_SUM = 1, RED_NONE = 2 };

inline bool bad_k(int K) { return K < 1 || K > KMAX; }

// the label's softmax entry and its class weight; a label outside [0, K) reads nothing and weighs 0
__device__ __forceinline__ void target_entry(const float* pr, const float* __restrict__ weight, long t, int K,
                                             float* pt, float* wt) {
  *pt = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K && k == t) *pt = pr[k];
  const bool in = t >= 0 && t < K;
  *wt = !in ? 0.f : (weight ? weight[t] : 1.f);
}

// ---------------------------------------------------------------- class-weighted softmax-KL
// MAP: the per-pixel value goes to map[pix]; otherwise one f64 partial per block
template <int KT, bool MAP>
__device__ __forceinline__ void wkl_fwd_body(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                             const float* __restrict__ weight, double* __restrict__ partial,
                                             float* __restrict__ map, long npix, int Krt, float eps) {
  const int K = KT ? KT : Krt;
  double acc = 0.0;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float z[KMAX], pr[KMAX], pt, wt;
    load_row<KT>(logits, p, K, z);
    softmax_k(z, pr, K);
    target_entry(pr, weight, (long)target[p], K, &pt, &wt);
    const float l = wt == 0.f ? 0.f : -wt * logf((pt + eps) / (1.f + eps));
    if constexpr (MAP)
      map[p] = l;
    else
      acc += (double)l;
  }
  if constexpr (!MAP) {
    __shared__ double sh[256];
    const double tot = block_sum_d(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
  }
}

template <int KT>
__global__ void __launch_bounds__(256)
    softmax_wkl_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                           const float* __restrict__ weight, double* __restrict__ partial, long npix, int Krt,
                           float eps) {
  wkl_fwd_body<KT, false>(logits, target, weight, partial, nullptr, npix, Krt, eps);
}

template <int KT>
__global__ void __launch_bounds__(256)
    softmax_wkl_map_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                               const float* __restrict__ weight, float* __restrict__ map, long npix, int Krt,
                               float eps) {
  wkl_fwd_body<KT, true>(logits, target, weight, nullptr, map, npix, Krt, eps);
}

// up: the device scalar gscale (MAP false; G = up[0] / denom) or the upstream map (MAP true; G = up[pix])
template <int KT, bool MAP>
__device__ __forceinline__ void wkl_bwd_body(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                             const float* __restrict__ weight, const float* __restrict__ up,
                                             float* __restrict__ dlogits, long npix, int Krt, float eps,
                                             double denom) {
  const int K = KT ? KT : Krt;
  const float gs = MAP ? 0.f : (float)((double)up[0] / denom);
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float z[KMAX], pr[KMAX], pt, wt;
    load_row<KT>(logits, p, K, z);
    softmax_k(z, pr, K);
    const long t = (long)target[p];
    target_entry(pr, weight, t, K, &pt, &wt);
    const float G = MAP ? up[p] : gs;
    const float coef = wt == 0.f ? 0.f : -G * wt * (pt / (pt + eps));
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) z[k] = coef * ((k == t ? 1.f : 0.f) - pr[k]);
    store_row<KT>(dlogits, p, K, z);
  }
}

template <int KT>
__global__ void __launch_bounds__(256)
    softmax_wkl_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                           const float* __restrict__ weight, const float* __restrict__ gscale,
                           float* __restrict__ dlogits, long npix, int Krt, float eps, double denom) {
  wkl_bwd_body<KT, false>(logits, target, weight, gscale, dlogits, npix, Krt, eps, denom);
}

template <int KT>
__global__ void __launch_bounds__(256)
    softmax_wkl_map_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                               const float* __restrict__ weight, const float* __restrict__ dmap,
                               float* __restrict__ dlogits, long npix, int Krt, float eps) {
  wkl_bwd_body<KT, true>(logits, target, weight, dmap, dlogits, npix, Krt, eps, 1.0);
}

// ---------------------------------------------------------------- soft Dice of the softmax
// blocks per image: one per 256 pixels, the whole grid held to LOSS_GRID_CAP (at least one per image)
inline int dice_blocks_per_image(int N, long HW) {
  long cap = LOSS_GRID_CAP / (N < 1 ? 1 : N);
  if (cap < 1) cap = 1;
  long b = (HW + 255) / 256;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// block (n, b) of the N x bpi grid: part[blk][k] = {A, B} over its pixels of image n, cnt[blk][k] = T
template <int KT>
__global__ void __launch_bounds__(256)
    softmax_dice_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                            double* __restrict__ part, long long* __restrict__ cnt, long HW, int bpi, int Krt, int P) {
  const int K = KT ? KT : Krt;
  const long n = blockIdx.x / bpi, b = blockIdx.x % bpi;
  double A[KMAX], B[KMAX];
  int T[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) A[k] = 0.0, B[k] = 0.0, T[k] = 0;
  for (long q = b * 256L + threadIdx.x; q < HW; q += bpi * 256L) {
    const long p = n * HW + q;
    float z[KMAX], pr[KMAX];
    load_row<KT>(logits, p, K, z);
    softmax_k(z, pr, K);
    const long t = (long)target[p];
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        B[k] += (double)(P == 2 ? pr[k] * pr[k] : pr[k]);
        if (k == t) {
          A[k] += (double)pr[k];
          T[k] += 1;
        }
      }
  }
  // four waves: each sums its lanes by shuffles, then one thread per value adds the four in wave order
  __shared__ double sh[4][2 * KMAX];
  __shared__ int shc[4][KMAX];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      const double a = wave_sum(A[k]), bb = wave_sum(B[k]);
      const int tt = wave_sum(T[k]);
      if (lane == 0) sh[wave][2 * k] = a, sh[wave][2 * k + 1] = bb, shc[wave][k] = tt;
    }
  __syncthreads();
  const int i = threadIdx.x;
  if (i < 2 * K) {
    part[(long)blockIdx.x * 2 * K + i] = ((sh[0][i] + sh[1][i]) + sh[2][i]) + sh[3][i];  // [blk][k][{A, B}]
  } else if (i < 3 * K) {
    const int k = i - 2 * K;
    cnt[(long)blockIdx.x * K + k] = (long long)shc[0][k] + shc[1][k] + shc[2][k] + shc[3][k];
  }
}

// one block: table[n][c] = {num, den} from the bpi partials of image n in block order, then the result:
// none: result[n] = (1/K) sum_{c != ignore} L_nc;  mean / sum: result[0] = (r/K) sum_n sum_{c != ignore} L_nc
__global__ void __launch_bounds__(256)
    softmax_dice_finalize_kernel(const double* __restrict__ part, const long long* __restrict__ cnt,
                                 double* __restrict__ table, float* __restrict__ result, int N, int bpi, int K,
                                 double smooth, int ignore, int reduction) {
  __shared__ double sh[256];
  // one thread per table entry (n, c, num | den); the loads of a thread do not depend on each other: several in flight
  for (long i = threadIdx.x; i < 2L * N * K; i += 256) {
    const long nc = i >> 1, n = nc / K;
    const int c = (int)(nc % K), den = (int)(i & 1);
    const double* src = part + (n * bpi * K + c) * 2 + den;
    const long long* csrc = cnt + n * bpi * K + c;
    double s = 0.0;
    long long t = 0;
#pragma unroll 8
    for (int j = 0; j < bpi; ++j) {
      s += src[(long)j * K * 2];
      if (den) t += csrc[(long)j * K];
    }
    table[i] = s + (double)t + smooth;
  }
  __syncthreads();  // the table rows of image n were written by other threads of this block
  double acc = 0.0;
  for (long n = threadIdx.x; n < N; n += 256) {
    double Ln = 0.0;
    for (int c = 0; c < K; ++c)
      if (c != ignore) Ln += 1.0 - table[2 * (n * K + c)] / table[2 * (n * K + c) + 1];
    if (reduction == RED_NONE)
      result[n] = (float)(Ln / (double)K);
    else
      acc += Ln;
  }
  if (reduction != RED_NONE) {
    const double tot = block_sum_d(acc, sh);
    if (threadIdx.x == 0) result[0] = (float)(tot / ((double)K * (reduction == RED_MEAN ? (double)N : 1.0)));
  }
}

// gup: the upstream gradient, a device scalar (mean, sum) or the [N] vector (none)
template <int KT>
__global__ void __launch_bounds__(256)
    softmax_dice_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                            const double* __restrict__ table, const float* __restrict__ gup,
                            float* __restrict__ dlogits, int N, long HW, int bpi, int Krt, int P, int ignore,
                            int reduction) {
  const int K = KT ? KT : Krt;
  const long n = blockIdx.x / bpi, b = blockIdx.x % bpi;
  // g_c = ca[c] [y = c] + cb[c] p_c^(P-1): the coefficients of image n, once per block in f64
  __shared__ float sca[KMAX], scb[KMAX];
  if (threadIdx.x < KMAX) {
    const int c = threadIdx.x;
    float a = 0.f, bb = 0.f;
    if (c < K && c != ignore) {
      const double G = (double)gup[reduction == RED_NONE ? n : 0];
      const double s = G * (reduction == RED_MEAN ? 1.0 / (double)N : 1.0) / (double)K;
      const double num = table[2 * (n * K + c)], den = table[2 * (n * K + c) + 1];
      a = (float)(-s / den);
      bb = (float)(s * num * (double)P / (den * den));
    }
    sca[c] = a, scb[c] = bb;
  }
  __syncthreads();
  float ca[KMAX], cb[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) ca[k] = sca[k], cb[k] = scb[k];
  for (long q = b * 256L + threadIdx.x; q < HW; q += bpi * 256L) {
    const long p = n * HW + q;
    float z[KMAX], pr[KMAX];
    load_row<KT>(logits, p, K, z);
    softmax_k(z, pr, K);
    const long t = (long)target[p];
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        z[k] = (k == t ? ca[k] : 0.f) + (P == 2 ? cb[k] * pr[k] : cb[k]);
        dot = fmaf(pr[k], z[k], dot);
      }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) z[k] = pr[k] * (z[k] - dot);
    store_row<KT>(dlogits, p, K, z);
  }
}

}  // namespace

extern "C" {

size_t cy_softmax_wkl_ws_bytes(long npix) { return (size_t)cy_blocks(npix, 256, LOSS_GRID_CAP) * sizeof(double); }

int cy_softmax_wkl_fwd(const float* logits, const int64_t* target, const float* weight, float* loss, long npix, int K,
                       float eps, double denom, void* ws, size_t ws_bytes, void* stream) {
  if (!logits || !target || !loss || !ws || npix <= 0 || !(denom > 0.0)) return CY_ERR_ARG;
  if (bad_k(K)) return CY_ERR_SHAPE;
  if (ws_bytes < cy_softmax_wkl_ws_bytes(npix)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = cy_blocks(npix, 256, LOSS_GRID_CAP);
  CY_LAUNCH_BY_K(softmax_wkl_fwd_kernel, nblk, st, logits, target, weight, (double*)ws, npix, K, eps);
  hipLaunchKernelGGL(mean_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, nblk, denom, loss);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_softmax_wkl_map_fwd(const float* logits, const int64_t* target, const float* weight, float* map, long npix,
                           int K, float eps, void* stream) {
  if (!logits || !target || !map || npix <= 0) return CY_ERR_ARG;
  if (bad_k(K)) return CY_ERR_SHAPE;
  CY_LAUNCH_BY_K(softmax_wkl_map_fwd_kernel, cy_blocks(npix, 256, LOSS_GRID_CAP) * 2, (hipStream_t)stream, logits,
                 target, weight, map, npix, K, eps);
  return CY_OK;
}

int cy_softmax_wkl_bwd(const float* logits, const int64_t* target, const float* weight, const float* gscale,
                       float* dlogits, long npix, int K, float eps, double denom, void* stream) {
  if (!logits || !target || !gscale || !dlogits || npix <= 0 || !(denom > 0.0)) return CY_ERR_ARG;
  if (bad_k(K)) return CY_ERR_SHAPE;
  CY_LAUNCH_BY_K(softmax_wkl_bwd_kernel, cy_blocks(npix, 256, LOSS_GRID_CAP) * 2, (hipStream_t)stream, logits, target,
                 weight, gscale, dlogits, npix, K, eps, denom);
  return CY_OK;
}

int cy_softmax_wkl_map_bwd(const float* logits, const int64_t* target, const float* weight, const float* dmap,
                           float* dlogits, long npix, int K, float eps, void* stream) {
  if (!logits || !target || !dmap || !dlogits || npix <= 0) return CY_ERR_ARG;
  if (bad_k(K)) return CY_ERR_SHAPE;
  CY_LAUNCH_BY_K(softmax_wkl_map_bwd_kernel, cy_blocks(npix, 256, LOSS_GRID_CAP) * 2, (hipStream_t)stream, logits,
                 target, weight, dmap, dlogits, npix, K, eps);
  return CY_OK;
}

size_t cy_softmax_dice_ws_bytes(int N, long HW, int K) {
  if (N < 1 || HW < 1 || bad_k(K)) return 0;
  return (size_t)N * dice_blocks_per_image(N, HW) * K * (2 * sizeof(double) + sizeof(long long));
}

int cy_softmax_dice_fwd(const float* logits, const int64_t* target, void* table, float* result, int N, long HW, int K,
                        int P, double smooth, int ignore, int reduction, void* ws, size_t ws_bytes, void* stream) {
  if (!logits || !target || !table || !result || !ws || N <= 0 || HW <= 0 || (P != 1 && P != 2) ||
      reduction < RED_MEAN || reduction > RED_NONE)
    return CY_ERR_ARG;
  if (bad_k(K)) return CY_ERR_SHAPE;
  if (ws_bytes < cy_softmax_dice_ws_bytes(N, HW, K)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int bpi = dice_blocks_per_image(N, HW);
  double* part = (double*)ws;
  long long* cnt = (long long*)(part + (size_t)N * bpi * K * 2);
  CY_LAUNCH_BY_K(softmax_dice_fwd_kernel, N * bpi, st, logits, target, part, cnt, HW, bpi, K, P);
  hipLaunchKernelGGL(softmax_dice_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)part,
                     (const long long*)cnt, (double*)table, result, N, bpi, K, smooth, ignore, reduction);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_softmax_dice_bwd(const float* logits, const int64_t* target, const void* table, const float* gup,
                        float* dlogits, int N, long HW, int K, int P, int ignore, int reduction, void* stream) {
  if (!logits || !target || !table || !gup || !dlogits || N <= 0 || HW <= 0 || (P != 1 && P != 2) ||
      reduction < RED_MEAN || reduction > RED_NONE)
    return CY_ERR_ARG;
  if (bad_k(K)) return CY_ERR_SHAPE;
  const int bpi = dice_blocks_per_image(N, HW);
  CY_LAUNCH_BY_K(softmax_dice_bwd_kernel, N * bpi, (hipStream_t)stream, logits, target, (const double*)table, gup,
                 dlogits, N, HW, bpi, K, P, ignore, reduction);
  return CY_OK;
}

}  // extern "C"
