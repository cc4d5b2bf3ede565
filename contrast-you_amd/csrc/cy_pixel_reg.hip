// Pixel-wise regularisers of the semi-supervised baselines, on [pixels][K] f32 logits (K = classes, 2..16):
//   Entropy()(softmax(logits))                                 semi_seg/hooks/entmin.py:29-30,
//                                                              contrastyou/losses/kl.py:48-56
//   MSELoss()(softmax(logits), one_hot(argmax))                semi_seg/hooks/pseudolabel.py:30-36
//   UA-MT: MSE(teacher, softmax(student)) under the mask       semi_seg/hooks/mt.py:242-248,266-267
//          [teacher entropy < thr], over (mask.mean() + 1e-2)
// The family of cy_head_loss.hip: every kernel reads its logits once, one thread per pixel, grid-stride; the forward
// writes one f64 partial per block and a one-block finalize launch sums them in a fixed order (no atomics: two runs
// give the same bits); the backward is one launch that recomputes the softmax.  K = 2, 4, 8 are compiled with K known
// (exact register arrays, 8- / 16-byte row accesses); any other K takes the run-time form.
#include "cy_common.h"
#include "cy_pixel_loss.h"
#include "cy_reduce.h"  // block_sum_d, mean_finalize_kernel, uamt_finalize_kernel, UAMT_DENOM_EPS

namespace {

// first maximal index (torch.argmax's rule; the warp's padding rows are all-zero logits: class 0)
__device__ __forceinline__ int argmax_k(const float* z, int K) {
  int best = 0;
  float bv = z[0];
#pragma unroll
  for (int k = 1; k < KMAX; ++k)
    if (k < K && z[k] > bv) {
      bv = z[k];
      best = k;
    }
  return best;
}

// -sum_k p_k log(p_k + eps); a p_k that underflowed to 0 adds 0 * log(eps) = 0
__device__ __forceinline__ float entropy_k(const float* p, int K, float eps) {
  float h = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) h = fmaf(-p[k], logf(p[k] + eps), h);
  return h;
}

// ---------------------------------------------------------------- softmax entropy
template <int KT>
__global__ void __launch_bounds__(256)
    softmax_entropy_fwd_kernel(const float* __restrict__ logits, double* __restrict__ partial, long npix, int Krt,
                               float eps) {
  const int K = KT ? KT : Krt;
  __shared__ double sh[256];
  double acc = 0.0;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float z[KMAX], pr[KMAX];
    load_row<KT>(logits, p, K, z);
    softmax_k(z, pr, K);
    acc += (double)entropy_k(pr, K, eps);
  }
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

template <int KT>
__global__ void __launch_bounds__(256)
    softmax_entropy_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ gscale,
                               float* __restrict__ dlogits, long npix, int Krt, float eps) {
  const int K = KT ? KT : Krt;
  const float gs = gscale[0] / (float)npix;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float z[KMAX], pr[KMAX], a[KMAX];
    load_row<KT>(logits, p, K, z);
    softmax_k(z, pr, K);
    // dH/dp_k = a_k = -(log(p_k + eps) + p_k / (p_k + eps));  dz = p * (a - sum_j p_j a_j)
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        const float q = pr[k] + eps;
        a[k] = -(logf(q) + pr[k] / q);
        dot = fmaf(pr[k], a[k], dot);
      }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) a[k] = gs * pr[k] * (a[k] - dot);
    store_row<KT>(dlogits, p, K, a);
  }
}

// ---------------------------------------------------------------- MSE against the own arg-max one-hot
template <int KT>
__global__ void __launch_bounds__(256)
    softmax_selfmse_fwd_kernel(const float* __restrict__ logits, double* __restrict__ partial, long npix, int Krt) {
  const int K = KT ? KT : Krt;
  __shared__ double sh[256];
  double acc = 0.0;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float z[KMAX], pr[KMAX];
    load_row<KT>(logits, p, K, z);
    softmax_k(z, pr, K);
    const int best = argmax_k(z, K);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        const float d = pr[k] - (k == best ? 1.f : 0.f);
        s = fmaf(d, d, s);
      }
    acc += (double)s;
  }
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

template <int KT>
__global__ void __launch_bounds__(256)
    softmax_selfmse_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ gscale,
                               float* __restrict__ dlogits, long npix, int Krt) {
  const int K = KT ? KT : Krt;
  const float gs = 2.f * gscale[0] / ((float)npix * (float)K);
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float z[KMAX], pr[KMAX], d[KMAX];
    load_row<KT>(logits, p, K, z);
    softmax_k(z, pr, K);
    const int best = argmax_k(z, K);
    // the one-hot is a constant: dL/dp_k = gs * d_k, d = p - o;  dz = p * (d - sum_j d_j p_j)
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        d[k] = pr[k] - (k == best ? 1.f : 0.f);
        dot = fmaf(d[k], pr[k], dot);
      }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) d[k] = gs * pr[k] * (d[k] - dot);
    store_row<KT>(dlogits, p, K, d);
  }
}

// ---------------------------------------------------------------- UA-MT: entropy-masked teacher / student MSE
// the teacher's target row (soft, or the one-hot of its arg-max) and its mask bit; the entropy is always the soft one
template <int KT>
__device__ __forceinline__ bool uamt_target(const float* __restrict__ zt, long p, int K, float thr, int hard,
                                            float* tau) {
  float z[KMAX];
  load_row<KT>(zt, p, K, z);
  softmax_k(z, tau, K);
  const bool m = entropy_k(tau, K, 1e-16f) < thr;
  if (hard) {
    const int best = argmax_k(z, K);
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) tau[k] = k == best ? 1.f : 0.f;
  }
  return m;
}

template <int KT>
__global__ void __launch_bounds__(256)
    uamt_mse_fwd_kernel(const float* __restrict__ zt, const float* __restrict__ zs, double* __restrict__ partial,
                        long npix, int Krt, float thr, int hard) {
  const int K = KT ? KT : Krt;
  __shared__ double sh1[256], sh2[256];
  double acc = 0.0, cnt = 0.0;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float tau[KMAX], z[KMAX], s[KMAX];
    const bool m = uamt_target<KT>(zt, p, K, thr, hard, tau);
    load_row<KT>(zs, p, K, z);
    softmax_k(z, s, K);
    float e = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        const float d = tau[k] - s[k];
        e = fmaf(d, d, e);
      }
    if (m) {
      acc += (double)(e / (float)K);
      cnt += 1.0;
    }
  }
  const double t1 = block_sum_d(acc, sh1);
  const double t2 = block_sum_d(cnt, sh2);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = t1;
    partial[2 * blockIdx.x + 1] = t2;
  }
}

template <int KT>
__global__ void __launch_bounds__(256)
    uamt_mse_bwd_kernel(const float* __restrict__ zt, const float* __restrict__ zs, const float* __restrict__ result,
                        const float* __restrict__ gscale, float* __restrict__ dzs, long npix, int Krt, float thr,
                        int hard) {
  const int K = KT ? KT : Krt;
  // the denominator is a constant of the gradient (the reference takes it through .item())
  const float gs = (float)(2.0 * (double)gscale[0] /
                           ((double)K * (double)npix * ((double)result[1] + UAMT_DENOM_EPS)));
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float tau[KMAX], z[KMAX], s[KMAX];
    const bool m = uamt_target<KT>(zt, p, K, thr, hard, tau);
    load_row<KT>(zs, p, K, z);
    softmax_k(z, s, K);
    const float c = m ? gs : 0.f;
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        tau[k] = s[k] - tau[k];  // d = s - tau
        dot = fmaf(tau[k], s[k], dot);
      }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) tau[k] = m ? c * s[k] * (tau[k] - dot) : 0.f;
    store_row<KT>(dzs, p, K, tau);
  }
}

inline bool bad_k(int K) { return K < 2 || K > KMAX; }

}  // namespace

extern "C" {

size_t cy_softmax_entropy_ws_bytes(long npix) { return (size_t)cy_blocks(npix, 256, LOSS_GRID_CAP) * sizeof(double); }

int cy_softmax_entropy_fwd(const float* logits, float* loss, long npix, int K, float eps, void* ws, size_t ws_bytes,
                           void* stream) {
  if (!logits || !loss || !ws || npix <= 0 || bad_k(K)) return CY_ERR_ARG;
  if (ws_bytes < cy_softmax_entropy_ws_bytes(npix)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = cy_blocks(npix, 256, LOSS_GRID_CAP);
  CY_LAUNCH_BY_K(softmax_entropy_fwd_kernel, nblk, st, logits, (double*)ws, npix, K, eps);
  hipLaunchKernelGGL(mean_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, nblk, (double)npix, loss);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_softmax_entropy_bwd(const float* logits, const float* gscale, float* dlogits, long npix, int K, float eps,
                           void* stream) {
  if (!logits || !gscale || !dlogits || npix <= 0 || bad_k(K)) return CY_ERR_ARG;
  CY_LAUNCH_BY_K(softmax_entropy_bwd_kernel, cy_blocks(npix, 256, LOSS_GRID_CAP) * 2, (hipStream_t)stream, logits,
                 gscale, dlogits, npix, K, eps);
  return CY_OK;
}

size_t cy_softmax_selfmse_ws_bytes(long npix) { return (size_t)cy_blocks(npix, 256, LOSS_GRID_CAP) * sizeof(double); }

int cy_softmax_selfmse_fwd(const float* logits, float* loss, long npix, int K, void* ws, size_t ws_bytes,
                           void* stream) {
  if (!logits || !loss || !ws || npix <= 0 || bad_k(K)) return CY_ERR_ARG;
  if (ws_bytes < cy_softmax_selfmse_ws_bytes(npix)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = cy_blocks(npix, 256, LOSS_GRID_CAP);
  CY_LAUNCH_BY_K(softmax_selfmse_fwd_kernel, nblk, st, logits, (double*)ws, npix, K);
  hipLaunchKernelGGL(mean_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, nblk,
                     (double)npix * (double)K, loss);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_softmax_selfmse_bwd(const float* logits, const float* gscale, float* dlogits, long npix, int K, void* stream) {
  if (!logits || !gscale || !dlogits || npix <= 0 || bad_k(K)) return CY_ERR_ARG;
  CY_LAUNCH_BY_K(softmax_selfmse_bwd_kernel, cy_blocks(npix, 256, LOSS_GRID_CAP) * 2, (hipStream_t)stream, logits,
                 gscale, dlogits, npix, K);
  return CY_OK;
}

size_t cy_uamt_mse_ws_bytes(long npix) { return (size_t)cy_blocks(npix, 256, LOSS_GRID_CAP) * 2 * sizeof(double); }

int cy_uamt_mse_fwd(const float* teacher, const float* student, float* result, long npix, int K, float thr, int hard,
                    void* ws, size_t ws_bytes, void* stream) {
  if (!teacher || !student || !result || !ws || npix <= 0 || bad_k(K)) return CY_ERR_ARG;
  if (ws_bytes < cy_uamt_mse_ws_bytes(npix)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = cy_blocks(npix, 256, LOSS_GRID_CAP);
  CY_LAUNCH_BY_K(uamt_mse_fwd_kernel, nblk, st, teacher, student, (double*)ws, npix, K, thr, hard);
  hipLaunchKernelGGL(uamt_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, nblk, (double)npix, result);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_uamt_mse_bwd(const float* teacher, const float* student, const float* result, const float* gscale,
                    float* dstudent, long npix, int K, float thr, int hard, void* stream) {
  if (!teacher || !student || !result || !gscale || !dstudent || npix <= 0 || bad_k(K)) return CY_ERR_ARG;
  CY_LAUNCH_BY_K(uamt_mse_bwd_kernel, cy_blocks(npix, 256, LOSS_GRID_CAP) * 2, (hipStream_t)stream, teacher, student,
                 result, gscale, dstudent, npix, K, thr, hard);
  return CY_OK;
}

}  // extern "C"
