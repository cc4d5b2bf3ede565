// Pixel-wise regularisers of the semi-supervised baselines on multi-prototype ("multicore") logits: [pixels][K] f32,
// 16 < K <= 64, the sixteen-lanes-per-pixel ("row") form of cy_row_loss.h.  Same values as their K <= 16 kernels:
//   Entropy()(softmax(logits))                                 cy_pixel_reg.hip   cy_softmax_entropy_*
//   MSELoss()(softmax(logits), one_hot(argmax))                cy_pixel_reg.hip   cy_softmax_selfmse_*
//   UA-MT: entropy-masked teacher / student MSE                cy_pixel_reg.hip   cy_uamt_mse_*
//   ICT: MSE against the blend of two teacher softmaxes        cy_mixup.hip       cy_softmax_mixmse_*
// Lane j of a row holds logits 4j..4j+3, absent ones (k >= K) as -inf: their exp is 0, so sums of probabilities need no
// mask, but every term that takes a logarithm is masked by index.  A wave holds 4 pixels, a block 16 per grid-stride
// iteration; every lane of a block runs the same number of iterations: rows past the end recompute the last pixel, take
// part in every shuffle and neither store nor accumulate.  Lane k0 == 0 of a live row adds the row's value to the f64
// accumulators; the forward writes one f64 partial per block (UA-MT: sum and count) and a one-block launch sums them in
// block order: no atomics, two runs give the same bits.  The backward is one launch that recomputes the softmax.
// One launch rule (wide_plan) for all four: 16-byte accesses where K % 4 == 0 and every base is 16-byte aligned.
#include "cy_common.h"
#include "cy_reduce.h"    // block_sum_d, mean_finalize_kernel, uamt_finalize_kernel, UAMT_DENOM_EPS
#include "cy_row_loss.h"  // KROW, ROW, ROWS, row_sum, row_max, load_row4, store_row4, row_exp

namespace {

constexpr int WIDE_KMIN = 17;       // below it the one-thread-per-pixel kernels
constexpr int WIDE_GRID_CAP = 4096;  // blocks either way: 32 KiB of partials (64 KiB UA-MT), 16 per thread of the final sum

// first maximal index of the row, in every lane: torch.argmax's rule (the warp's all-zero padding rows: class 0).
// (value, index) pairs are reduced with ties going to the smaller index; an absent channel (-inf) never wins.
__device__ __forceinline__ int row_argmax(const float* z, int k0) {
  float bv = z[0];
  int best = k0;
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (z[i] > bv) bv = z[i], best = k0 + i;
#pragma unroll
  for (int o = ROW / 2; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(best, o, 64);
    if (ov > bv || (ov == bv && oi < best)) bv = ov, best = oi;
  }
  return best;
}

// p = softmax of the row, this lane's four (0 for absent channels)
__device__ __forceinline__ void row_softmax(const float* z, float* p) {
  const float inv = 1.f / row_exp(z, p);
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] *= inv;
}

// the row's -sum_k p_k log(p_k + eps) over the channels that exist, in every lane; a present p_k that underflowed to 0
// adds 0 * log(eps) = 0 (NaN at eps == 0, as the reference)
__device__ __forceinline__ float row_entropy(const float* p, int K, int k0, float eps) {
  float h = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (k0 + i < K) h = fmaf(-p[i], logf(p[i] + eps), h);
  return row_sum(h);
}

// the row's sum of (a_k - b_k)^2, in every lane
__device__ __forceinline__ float row_sqdist(const float* a, const float* b) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float d = a[i] - b[i];
    s = fmaf(d, d, s);
  }
  return row_sum(s);
}

// the softmax backward of a constant target: d = p - t, out = c p (d - sum_j d_j p_j)
__device__ __forceinline__ void row_mse_grad(const float* p, const float* t, float c, float* out) {
  float d[4], dot = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    d[i] = p[i] - t[i];
    dot = fmaf(d[i], p[i], dot);
  }
  dot = row_sum(dot);
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = c * p[i] * (d[i] - dot);
}

__device__ __forceinline__ void row_onehot(int best, int k0, float* t) {
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = k0 + i == best ? 1.f : 0.f;
}

// the loop every kernel here runs: r = the block's row of this lane, k0 = its first channel
#define WIDE_ROWS_LOOP                                                                              \
  const int r = threadIdx.x / ROW, k0 = 4 * (threadIdx.x % ROW);                                    \
  for (long base = (long)blockIdx.x * ROWS; base < npix; base += (long)gridDim.x * ROWS)
#define WIDE_ROW_PIXEL                      \
  const bool live = base + r < npix;        \
  const long p = live ? base + r : npix - 1

// ---------------------------------------------------------------- softmax entropy
template <bool VEC>
__global__ void __launch_bounds__(256)
    softmax_entropy_fwd_row_kernel(const float* __restrict__ logits, double* __restrict__ partial, long npix, int K,
                                   float eps) {
  __shared__ double sh[256];
  double acc = 0.0;
  WIDE_ROWS_LOOP {
    WIDE_ROW_PIXEL;
    float z[4], pr[4];
    load_row4<VEC>(logits, p, K, k0, z);
    row_softmax(z, pr);
    const float h = row_entropy(pr, K, k0, eps);
    if (live && k0 == 0) acc += (double)h;
  }
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

template <bool VEC>
__global__ void __launch_bounds__(256)
    softmax_entropy_bwd_row_kernel(const float* __restrict__ logits, const float* __restrict__ gscale,
                                   float* __restrict__ dlogits, long npix, int K, float eps) {
  const float gs = gscale[0] / (float)npix;
  WIDE_ROWS_LOOP {
    WIDE_ROW_PIXEL;
    float z[4], pr[4], a[4];
    load_row4<VEC>(logits, p, K, k0, z);
    row_softmax(z, pr);
    // dH/dp_k = a_k = -(log(p_k + eps) + p_k / (p_k + eps));  dz = p * (a - sum_j p_j a_j)
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[i] = 0.f;
      if (k0 + i < K) {
        const float q = pr[i] + eps;
        a[i] = -(logf(q) + pr[i] / q);
        dot = fmaf(pr[i], a[i], dot);
      }
    }
    dot = row_sum(dot);
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = gs * pr[i] * (a[i] - dot);
    if (live) store_row4<VEC>(dlogits, p, K, k0, a);
  }
}

// ---------------------------------------------------------------- MSE against the own arg-max one-hot
template <bool VEC>
__global__ void __launch_bounds__(256)
    softmax_selfmse_fwd_row_kernel(const float* __restrict__ logits, double* __restrict__ partial, long npix, int K) {
  __shared__ double sh[256];
  double acc = 0.0;
  WIDE_ROWS_LOOP {
    WIDE_ROW_PIXEL;
    float z[4], pr[4], t[4];
    load_row4<VEC>(logits, p, K, k0, z);
    row_softmax(z, pr);
    row_onehot(row_argmax(z, k0), k0, t);
    const float s = row_sqdist(pr, t);
    if (live && k0 == 0) acc += (double)s;
  }
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

template <bool VEC>
__global__ void __launch_bounds__(256)
    softmax_selfmse_bwd_row_kernel(const float* __restrict__ logits, const float* __restrict__ gscale,
                                   float* __restrict__ dlogits, long npix, int K) {
  const float gs = 2.f * gscale[0] / ((float)npix * (float)K);
  WIDE_ROWS_LOOP {
    WIDE_ROW_PIXEL;
    float z[4], pr[4], t[4];
    load_row4<VEC>(logits, p, K, k0, z);
    row_softmax(z, pr);
    row_onehot(row_argmax(z, k0), k0, t);  // the one-hot is a constant
    row_mse_grad(pr, t, gs, t);
    if (live) store_row4<VEC>(dlogits, p, K, k0, t);
  }
}

// ---------------------------------------------------------------- UA-MT: entropy-masked teacher / student MSE
// the teacher's target row (soft, or the one-hot of its arg-max) and its mask bit; the entropy is always the soft one
template <bool VEC>
__device__ __forceinline__ bool uamt_target_row(const float* __restrict__ zt, long p, int K, int k0, float thr,
                                                int hard, float* tau) {
  float z[4];
  load_row4<VEC>(zt, p, K, k0, z);
  row_softmax(z, tau);
  const bool m = row_entropy(tau, K, k0, 1e-16f) < thr;
  if (hard) row_onehot(row_argmax(z, k0), k0, tau);  // (uniform over the block: every lane shuffles)
  return m;
}

template <bool VEC>
__global__ void __launch_bounds__(256)
    uamt_mse_fwd_row_kernel(const float* __restrict__ zt, const float* __restrict__ zs, double* __restrict__ partial,
                            long npix, int K, float thr, int hard) {
  __shared__ double sh1[256], sh2[256];
  double acc = 0.0, cnt = 0.0;
  WIDE_ROWS_LOOP {
    WIDE_ROW_PIXEL;
    float tau[4], z[4], s[4];
    const bool m = uamt_target_row<VEC>(zt, p, K, k0, thr, hard, tau);
    load_row4<VEC>(zs, p, K, k0, z);
    row_softmax(z, s);
    const float e = row_sqdist(tau, s);
    if (live && k0 == 0 && m) {
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

template <bool VEC>
__global__ void __launch_bounds__(256)
    uamt_mse_bwd_row_kernel(const float* __restrict__ zt, const float* __restrict__ zs,
                            const float* __restrict__ result, const float* __restrict__ gscale,
                            float* __restrict__ dzs, long npix, int K, float thr, int hard) {
  // the denominator is a constant of the gradient (the reference takes it through .item())
  const float gs = (float)(2.0 * (double)gscale[0] /
                           ((double)K * (double)npix * ((double)result[1] + UAMT_DENOM_EPS)));
  WIDE_ROWS_LOOP {
    WIDE_ROW_PIXEL;
    float tau[4], z[4], s[4];
    const bool m = uamt_target_row<VEC>(zt, p, K, k0, thr, hard, tau);
    load_row4<VEC>(zs, p, K, k0, z);
    row_softmax(z, s);
    row_mse_grad(s, tau, gs, tau);
    if (!m) tau[0] = tau[1] = tau[2] = tau[3] = 0.f;
    if (live) store_row4<VEC>(dzs, p, K, k0, tau);
  }
}

// ---------------------------------------------------------------- ICT: MSE against the blend of two teacher softmaxes
// m = ws softmax(t[p]) + wo softmax(t[partner]); the partner is the same pixel of image index[n]
template <bool VEC>
__device__ __forceinline__ void ict_target_row(const float* __restrict__ zt, const int32_t* __restrict__ index, long p,
                                               long HW, int K, int k0, float ws, float wo, float* m) {
  float z[4], q[4];
  load_row4<VEC>(zt, p, K, k0, z);
  row_softmax(z, m);
  const long n = p / HW;
  load_row4<VEC>(zt, (long)index[n] * HW + (p - n * HW), K, k0, z);
  row_softmax(z, q);
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = fmaf(wo, q[i], ws * m[i]);
}

template <bool VEC>
__global__ void __launch_bounds__(256)
    softmax_mixmse_fwd_row_kernel(const float* __restrict__ zs, const float* __restrict__ zt,
                                  const int32_t* __restrict__ index, float ws, float wo,
                                  double* __restrict__ partial, long npix, long HW, int K) {
  __shared__ double sh[256];
  double acc = 0.0;
  WIDE_ROWS_LOOP {
    WIDE_ROW_PIXEL;
    float m[4], z[4], s[4];
    ict_target_row<VEC>(zt, index, p, HW, K, k0, ws, wo, m);
    load_row4<VEC>(zs, p, K, k0, z);
    row_softmax(z, s);
    const float e = row_sqdist(s, m);
    if (live && k0 == 0) acc += (double)e;
  }
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

template <bool VEC>
__global__ void __launch_bounds__(256)
    softmax_mixmse_bwd_row_kernel(const float* __restrict__ zs, const float* __restrict__ zt,
                                  const int32_t* __restrict__ index, float ws, float wo,
                                  const float* __restrict__ gscale, float* __restrict__ dzs, long npix, long HW,
                                  int K) {
  const float gs = (float)(2.0 * (double)gscale[0] / ((double)npix * (double)K));
  WIDE_ROWS_LOOP {
    WIDE_ROW_PIXEL;
    float m[4], z[4], s[4];
    ict_target_row<VEC>(zt, index, p, HW, K, k0, ws, wo, m);  // the target is a constant
    load_row4<VEC>(zs, p, K, k0, z);
    row_softmax(z, s);
    row_mse_grad(s, m, gs, m);
    if (live) store_row4<VEC>(dzs, p, K, k0, m);
  }
}

// ---------------------------------------------------------------- the launch rule
// the one place the four families take their kernel form and grid from; a status as the launches return it, and nothing
// is written to `pl` before the last refusal
int wide_plan(int family, long npix, int K, int align, cy_wide_reg_plan_t* pl) {
  if (!pl || family < CY_WIDE_ENTROPY || family > CY_WIDE_MIXMSE || npix < 1 || align < 1) return CY_ERR_ARG;
  if (K < WIDE_KMIN || K > KROW) return CY_ERR_SHAPE;
  if (align % 4 != 0) return CY_ERR_ARG;
  pl->vec = (K % 4 == 0 && align % 16 == 0) ? 4 : 1;
  pl->rows_per_block = ROWS;
  pl->fwd_grid = pl->bwd_grid = cy_blocks(npix, ROWS, WIDE_GRID_CAP);
  pl->fwd_trips = pl->bwd_trips = cy_trips(npix, pl->fwd_grid, ROWS);
  return CY_OK;
}

// partials per block: UA-MT keeps the sum and the count
inline size_t wide_ws_bytes(long npix, int per_block) {
  if (npix < 1) return 0;
  return (size_t)cy_blocks(npix, ROWS, WIDE_GRID_CAP) * per_block * sizeof(double);
}

// launch `KERNEL<vec == 4>` on the plan's grid
#define CY_WIDE_LAUNCH(KERNEL, VEC_, GRID, ST, ...)                                    \
  do {                                                                                 \
    if ((VEC_) == 4)                                                                   \
      hipLaunchKernelGGL(KERNEL<true>, dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);     \
    else                                                                               \
      hipLaunchKernelGGL(KERNEL<false>, dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);    \
    CY_CHECK_LAUNCH();                                                                 \
  } while (0)

}  // namespace

extern "C" {

int cy_wide_reg_plan(int family, long npix, int K, int align, cy_wide_reg_plan_t* out) {
  return wide_plan(family, npix, K, align, out);  // (a NULL `out` is the rule's first refusal)
}

size_t cy_softmax_entropy_row_ws_bytes(long npix) { return wide_ws_bytes(npix, 1); }

int cy_softmax_entropy_row_fwd(const float* logits, float* loss, long npix, int K, float eps, void* ws,
                               size_t ws_bytes, void* stream) {
  if (!logits || !loss || !ws) return CY_ERR_ARG;
  cy_wide_reg_plan_t pl;
  const int rc = wide_plan(CY_WIDE_ENTROPY, npix, K, ptr_align(logits), &pl);
  if (rc != CY_OK) return rc;
  if (ws_bytes < wide_ws_bytes(npix, 1)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  CY_WIDE_LAUNCH(softmax_entropy_fwd_row_kernel, pl.vec, pl.fwd_grid, st, logits, (double*)ws, npix, K, eps);
  hipLaunchKernelGGL(mean_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, pl.fwd_grid, (double)npix,
                     loss);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_softmax_entropy_row_bwd(const float* logits, const float* gscale, float* dlogits, long npix, int K, float eps,
                               void* stream) {
  if (!logits || !gscale || !dlogits) return CY_ERR_ARG;
  cy_wide_reg_plan_t pl;
  const int rc = wide_plan(CY_WIDE_ENTROPY, npix, K, min_int(ptr_align(logits), ptr_align(dlogits)), &pl);
  if (rc != CY_OK) return rc;
  CY_WIDE_LAUNCH(softmax_entropy_bwd_row_kernel, pl.vec, pl.bwd_grid, (hipStream_t)stream, logits, gscale, dlogits,
                 npix, K, eps);
  return CY_OK;
}

size_t cy_softmax_selfmse_row_ws_bytes(long npix) { return wide_ws_bytes(npix, 1); }

int cy_softmax_selfmse_row_fwd(const float* logits, float* loss, long npix, int K, void* ws, size_t ws_bytes,
                               void* stream) {
  if (!logits || !loss || !ws) return CY_ERR_ARG;
  cy_wide_reg_plan_t pl;
  const int rc = wide_plan(CY_WIDE_SELFMSE, npix, K, ptr_align(logits), &pl);
  if (rc != CY_OK) return rc;
  if (ws_bytes < wide_ws_bytes(npix, 1)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  CY_WIDE_LAUNCH(softmax_selfmse_fwd_row_kernel, pl.vec, pl.fwd_grid, st, logits, (double*)ws, npix, K);
  hipLaunchKernelGGL(mean_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, pl.fwd_grid,
                     (double)npix * (double)K, loss);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_softmax_selfmse_row_bwd(const float* logits, const float* gscale, float* dlogits, long npix, int K,
                               void* stream) {
  if (!logits || !gscale || !dlogits) return CY_ERR_ARG;
  cy_wide_reg_plan_t pl;
  const int rc = wide_plan(CY_WIDE_SELFMSE, npix, K, min_int(ptr_align(logits), ptr_align(dlogits)), &pl);
  if (rc != CY_OK) return rc;
  CY_WIDE_LAUNCH(softmax_selfmse_bwd_row_kernel, pl.vec, pl.bwd_grid, (hipStream_t)stream, logits, gscale, dlogits,
                 npix, K);
  return CY_OK;
}

size_t cy_uamt_mse_row_ws_bytes(long npix) { return wide_ws_bytes(npix, 2); }

int cy_uamt_mse_row_fwd(const float* teacher, const float* student, float* result, long npix, int K, float thr,
                        int hard, void* ws, size_t ws_bytes, void* stream) {
  if (!teacher || !student || !result || !ws) return CY_ERR_ARG;
  cy_wide_reg_plan_t pl;
  const int rc = wide_plan(CY_WIDE_UAMT, npix, K, min_int(ptr_align(teacher), ptr_align(student)), &pl);
  if (rc != CY_OK) return rc;
  if (ws_bytes < wide_ws_bytes(npix, 2)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  CY_WIDE_LAUNCH(uamt_mse_fwd_row_kernel, pl.vec, pl.fwd_grid, st, teacher, student, (double*)ws, npix, K, thr, hard);
  hipLaunchKernelGGL(uamt_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, pl.fwd_grid, (double)npix,
                     result);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_uamt_mse_row_bwd(const float* teacher, const float* student, const float* result, const float* gscale,
                        float* dstudent, long npix, int K, float thr, int hard, void* stream) {
  if (!teacher || !student || !result || !gscale || !dstudent) return CY_ERR_ARG;
  cy_wide_reg_plan_t pl;
  const int rc = wide_plan(CY_WIDE_UAMT, npix, K,
                           min_int(min_int(ptr_align(teacher), ptr_align(student)), ptr_align(dstudent)), &pl);
  if (rc != CY_OK) return rc;
  CY_WIDE_LAUNCH(uamt_mse_bwd_row_kernel, pl.vec, pl.bwd_grid, (hipStream_t)stream, teacher, student, result, gscale,
                 dstudent, npix, K, thr, hard);
  return CY_OK;
}

size_t cy_softmax_mixmse_row_ws_bytes(int N, long HW) { return (N < 1 || HW < 1) ? 0 : wide_ws_bytes((long)N * HW, 1); }

int cy_softmax_mixmse_row_fwd(const float* student, const float* teacher, const int32_t* index, float w_self,
                              float w_other, float* loss, int N, long HW, int K, void* ws, size_t ws_bytes,
                              void* stream) {
  if (!student || !teacher || !index || !loss || !ws || N < 1 || HW < 1) return CY_ERR_ARG;
  const long npix = (long)N * HW;
  cy_wide_reg_plan_t pl;
  const int rc = wide_plan(CY_WIDE_MIXMSE, npix, K, min_int(ptr_align(student), ptr_align(teacher)), &pl);
  if (rc != CY_OK) return rc;
  if (ws_bytes < wide_ws_bytes(npix, 1)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  CY_WIDE_LAUNCH(softmax_mixmse_fwd_row_kernel, pl.vec, pl.fwd_grid, st, student, teacher, index, w_self, w_other,
                 (double*)ws, npix, HW, K);
  hipLaunchKernelGGL(mean_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, pl.fwd_grid,
                     (double)npix * (double)K, loss);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_softmax_mixmse_row_bwd(const float* student, const float* teacher, const int32_t* index, float w_self,
                              float w_other, const float* gscale, float* dstudent, int N, long HW, int K,
                              void* stream) {
  if (!student || !teacher || !index || !gscale || !dstudent || N < 1 || HW < 1) return CY_ERR_ARG;
  const long npix = (long)N * HW;
  cy_wide_reg_plan_t pl;
  const int rc = wide_plan(CY_WIDE_MIXMSE, npix, K,
                           min_int(min_int(ptr_align(student), ptr_align(teacher)), ptr_align(dstudent)), &pl);
  if (rc != CY_OK) return rc;
  CY_WIDE_LAUNCH(softmax_mixmse_bwd_row_kernel, pl.vec, pl.bwd_grid, (hipStream_t)stream, student, teacher, index,
                 w_self, w_other, gscale, dstudent, npix, HW, K);
  return CY_OK;
}

}  // extern "C"
