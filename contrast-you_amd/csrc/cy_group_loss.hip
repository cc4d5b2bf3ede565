// Pixel-wise losses of the multi-prototype ("multicore") recipes over [pixels][K] f32 logits, K = G classes x m prototypes.
//   MultiCoreKL: KL_div(group sums of softmax(logits), one_hot(target))   contrastyou/losses/multicore_loss.py:41-60
//   UniversalDice on the reduced arg-max                                  semi_seg/epochers/features/multicore_epocher.py:64-67,84-91
//   MSE(softmax(a), softmax(b)) at 16 < K <= 64                           semi_seg/hooks/consistency.py:34-36
// Class g owns the contiguous channels [g*m, (g+1)*m).
// Two forms, chosen on the host by K:
//   K <= 16       one thread per pixel on the helpers of cy_pixel_loss.h, the group sums taken in registers;
//   16 < K <= 64  sixteen lanes per pixel (a "row"): lane j holds logits 4j..4j+3, absent ones as -inf; maximum, sums and
//                 arg-max are reduced with __shfl_xor at offsets 8, 4, 2, 1, which never leave the aligned 16-lane row.
//                 A wave holds 4 pixels, a block 16 per grid-stride iteration; every lane of a block runs the same number
//                 of iterations (rows past the end recompute the last pixel and contribute nothing).
// Loss partials are one f64 per block, summed in a fixed order by mean_finalize_kernel: two runs give the same bits.
#include "cy_common.h"
#include "cy_pixel_loss.h"  // KMAX, softmax_k, load_logits
#include "cy_reduce.h"      // block_sum_d, mean_finalize_kernel, LOSS_GRID_CAP
#include "cy_row_loss.h"    // KROW, ROW, ROWS, row_sum, row_max, load_row4, store_row4, row_exp, part_in

namespace {

// ---------------------------------------------------------------- grouped softmax + KL(one-hot), K <= 16
__global__ void __launch_bounds__(256)
    group_kl_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                        double* __restrict__ partial, long npix, int K, int m, float eps) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float z[KMAX], pr[KMAX];
    load_logits(logits, p, K, z);
    softmax_k(z, pr, K);
    const int lo = (int)target[p] * m, hi = lo + m;
    float pt = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K && k >= lo && k < hi) pt += pr[k];
    acc += (double)(-logf((pt + eps) / (1.f + eps)));
  }
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(256)
    group_kl_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                        const float* __restrict__ gscale, float* __restrict__ dlogits, long npix, int K,
                        int m, float eps) {
  const float gs = gscale[0] / (float)npix;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float z[KMAX], pr[KMAX];
    load_logits(logits, p, K, z);
    softmax_k(z, pr, K);
    const int lo = (int)target[p] * m, hi = lo + m;
    float pt = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K && k >= lo && k < hi) pt += pr[k];
    const float coef = -gs / (pt + eps);
    if (K == 4) {
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = coef * pr[k] * ((k >= lo && k < hi ? 1.f : 0.f) - pt);
      *reinterpret_cast<f32x4*>(dlogits + p * 4) = o;
    } else {
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) dlogits[p * K + k] = coef * pr[k] * ((k >= lo && k < hi ? 1.f : 0.f) - pt);
    }
  }
}

// ---------------------------------------------------------------- grouped softmax + KL(one-hot), 16 < K <= 64
template <bool VEC>
__global__ void __launch_bounds__(256)
    group_kl_fwd_row_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                            double* __restrict__ partial, long npix, int K, int m, float eps) {
  __shared__ double sh[256];
  const int r = threadIdx.x / ROW, k0 = 4 * (threadIdx.x % ROW);
  double acc = 0.0;
  for (long base = (long)blockIdx.x * ROWS; base < npix; base += (long)gridDim.x * ROWS) {
    const bool live = base + r < npix;
    const long p = live ? base + r : npix - 1;
    float z[4], e[4];
    load_row4<VEC>(logits, p, K, k0, z);
    const float s = row_exp(z, e);
    const int lo = (int)target[p] * m;
    const float pt = row_sum(part_in(e, k0, lo, lo + m)) / s;
    if (live && k0 == 0) acc += (double)(-logf((pt + eps) / (1.f + eps)));
  }
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

template <bool VEC>
__global__ void __launch_bounds__(256)
    group_kl_bwd_row_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                            const float* __restrict__ gscale, float* __restrict__ dlogits, long npix,
                            int K, int m, float eps) {
  const float gs = gscale[0] / (float)npix;
  const int r = threadIdx.x / ROW, k0 = 4 * (threadIdx.x % ROW);
  for (long base = (long)blockIdx.x * ROWS; base < npix; base += (long)gridDim.x * ROWS) {
    const bool live = base + r < npix;
    const long p = live ? base + r : npix - 1;
    float z[4], e[4], d[4];
    load_row4<VEC>(logits, p, K, k0, z);
    const float inv = 1.f / row_exp(z, e);
    const int lo = (int)target[p] * m, hi = lo + m;
    const float pt = row_sum(part_in(e, k0, lo, hi)) * inv;
    const float coef = -gs / (pt + eps);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      d[i] = coef * (e[i] * inv) * ((k0 + i >= lo && k0 + i < hi ? 1.f : 0.f) - pt);
    if (live) store_row4<VEC>(dlogits, p, K, k0, d);
  }
}

// ---------------------------------------------------------------- MSE of two softmaxes, 16 < K <= 64
template <bool VEC>
__global__ void __launch_bounds__(256)
    softmax_mse_fwd_row_kernel(const float* __restrict__ a, const float* __restrict__ b,
                               double* __restrict__ partial, long npix, int K) {
  __shared__ double sh[256];
  const int r = threadIdx.x / ROW, k0 = 4 * (threadIdx.x % ROW);
  double acc = 0.0;
  for (long base = (long)blockIdx.x * ROWS; base < npix; base += (long)gridDim.x * ROWS) {
    const bool live = base + r < npix;
    const long p = live ? base + r : npix - 1;
    float za[4], zb[4], ea[4], eb[4];
    load_row4<VEC>(a, p, K, k0, za);
    load_row4<VEC>(b, p, K, k0, zb);
    const float ia = 1.f / row_exp(za, ea), ib = 1.f / row_exp(zb, eb);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float d = ea[i] * ia - eb[i] * ib;
      s = fmaf(d, d, s);
    }
    s = row_sum(s);
    if (live && k0 == 0) acc += (double)s;
  }
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

template <bool VEC>
__global__ void __launch_bounds__(256)
    softmax_mse_bwd_row_kernel(const float* __restrict__ a, const float* __restrict__ b,
                               const float* __restrict__ gscale, float* __restrict__ da,
                               float* __restrict__ db, long npix, int K) {
  const float gs = 2.f * gscale[0] / ((float)npix * (float)K);
  const int r = threadIdx.x / ROW, k0 = 4 * (threadIdx.x % ROW);
  for (long base = (long)blockIdx.x * ROWS; base < npix; base += (long)gridDim.x * ROWS) {
    const bool live = base + r < npix;
    const long p = live ? base + r : npix - 1;
    float za[4], zb[4], pa[4], pb[4], ga[4], gb[4];
    load_row4<VEC>(a, p, K, k0, za);
    load_row4<VEC>(b, p, K, k0, zb);
    const float ia = 1.f / row_exp(za, pa), ib = 1.f / row_exp(zb, pb);
    // dL/dpa_k = gs*(pa_k-pb_k); dz = p * (g - sum_j g_j p_j)
    float dota = 0.f, dotb = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pa[i] *= ia;
      pb[i] *= ib;
      const float d = pa[i] - pb[i];
      dota = fmaf(d, pa[i], dota);
      dotb = fmaf(d, pb[i], dotb);
    }
    dota = row_sum(dota);
    dotb = row_sum(dotb);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float d = pa[i] - pb[i];
      ga[i] = gs * pa[i] * (d - dota);
      gb[i] = -gs * pb[i] * (d - dotb);
    }
    if (live && da) store_row4<VEC>(da, p, K, k0, ga);
    if (live && db) store_row4<VEC>(db, p, K, k0, gb);
  }
}

// ---------------------------------------------------------------- dice counts on the reduced arg-max
// grid (blocks_per_sample, N).  The predicted class is the first maximal group sum of exp(z - max z).
__global__ void __launch_bounds__(256)
    group_dice_counts_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                             unsigned long long* __restrict__ counts, int HW, int K, int G, int m) {
  __shared__ unsigned int sc[KMAX * 2];
  const int n = blockIdx.y;
  if (threadIdx.x < KMAX * 2) sc[threadIdx.x] = 0u;
  __syncthreads();
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const long gp = (long)n * HW + p;
    float z[KMAX];
    load_logits(logits, gp, K, z);
    float mx = z[0];
#pragma unroll
    for (int k = 1; k < KMAX; ++k)
      if (k < K) mx = fmaxf(mx, z[k]);
    int best = 0, g = 0, c = 0;
    float bv = -1.f, cur = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        cur += expf(z[k] - mx);
        if (++c == m) {
          if (cur > bv) bv = cur, best = g;
          cur = 0.f, c = 0, ++g;
        }
      }
    const int t = (int)target[gp];
    if (best == t) atomicAdd(&sc[best * 2 + 0], 1u);
    atomicAdd(&sc[best * 2 + 1], 1u);
    if (t >= 0 && t < G) atomicAdd(&sc[t * 2 + 1], 1u);
  }
  __syncthreads();
  if (threadIdx.x < G * 2 && sc[threadIdx.x])
    atomicAdd(&counts[(size_t)n * G * 2 + threadIdx.x], (unsigned long long)sc[threadIdx.x]);
}

template <bool VEC>
__global__ void __launch_bounds__(256)
    group_dice_counts_row_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                 unsigned long long* __restrict__ counts, int HW, int K, int G, int m) {
  __shared__ unsigned int sc[KROW * 2];
  const int n = blockIdx.y;
  if (threadIdx.x < KROW * 2) sc[threadIdx.x] = 0u;
  __syncthreads();
  const int r = threadIdx.x / ROW, k0 = 4 * (threadIdx.x % ROW);
  for (int base = blockIdx.x * ROWS; base < HW; base += gridDim.x * ROWS) {
    const bool live = base + r < HW;
    const long gp = (long)n * HW + (live ? base + r : HW - 1);
    float z[4], e[4];
    load_row4<VEC>(logits, gp, K, k0, z);
    row_exp(z, e);
    int best = 0;
    float bv = -1.f;
    for (int g = 0; g < G; ++g) {  // every lane of the row ends with the same (bv, best)
      const float s = row_sum(part_in(e, k0, g * m, g * m + m));
      if (s > bv) bv = s, best = g;
    }
    if (live && k0 == 0) {
      const int t = (int)target[gp];
      if (best == t) atomicAdd(&sc[best * 2 + 0], 1u);
      atomicAdd(&sc[best * 2 + 1], 1u);
      if (t >= 0 && t < G) atomicAdd(&sc[t * 2 + 1], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x < G * 2 && sc[threadIdx.x])
    atomicAdd(&counts[(size_t)n * G * 2 + threadIdx.x], (unsigned long long)sc[threadIdx.x]);
}

inline int group_kl_blocks(long npix, int K) {
  return K <= KMAX ? cy_blocks(npix, 256, LOSS_GRID_CAP) : cy_blocks(npix, ROWS, 1024);
}

}  // namespace

// the wide softmax-MSE behind cy_softmax_mse_fwd / cy_softmax_mse_bwd (cy_head_loss.hip, same shared object): arguments
// are checked there; nblk partials fit the workspace of cy_softmax_mse_ws_bytes
int cy_softmax_mse_row_fwd(const float* a, const float* b, float* loss, long npix, int K, void* ws, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int nblk = cy_blocks(npix, 256, LOSS_GRID_CAP);
  if (K % 4 == 0)
    hipLaunchKernelGGL(softmax_mse_fwd_row_kernel<true>, dim3(nblk), dim3(256), 0, st, a, b, (double*)ws, npix, K);
  else
    hipLaunchKernelGGL(softmax_mse_fwd_row_kernel<false>, dim3(nblk), dim3(256), 0, st, a, b, (double*)ws, npix, K);
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(mean_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, nblk,
                     (double)npix * (double)K, loss);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_softmax_mse_row_bwd(const float* a, const float* b, const float* gscale, float* da, float* db, long npix, int K,
                           void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int nblk = cy_blocks(npix, ROWS, 4096);
  if (K % 4 == 0)
    hipLaunchKernelGGL(softmax_mse_bwd_row_kernel<true>, dim3(nblk), dim3(256), 0, st, a, b, gscale, da, db, npix, K);
  else
    hipLaunchKernelGGL(softmax_mse_bwd_row_kernel<false>, dim3(nblk), dim3(256), 0, st, a, b, gscale, da, db, npix, K);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

extern "C" {

size_t cy_softmax_group_kl_ws_bytes(long npix, int K) { return (size_t)group_kl_blocks(npix, K) * sizeof(double); }

int cy_softmax_group_kl_fwd(const float* logits, const int64_t* target, float* loss, long npix, int K, int G,
                            float eps, void* ws, size_t ws_bytes, void* stream) {
  if (!logits || !target || !loss || !ws || npix <= 0) return CY_ERR_ARG;
  if (K < 1 || K > KROW || G < 1 || K % G) return CY_ERR_SHAPE;
  if (ws_bytes < cy_softmax_group_kl_ws_bytes(npix, K)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = group_kl_blocks(npix, K), m = K / G;
  if (K <= KMAX)
    hipLaunchKernelGGL(group_kl_fwd_kernel, dim3(nblk), dim3(256), 0, st, logits, target, (double*)ws, npix, K, m,
                       eps);
  else if (K % 4 == 0)
    hipLaunchKernelGGL(group_kl_fwd_row_kernel<true>, dim3(nblk), dim3(256), 0, st, logits, target, (double*)ws,
                       npix, K, m, eps);
  else
    hipLaunchKernelGGL(group_kl_fwd_row_kernel<false>, dim3(nblk), dim3(256), 0, st, logits, target, (double*)ws,
                       npix, K, m, eps);
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(mean_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, nblk, (double)npix, loss);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_softmax_group_kl_bwd(const float* logits, const int64_t* target, const float* gscale, float* dlogits,
                            long npix, int K, int G, float eps, void* stream) {
  if (!logits || !target || !gscale || !dlogits || npix <= 0) return CY_ERR_ARG;
  if (K < 1 || K > KROW || G < 1 || K % G) return CY_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int m = K / G;
  if (K <= KMAX)
    hipLaunchKernelGGL(group_kl_bwd_kernel, dim3(cy_blocks(npix, 256, LOSS_GRID_CAP) * 2), dim3(256), 0, st, logits,
                       target, gscale, dlogits, npix, K, m, eps);
  else if (K % 4 == 0)
    hipLaunchKernelGGL(group_kl_bwd_row_kernel<true>, dim3(cy_blocks(npix, ROWS, 4096)), dim3(256), 0, st, logits,
                       target, gscale, dlogits, npix, K, m, eps);
  else
    hipLaunchKernelGGL(group_kl_bwd_row_kernel<false>, dim3(cy_blocks(npix, ROWS, 4096)), dim3(256), 0, st, logits,
                       target, gscale, dlogits, npix, K, m, eps);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_group_dice_counts(const float* logits, const int64_t* target, int64_t* counts, int N, int HW, int K, int G,
                         void* stream) {
  if (!logits || !target || !counts || N <= 0 || HW <= 0) return CY_ERR_ARG;
  if (K < 1 || K > KROW || G < 1 || K % G) return CY_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, (size_t)N * G * 2 * sizeof(int64_t), st) != hipSuccess) return CY_ERR_LAUNCH;
  const int m = K / G;
  if (K <= KMAX) {
    int bps = (HW + 255) / 256;
    if (bps > 64) bps = 64;
    hipLaunchKernelGGL(group_dice_counts_kernel, dim3(bps, N), dim3(256), 0, st, logits, target,
                       (unsigned long long*)counts, HW, K, G, m);
  } else {
    const int bps = cy_blocks(HW, ROWS, 256);
    if (K % 4 == 0)
      hipLaunchKernelGGL(group_dice_counts_row_kernel<true>, dim3(bps, N), dim3(256), 0, st, logits, target,
                         (unsigned long long*)counts, HW, K, G, m);
    else
      hipLaunchKernelGGL(group_dice_counts_row_kernel<false>, dim3(bps, N), dim3(256), 0, st, logits, target,
                         (unsigned long long*)counts, HW, K, G, m);
  }
  CY_CHECK_LAUNCH();
  return CY_OK;
}

}  // extern "C"
