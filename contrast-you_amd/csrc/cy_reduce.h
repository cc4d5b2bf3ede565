// Reductions shared by the kernels: wave64 shuffles, the fixed tree over a 256-thread workgroup, and the ordered sum
// of per-block f64 partials that ends every loss.  Each exists once: the determinism of the losses ("two runs give the
// same bits") rests on the order of these sums.
#pragma once
#include "cy_common.h"

namespace {

// ---- wave64, all lanes (result in every lane); xor offsets 32 .. 1
template <typename T> __device__ __forceinline__ T wave_sum(T v) {  // float, double, int
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- 256-thread workgroup: sh[tid] = op(sh[tid], sh[tid + o]) for o = 128, 64, .., 1 over sh[256].
// One convention for every caller: a barrier before the first LDS write and one after the last read, so `sh` may hold
// anything before the call and be reused right after it; the result is in every thread.  All 256 threads must call.
template <typename T, typename Op> __device__ __forceinline__ T block_tree(T v, T* sh /* [256] */, Op op) {
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sh[tid] = op(sh[tid], sh[tid + o]);
    __syncthreads();
  }
  const T r = sh[0];
  __syncthreads();
  return r;
}
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
  return block_tree(v, sh, [](double a, double b) { return a + b; });
}
__device__ __forceinline__ double block_min_d(double v, double* sh) {
  return block_tree(v, sh, [](double a, double b) { return fmin(a, b); });
}
__device__ __forceinline__ float block_sum_f(float v, float* sh) {
  return block_tree(v, sh, [](float a, float b) { return a + b; });
}
__device__ __forceinline__ float block_max_f(float v, float* sh) {
  return block_tree(v, sh, [](float a, float b) { return fmaxf(a, b); });
}

// ---- per-block partials: thread t adds p[i * stride] for i = t, t + 256, .. in that order, then the tree
__device__ __forceinline__ double sum_partials_d(const double* p, int n, long stride, double* sh /* [256] */) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += p[i * stride];
  return block_sum_d(acc, sh);
}

// grid cap of the loss kernels that leave one partial per block of 256 items: it bounds their workspace (8 KiB of
// partials) and the one-block sum above (four partials per thread)
constexpr int LOSS_GRID_CAP = 1024;

// loss[0] = (sum of the nblk partials) / denom; one block
__global__ void __launch_bounds__(256)
    mean_finalize_kernel(const double* __restrict__ partial, int nblk, double denom,
                         float* __restrict__ loss) {
  __shared__ double sh[256];
  const double tot = sum_partials_d(partial, nblk, 1, sh);
  if (threadIdx.x == 0) loss[0] = (float)(tot / denom);
}

// the end of the UA-MT forward in both of its forms (cy_pixel_reg.hip, cy_wide_reg.hip): partial holds (sum, count) per
// block; out[0] = (S1 / P) / (S2 / P + 1e-2), out[1] = S2 / P
constexpr double UAMT_DENOM_EPS = 1e-2;  // mt.py:246: loss.mean() / (mask.mean().item() + 1e-2)
__global__ void __launch_bounds__(256)
    uamt_finalize_kernel(const double* __restrict__ partial, int nblk, double npix, float* __restrict__ out) {
  __shared__ double sh1[256], sh2[256];
  const double s1 = sum_partials_d(partial, nblk, 2, sh1);
  const double s2 = sum_partials_d(partial + 1, nblk, 2, sh2);
  if (threadIdx.x == 0) {
    const float mask_mean = (float)(s2 / npix);
    out[0] = (float)((s1 / npix) / ((double)mask_mean + UAMT_DENOM_EPS));
    out[1] = mask_mean;
  }
}

}  // namespace
