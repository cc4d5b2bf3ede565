// Helpers of the pixel-wise loss kernels over [pixels][K] f32 logits (cy_head_loss.hip, cy_pixel_reg.hip):
// one thread per pixel, grid-stride; per-block f64 partials summed by a one-block finalize launch in a fixed order.
#pragma once
#include "cy_common.h"

namespace {

constexpr int KMAX = 16;  // segmentation classes

__device__ __forceinline__ void softmax_k(const float* z, float* p, int K) {
  float m = z[0];
#pragma unroll
  for (int k = 1; k < KMAX; ++k)
    if (k < K) m = fmaxf(m, z[k]);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      p[k] = expf(z[k] - m);
      s += p[k];
    }
  const float inv = 1.f / s;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) p[k] *= inv;
}

__device__ __forceinline__ void load_logits(const float* l, long p, int K, float* z) {
  if (K == 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(l + p * 4);
    z[0] = v[0], z[1] = v[1], z[2] = v[2], z[3] = v[3];
  } else {
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) z[k] = l[p * K + k];
  }
}

__device__ __forceinline__ double block_sum_d(double v, double* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sh[tid] += sh[tid + o];
    __syncthreads();
  }
  return sh[0];
}

__global__ void __launch_bounds__(256)
    mean_finalize_kernel(const double* __restrict__ partial, int nblk, double denom,
                         float* __restrict__ loss) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) acc += partial[i];
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) loss[0] = (float)(tot / denom);
}

inline int loss_blocks(long npix) {
  long b = (npix + 255) / 256;
  if (b > 1024) b = 1024;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace
