// Helpers of the pixel-wise loss kernels over [pixels][K] f32 logits (cy_head_loss.hip, cy_pixel_reg.hip,
// cy_seg_loss.hip):
// one thread per pixel, grid-stride: the logits rows and their softmax.  The per-block f64 partials, their one-block
// finalize launch and the block count are in cy_reduce.h.
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

// KT > 0: K known at compile time (the loops of the shared helpers fold); KT == 0: run-time K
template <int KT> __device__ __forceinline__ void load_row(const float* l, long p, int K, float* z) {
  if constexpr (KT == 2) {
    const f32x2 v = *reinterpret_cast<const f32x2*>(l + p * 2);
    z[0] = v[0], z[1] = v[1];
  } else if constexpr (KT == 8) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(l + p * 8);
    const f32x4 b = *reinterpret_cast<const f32x4*>(l + p * 8 + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) z[k] = a[k], z[4 + k] = b[k];
  } else {
    load_logits(l, p, K, z);  // (16 bytes at K == 4)
  }
}

template <int KT> __device__ __forceinline__ void store_row(float* d, long p, int K, const float* v) {
  if constexpr (KT == 2) {
    f32x2 o;
    o[0] = v[0], o[1] = v[1];
    *reinterpret_cast<f32x2*>(d + p * 2) = o;
  } else if constexpr (KT == 4 || KT == 8) {
#pragma unroll
    for (int q = 0; q < KT / 4; ++q) {
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = v[4 * q + k];
      *reinterpret_cast<f32x4*>(d + p * KT + 4 * q) = o;
    }
  } else {
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) d[p * K + k] = v[k];
  }
}

// launch `KERNEL<KT>` with KT = K for the compiled class counts, 0 otherwise
#define CY_LAUNCH_BY_K(KERNEL, GRID, ST, ...)                                          \
  do {                                                                                 \
    if (K == 2)                                                                        \
      hipLaunchKernelGGL(KERNEL<2>, dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);        \
    else if (K == 4)                                                                   \
      hipLaunchKernelGGL(KERNEL<4>, dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);        \
    else if (K == 8)                                                                   \
      hipLaunchKernelGGL(KERNEL<8>, dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);        \
    else                                                                               \
      hipLaunchKernelGGL(KERNEL<0>, dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);        \
    CY_CHECK_LAUNCH();                                                                 \
  } while (0)

}  // namespace
