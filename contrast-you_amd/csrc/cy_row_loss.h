// Helpers of the sixteen-lanes-per-pixel ("row") form of the pixel-wise loss kernels over [pixels][K] f32 logits,
// 16 < K <= 64 (cy_group_loss.hip, cy_mix_loss.hip): lane j of a row holds logits 4j..4j+3, absent ones as -inf;
// maximum and sums are reduced with __shfl_xor at offsets 8, 4, 2, 1, which never leave the aligned 16-lane row.
#pragma once
#include "cy_common.h"

namespace {

constexpr int KROW = 64;    // widest row of the cooperative form
constexpr int ROW = 16;     // lanes per pixel
constexpr int ROWS = 256 / ROW;  // pixels per block and iteration

__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int o = ROW / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float row_max(float v) {
#pragma unroll
  for (int o = ROW / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// logits k0..k0+3 of pixel p; channels >= K read as -inf.  VEC: K % 4 == 0, the rows are 16-byte aligned
template <bool VEC>
__device__ __forceinline__ void load_row4(const float* __restrict__ l, long p, int K, int k0, float* z) {
  const float ninf = -__builtin_inff();
  if (VEC) {
    if (k0 < K) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(l + p * K + k0);
      z[0] = v[0], z[1] = v[1], z[2] = v[2], z[3] = v[3];
    } else {
      z[0] = z[1] = z[2] = z[3] = ninf;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = (k0 + i < K) ? l[p * K + k0 + i] : ninf;
  }
}

template <bool VEC>
__device__ __forceinline__ void store_row4(float* __restrict__ d, long p, int K, int k0, const float* v) {
  if (VEC) {
    if (k0 < K) {
      f32x4 o;
      o[0] = v[0], o[1] = v[1], o[2] = v[2], o[3] = v[3];
      *reinterpret_cast<f32x4*>(d + p * K + k0) = o;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (k0 + i < K) d[p * K + k0 + i] = v[i];
  }
}

// e = exp(z - row maximum) (0 for absent channels); returns the row's sum of e
__device__ __forceinline__ float row_exp(const float* z, float* e) {
  const float m = row_max(fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3])));
#pragma unroll
  for (int i = 0; i < 4; ++i) e[i] = expf(z[i] - m);
  return row_sum((e[0] + e[1]) + (e[2] + e[3]));
}

// this lane's part of the sum of v over the channels [lo, hi)
__device__ __forceinline__ float part_in(const float* v, int k0, int lo, int hi) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (k0 + i >= lo && k0 + i < hi) s += v[i];
  return s;
}

}  // namespace
