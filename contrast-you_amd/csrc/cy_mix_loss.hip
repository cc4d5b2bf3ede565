// Pixel-wise loss and metric of the adaptive over-segmented criteria over [pixels][K] f32 logits: the K prototypes are
// mixed into C true classes by a dense [K][C] matrix M (softmax of the criteria's learnable "translation matrix").
//   AdaptiveOverSegmentedLoss, StricterAdaptiveOverSegmentedLoss(WithMI)   contrastyou/losses/multicore_loss.py:63-149
//   UniversalDice on the reduced arg-max                    semi_seg/epochers/features/multicore_epocher.py:64-67,84-91
//     R_c = sum_k p_k M[k,c], p = softmax(z);  loss = mean -log((R_t + eps) / (1 + eps))
//     dz_k = -(g/P) p_k (M[k,t] - R_t) / (R_t + eps);  dM[k,c] = -(g/P) sum_{pix: t = c} p_k / (R_t + eps)
// M is staged once per block in LDS, transposed and zero-padded: sm[c * KP + k], KP = 68, so that the four values a
// lane needs for class t are one 16-byte read and the classes start on different banks.
// The two forms of cy_group_loss.hip, chosen on the host:
//   thread form  K <= 16 (and, for the backward pass, at most 128 accumulators): one thread per pixel;
//   row form     sixteen lanes per pixel, lane j holds logits 4j..4j+3 (cy_row_loss.h); no barrier in the pixel loop,
//                rows past the end recompute the last pixel and contribute nothing.
// Nothing is summed with floating-point atomics.  Loss: one f64 partial per block + mean_finalize_kernel.  dM: every
// thread (lane) keeps [its channels][C] sums in registers, added under a `t == c` predicate; they are combined by
// __shfl_xor butterflies inside a wave, across the four waves through LDS in wave order, one [K][C] partial per block
// goes to the workspace, and mix_dm_finalize_kernel sums the blocks in a fixed order: two runs give the same bits.
// No multiply-add is formed that the source does not spell (fmaf), in this file and in the helpers it includes: the
// backward kernels with and without dM are different instantiations of one template and must give dlogits the same
// bits.
#pragma clang fp contract(off)

#include "cy_common.h"
#include "cy_pixel_loss.h"  // KMAX, load_logits
#include "cy_reduce.h"      // block_sum_d, mean_finalize_kernel, LOSS_GRID_CAP
#include "cy_row_loss.h"    // KROW, ROW, ROWS, row_sum, load_row4, store_row4, row_exp

namespace {

constexpr int CMIX = 16;           // most true classes
constexpr int KP = KROW + 4;       // pitch of one class's column of M in LDS
constexpr int DM_BLOCKS = 1024;    // most per-block dM partials

// sm[c * KP + k] = M[k][c], 0 outside [0, K) x [0, C)
__device__ __forceinline__ void stage_mix(float* sm, const float* __restrict__ mix, int K, int C) {
  for (int i = threadIdx.x; i < CMIX * KP; i += 256) {
    const int c = i / KP, k = i % KP;
    sm[i] = (c < C && k < K) ? mix[k * C + c] : 0.f;
  }
  __syncthreads();
}

// labels are in [0, C) by contract; an index outside never leaves the staged matrix
__device__ __forceinline__ int class_of(const int64_t* __restrict__ target, long p, int C) {
  const int t = (int)target[p];
  return t < 0 ? 0 : (t >= C ? C - 1 : t);
}

// thread form: e_k = exp(z_k - max z) for k < K, 0 beyond; returns their sum
__device__ __forceinline__ float thread_exp(const float* __restrict__ l, long p, int K, float* e) {
  float z[KMAX];
  load_logits(l, p, K, z);
  float m = z[0];
#pragma unroll
  for (int k = 1; k < KMAX; ++k)
    if (k < K) m = fmaxf(m, z[k]);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    e[k] = k < K ? expf(z[k] - m) : 0.f;
    s += e[k];
  }
  return s;
}

// thread form: mk = one class's column of M; returns sum_k e_k mk_k
__device__ __forceinline__ float col_dot(const float* col, const float* e, int K, float* mk) {
  float s = 0.f;
#pragma unroll
  for (int k4 = 0; k4 < KMAX; k4 += 4) {
    if (k4 < K) {
      const f32x4 m = *reinterpret_cast<const f32x4*>(col + k4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        mk[k4 + i] = m[i];
        s = fmaf(e[k4 + i], m[i], s);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) mk[k4 + i] = 0.f;
    }
  }
  return s;
}

// row form: m4 = M[k0..k0+3][c]; returns this lane's part of sum_k e_k M[k,c]
__device__ __forceinline__ float dot4(const float* col, int k0, const float* e, float* m4) {
  const f32x4 m = *reinterpret_cast<const f32x4*>(col + k0);
  m4[0] = m[0], m4[1] = m[1], m4[2] = m[2], m4[3] = m[3];
  return fmaf(e[3], m[3], fmaf(e[2], m[2], fmaf(e[1], m[1], e[0] * m[0])));
}

// sum over the lanes of a wave that differ in the bits FIRST, 2 FIRST, ..., 32 of the lane number
template <int FIRST>
__device__ __forceinline__ float wave_sum_from(float v) {
#pragma unroll
  for (int o = FIRST; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------- forward
__global__ void __launch_bounds__(256)
    mix_kl_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                      const float* __restrict__ mix, double* __restrict__ partial, long npix, int K, int C,
                      float eps) {
  __shared__ double sh[256];
  __shared__ __attribute__((aligned(16))) float sm[CMIX * KP];
  stage_mix(sm, mix, K, C);
  double acc = 0.0;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float e[KMAX], mk[KMAX];
    const float s = thread_exp(logits, p, K, e);
    const float R = col_dot(sm + class_of(target, p, C) * KP, e, K, mk) / s;
    acc += (double)(-logf((R + eps) / (1.f + eps)));
  }
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

template <bool VEC>
__global__ void __launch_bounds__(256)
    mix_kl_fwd_row_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                          const float* __restrict__ mix, double* __restrict__ partial, long npix, int K, int C,
                          float eps) {
  __shared__ double sh[256];
  __shared__ __attribute__((aligned(16))) float sm[CMIX * KP];
  stage_mix(sm, mix, K, C);
  const int r = threadIdx.x / ROW, k0 = 4 * (threadIdx.x % ROW);
  double acc = 0.0;
  for (long base = (long)blockIdx.x * ROWS; base < npix; base += (long)gridDim.x * ROWS) {
    const bool live = base + r < npix;
    const long p = live ? base + r : npix - 1;
    float z[4], e[4], m4[4];
    load_row4<VEC>(logits, p, K, k0, z);
    const float s = row_exp(z, e);
    const float R = row_sum(dot4(sm + class_of(target, p, C) * KP, k0, e, m4)) / s;
    if (live && k0 == 0) acc += (double)(-logf((R + eps) / (1.f + eps)));
  }
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// ---------------------------------------------------------------- backward
// CB = 0: dlogits only.  CB > 0: C <= CB, and the block's [K][C] sums of p_k / (R_t + eps) go to dm_part[blockIdx.x].
template <int KB, int CB>
__global__ void __launch_bounds__(256)
    mix_kl_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                      const float* __restrict__ mix, const float* __restrict__ gscale, float* __restrict__ dlogits,
                      float* __restrict__ dm_part, long npix, int K, int C, float eps) {
  constexpr int CA = CB > 0 ? CB : 1;
  __shared__ __attribute__((aligned(16))) float sm[CMIX * KP];
  __shared__ float sred[4 * KB * CA];
  stage_mix(sm, mix, K, C);
  const float gs = gscale[0] / (float)npix;
  float acc[KB][CA];
#pragma unroll
  for (int k = 0; k < KB; ++k)
#pragma unroll
    for (int c = 0; c < CA; ++c) acc[k][c] = 0.f;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float e[KMAX], mk[KMAX];
    const float inv = 1.f / thread_exp(logits, p, K, e);
    const int t = class_of(target, p, C);
    const float R = col_dot(sm + t * KP, e, K, mk) * inv;
    const float rinv = 1.f / (R + eps);
    const float coef = -gs * rinv;
    if (K == 4) {
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = coef * (e[k] * inv) * (mk[k] - R);
      *reinterpret_cast<f32x4*>(dlogits + p * 4) = o;
    } else {
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) dlogits[p * K + k] = coef * (e[k] * inv) * (mk[k] - R);
    }
    if (CB > 0) {
      const float w = inv * rinv;
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        const float v = e[k] * w;
#pragma unroll
        for (int c = 0; c < CA; ++c) acc[k][c] += (t == c) ? v : 0.f;
      }
    }
  }
  if (CB > 0) {
    const int wave = threadIdx.x / 64;
#pragma unroll
    for (int k = 0; k < KB; ++k)
#pragma unroll
      for (int c = 0; c < CA; ++c) {
        const float v = wave_sum_from<1>(acc[k][c]);
        if (threadIdx.x % 64 == 0) sred[(wave * KB + k) * CA + c] = v;
      }
    __syncthreads();
    if ((int)threadIdx.x < K * C) {
      const int k = threadIdx.x / C, c = threadIdx.x % C;
      float v = sred[k * CA + c];
#pragma unroll
      for (int w = 1; w < 4; ++w) v += sred[(w * KB + k) * CA + c];
      dm_part[(size_t)blockIdx.x * K * C + threadIdx.x] = v;
    }
  }
}

template <bool VEC, int CB>
__global__ void __launch_bounds__(256)
    mix_kl_bwd_row_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                          const float* __restrict__ mix, const float* __restrict__ gscale,
                          float* __restrict__ dlogits, float* __restrict__ dm_part, long npix, int K, int C,
                          float eps) {
  constexpr int CA = CB > 0 ? CB : 1;
  __shared__ __attribute__((aligned(16))) float sm[CMIX * KP];
  __shared__ float sred[CB > 0 ? 4 * KROW * CA : 1];
  stage_mix(sm, mix, K, C);
  const float gs = gscale[0] / (float)npix;
  const int r = threadIdx.x / ROW, k0 = 4 * (threadIdx.x % ROW);
  float acc[4][CA];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < CA; ++c) acc[i][c] = 0.f;
  for (long base = (long)blockIdx.x * ROWS; base < npix; base += (long)gridDim.x * ROWS) {
    const bool live = base + r < npix;
    const long p = live ? base + r : npix - 1;
    float z[4], e[4], m4[4], d[4];
    load_row4<VEC>(logits, p, K, k0, z);
    const float inv = 1.f / row_exp(z, e);
    const int t = class_of(target, p, C);
    const float R = row_sum(dot4(sm + t * KP, k0, e, m4)) * inv;
    const float rinv = 1.f / (R + eps);
    const float coef = -gs * rinv;
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = coef * (e[i] * inv) * (m4[i] - R);
    if (live) store_row4<VEC>(dlogits, p, K, k0, d);
    if (CB > 0) {
      const float w = live ? inv * rinv : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = e[i] * w;
#pragma unroll
        for (int c = 0; c < CA; ++c) acc[i][c] += (t == c) ? v : 0.f;
      }
    }
  }
  if (CB > 0) {
    // the four rows of a wave hold the same channels in lanes j, j + 16, j + 32, j + 48
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < CA; ++c) {
        const float v = wave_sum_from<ROW>(acc[i][c]);
        if (lane < ROW) sred[(wave * KROW + k0 + i) * CA + c] = v;
      }
    __syncthreads();
    for (int idx = threadIdx.x; idx < K * C; idx += 256) {
      const int k = idx / C, c = idx % C;
      float v = sred[k * CA + c];
#pragma unroll
      for (int w = 1; w < 4; ++w) v += sred[(w * KROW + k) * CA + c];
      dm_part[(size_t)blockIdx.x * K * C + idx] = v;
    }
  }
}

// dmix[e] = -(gscale / npix) * sum over the blocks' partials.  A block of 16 waves owns 64 consecutive entries, lane l
// entry 64 blockIdx.x + l, so a wave reads 256 contiguous bytes of one partial; wave w adds blocks w, w + 16, ... in
// f64, then the waves are added through LDS in wave order.
constexpr int FIN_WAVES = 16;
__global__ void __launch_bounds__(64 * FIN_WAVES)
    mix_dm_finalize_kernel(const float* __restrict__ dm_part, int nblk, int KC, const float* __restrict__ gscale,
                           double npix, float* __restrict__ dmix) {
  __shared__ double sh[FIN_WAVES][64];
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64, e = blockIdx.x * 64 + lane;
  double a = 0.0;
  if (e < KC)
    for (int b = wave; b < nblk; b += FIN_WAVES) a += (double)dm_part[(size_t)b * KC + e];
  sh[wave][lane] = a;
  __syncthreads();
  if (wave == 0 && e < KC) {
#pragma unroll
    for (int w = 1; w < FIN_WAVES; ++w) a += sh[w][lane];
    dmix[e] = (float)(-(double)gscale[0] / npix * a);
  }
}

// ---------------------------------------------------------------- dice counts on the reduced arg-max
// grid (blocks_per_sample, N).  The predicted class is the first maximal sum_k exp(z_k - max z) M[k,c].
__global__ void __launch_bounds__(256)
    mix_dice_counts_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                           const float* __restrict__ mix, unsigned long long* __restrict__ counts, int HW, int K,
                           int C) {
  __shared__ unsigned int sc[CMIX * 2];
  __shared__ __attribute__((aligned(16))) float sm[CMIX * KP];
  const int n = blockIdx.y;
  if (threadIdx.x < CMIX * 2) sc[threadIdx.x] = 0u;
  stage_mix(sm, mix, K, C);
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const long gp = (long)n * HW + p;
    float e[KMAX], mk[KMAX];
    thread_exp(logits, gp, K, e);
    int best = 0;
    float bv = -1.f;
    for (int c = 0; c < C; ++c) {
      const float s = col_dot(sm + c * KP, e, K, mk);
      if (s > bv) bv = s, best = c;
    }
    const int t = (int)target[gp];
    if (best == t) atomicAdd(&sc[best * 2 + 0], 1u);
    atomicAdd(&sc[best * 2 + 1], 1u);
    if (t >= 0 && t < C) atomicAdd(&sc[t * 2 + 1], 1u);
  }
  __syncthreads();
  if ((int)threadIdx.x < C * 2 && sc[threadIdx.x])
    atomicAdd(&counts[(size_t)n * C * 2 + threadIdx.x], (unsigned long long)sc[threadIdx.x]);
}

template <bool VEC>
__global__ void __launch_bounds__(256)
    mix_dice_counts_row_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                               const float* __restrict__ mix, unsigned long long* __restrict__ counts, int HW,
                               int K, int C) {
  __shared__ unsigned int sc[CMIX * 2];
  __shared__ __attribute__((aligned(16))) float sm[CMIX * KP];
  const int n = blockIdx.y;
  if (threadIdx.x < CMIX * 2) sc[threadIdx.x] = 0u;
  stage_mix(sm, mix, K, C);
  const int r = threadIdx.x / ROW, k0 = 4 * (threadIdx.x % ROW);
  for (int base = blockIdx.x * ROWS; base < HW; base += gridDim.x * ROWS) {
    const bool live = base + r < HW;
    const long gp = (long)n * HW + (live ? base + r : HW - 1);
    float z[4], e[4], m4[4];
    load_row4<VEC>(logits, gp, K, k0, z);
    row_exp(z, e);
    int best = 0;
    float bv = -1.f;
    for (int c = 0; c < C; ++c) {  // every lane of the row ends with the same (bv, best)
      const float s = row_sum(dot4(sm + c * KP, k0, e, m4));
      if (s > bv) bv = s, best = c;
    }
    if (live && k0 == 0) {
      const int t = (int)target[gp];
      if (best == t) atomicAdd(&sc[best * 2 + 0], 1u);
      atomicAdd(&sc[best * 2 + 1], 1u);
      if (t >= 0 && t < C) atomicAdd(&sc[t * 2 + 1], 1u);
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < C * 2 && sc[threadIdx.x])
    atomicAdd(&counts[(size_t)n * C * 2 + threadIdx.x], (unsigned long long)sc[threadIdx.x]);
}

inline int mix_kl_blocks(long npix, int K) {
  return K <= KMAX ? cy_blocks(npix, 256, LOSS_GRID_CAP) : cy_blocks(npix, ROWS, 1024);
}

inline int bucket(int v) { return v <= 4 ? 4 : (v <= 8 ? 8 : 16); }

// the backward pass takes the thread form where its [K][C] sums fit 128 registers, with or without dmix: dlogits has
// the same bits either way
inline bool bwd_thread_form(int K, int C) { return K <= KMAX && bucket(K) * bucket(C) <= 128; }

#define MIX_BWD_ARGS logits, target, mix, gscale, dlogits, (float*)ws, npix, K, C, eps
#define MIX_BWD_THREAD(KB, CB) \
  hipLaunchKernelGGL((mix_kl_bwd_kernel<KB, CB>), dim3(nblk), dim3(256), 0, st, MIX_BWD_ARGS)
#define MIX_BWD_ROW(VEC, CB) \
  hipLaunchKernelGGL((mix_kl_bwd_row_kernel<VEC, CB>), dim3(nblk), dim3(256), 0, st, MIX_BWD_ARGS)

}  // namespace

extern "C" {

size_t cy_softmax_mix_kl_ws_bytes(long npix, int K) { return (size_t)mix_kl_blocks(npix, K) * sizeof(double); }

int cy_softmax_mix_kl_fwd(const float* logits, const int64_t* target, const float* mix, float* loss, long npix, int K,
                          int C, float eps, void* ws, size_t ws_bytes, void* stream) {
  if (!logits || !target || !mix || !loss || !ws || npix <= 0) return CY_ERR_ARG;
  if (K < 1 || K > KROW || C < 1 || C > CMIX) return CY_ERR_SHAPE;
  if (ws_bytes < cy_softmax_mix_kl_ws_bytes(npix, K)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = mix_kl_blocks(npix, K);
  if (K <= KMAX)
    hipLaunchKernelGGL(mix_kl_fwd_kernel, dim3(nblk), dim3(256), 0, st, logits, target, mix, (double*)ws, npix, K, C,
                       eps);
  else if (K % 4 == 0)
    hipLaunchKernelGGL(mix_kl_fwd_row_kernel<true>, dim3(nblk), dim3(256), 0, st, logits, target, mix, (double*)ws,
                       npix, K, C, eps);
  else
    hipLaunchKernelGGL(mix_kl_fwd_row_kernel<false>, dim3(nblk), dim3(256), 0, st, logits, target, mix, (double*)ws,
                       npix, K, C, eps);
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(mean_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, nblk, (double)npix, loss);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

size_t cy_softmax_mix_kl_bwd_ws_bytes(long npix, int K, int C) {
  if (npix < 1 || K < 1 || C < 1) return 0;
  return (size_t)cy_blocks(npix, ROWS, DM_BLOCKS) * K * C * sizeof(float);
}

int cy_softmax_mix_kl_bwd(const float* logits, const int64_t* target, const float* mix, const float* gscale,
                          float* dlogits, float* dmix, long npix, int K, int C, float eps, void* ws, size_t ws_bytes,
                          void* stream) {
  if (!logits || !target || !mix || !gscale || !dlogits || (dmix && !ws) || npix <= 0) return CY_ERR_ARG;
  if (K < 1 || K > KROW || C < 1 || C > CMIX) return CY_ERR_SHAPE;
  if (dmix && ws_bytes < cy_softmax_mix_kl_bwd_ws_bytes(npix, K, C)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const bool thread_form = bwd_thread_form(K, C), vec = K % 4 == 0;
  int nblk;
  if (!dmix) {
    if (thread_form) {
      nblk = cy_blocks(npix, 256, LOSS_GRID_CAP) * 2;
      MIX_BWD_THREAD(KMAX, 0);
    } else {
      nblk = cy_blocks(npix, ROWS, 4096);
      if (vec) MIX_BWD_ROW(true, 0); else MIX_BWD_ROW(false, 0);
    }
    CY_CHECK_LAUNCH();
    return CY_OK;
  }
  // nblk <= cy_blocks(npix, ROWS, DM_BLOCKS), the count behind cy_softmax_mix_kl_bwd_ws_bytes
  if (thread_form) {
    nblk = cy_blocks(npix, 256, LOSS_GRID_CAP);
    switch (bucket(K) * 100 + bucket(C)) {
      case 404: MIX_BWD_THREAD(4, 4); break;
      case 408: MIX_BWD_THREAD(4, 8); break;
      case 416: MIX_BWD_THREAD(4, 16); break;
      case 804: MIX_BWD_THREAD(8, 4); break;
      case 808: MIX_BWD_THREAD(8, 8); break;
      case 816: MIX_BWD_THREAD(8, 16); break;
      case 1604: MIX_BWD_THREAD(16, 4); break;
      default: MIX_BWD_THREAD(16, 8); break;
    }
  } else {
    nblk = cy_blocks(npix, ROWS, DM_BLOCKS);
    switch (bucket(C) + (vec ? 100 : 0)) {
      case 104: MIX_BWD_ROW(true, 4); break;
      case 108: MIX_BWD_ROW(true, 8); break;
      case 116: MIX_BWD_ROW(true, 16); break;
      case 4: MIX_BWD_ROW(false, 4); break;
      case 8: MIX_BWD_ROW(false, 8); break;
      default: MIX_BWD_ROW(false, 16); break;
    }
  }
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(mix_dm_finalize_kernel, dim3((K * C + 63) / 64), dim3(64 * FIN_WAVES), 0, st, (const float*)ws,
                     nblk, K * C, gscale, (double)npix, dmix);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_mix_dice_counts(const float* logits, const int64_t* target, const float* mix, int64_t* counts, int N, int HW,
                       int K, int C, void* stream) {
  if (!logits || !target || !mix || !counts || N <= 0 || HW <= 0) return CY_ERR_ARG;
  if (K < 1 || K > KROW || C < 1 || C > CMIX) return CY_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, (size_t)N * C * 2 * sizeof(int64_t), st) != hipSuccess) return CY_ERR_LAUNCH;
  if (K <= KMAX) {
    int bps = (HW + 255) / 256;
    if (bps > 64) bps = 64;
    hipLaunchKernelGGL(mix_dice_counts_kernel, dim3(bps, N), dim3(256), 0, st, logits, target, mix,
                       (unsigned long long*)counts, HW, K, C);
  } else {
    const int bps = cy_blocks(HW, ROWS, 256);
    if (K % 4 == 0)
      hipLaunchKernelGGL(mix_dice_counts_row_kernel<true>, dim3(bps, N), dim3(256), 0, st, logits, target, mix,
                         (unsigned long long*)counts, HW, K, C);
    else
      hipLaunchKernelGGL(mix_dice_counts_row_kernel<false>, dim3(bps, N), dim3(256), 0, st, logits, target, mix,
                         (unsigned long long*)counts, HW, K, C);
  }
  CY_CHECK_LAUNCH();
  return CY_OK;
}

}  // extern "C"
