// Two small regularisers of the semi-supervised step.
//   DAE prior:   F.mse_loss(act(conv1x1_{K->1}(logits)), image)                semi_seg/hooks/autoencoder.py:52-57
//   orthogonal:  ((n n^T - I)^2).mean(), n = F.normalize(prototypes)           semi_seg/hooks/orthogonal.py:45-50
// DAE is of the family of cy_pixel_reg.hip: logits are [npix][K] f32 rows, one thread per pixel, grid-stride, one f64
// partial per block, a fixed-order finalize, no atomics.  The pre-activation is summed in f64 over the row, 16 floats
// at a time, so no K-long register array exists for any K <= 64; K = 2, 4, 8 on aligned rows are compiled with K known.
// The backward recomputes r per pixel, parks the pixel's coefficient g_p in LDS and then sweeps the block's 256 x K
// tile flat: the working threads are the largest multiple of K up to 256, so a thread keeps its class k, w_k and its
// share of dw_k are one register each, and the store of dlogits is contiguous for any K.  dw and db leave through
// [K + 1][blocks] f64 partials that K + 1 blocks sum in block order.
// The orthogonality loss is a K x C problem (K * C <= 16384): one block holds the normalised rows in LDS, forms the
// Gram matrix in f64 -- a thread per entry for short rows, a wave per entry for long ones -- and, backward, recomputes
// all of it and writes dV; nothing is saved but the input.
#include "cy_common.h"
#include "cy_reduce.h"

namespace {

constexpr int PRIOR_KMAX = 64;       // classes of the DAE logits, prototypes of the orthogonality loss
constexpr int DAE_CHUNK = 16;        // floats of a row in flight per thread
constexpr int DAE_CIMG_MAX = 4;      // the U-Net's input_dim limit
constexpr int ORTHO_ELEMS = 16384;   // K * C: 64 KB of f32 in LDS
constexpr int ORTHO_WAVE_C = 64;     // rows longer than this take a wave per Gram entry
constexpr float ORTHO_EPS = 1e-12f;  // F.normalize's clamp

// ---------------------------------------------------------------- DAE
template <int ACT> __device__ __forceinline__ float dae_act(float s) {
  if constexpr (ACT == CY_PRIOR_ACT_TANH)
    return tanhf(s);
  else
    return 1.f / (1.f + expf(-s));
}

// act'(s) from r = act(s)
template <int ACT> __device__ __forceinline__ float dae_dact(float r) {
  if constexpr (ACT == CY_PRIOR_ACT_TANH)
    return 1.f - r * r;
  else
    return r * (1.f - r);
}

// b + sum_k w_k z_k of one row, in f64.  VEC: floats per access (2: K == 2; 4: K % 4 == 0; both on aligned rows)
template <int KT, int VEC>
__device__ __forceinline__ float dae_pre(const float* __restrict__ row, const float* sw, int K, float b) {
  double s = (double)b;
  if constexpr (VEC == 2) {
    const f32x2 v = *reinterpret_cast<const f32x2*>(row);
    s = fma((double)v[0], (double)sw[0], s);
    s = fma((double)v[1], (double)sw[1], s);
  } else if constexpr (VEC == 4) {
    for (int k0 = 0; k0 < K; k0 += DAE_CHUNK) {
#pragma unroll
      for (int q = 0; q < DAE_CHUNK; q += 4)
        if (k0 + q < K) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(row + k0 + q);
#pragma unroll
          for (int j = 0; j < 4; ++j) s = fma((double)v[j], (double)sw[k0 + q + j], s);
        }
    }
  } else {
    for (int k0 = 0; k0 < K; k0 += DAE_CHUNK) {
#pragma unroll
      for (int q = 0; q < DAE_CHUNK; ++q)
        if (k0 + q < K) s = fma((double)row[k0 + q], (double)sw[k0 + q], s);
    }
  }
  return (float)s;
}

// sum_c (r - img_c) and sum_c (r - img_c)^2 of pixel p; the image is [N][Cimg][HW] planar
__device__ __forceinline__ void dae_diff(const float* __restrict__ img, long p, long HW, int Cimg, float r, float* d1,
                                         float* d2) {
  const long n = p / HW;
  const float* px = img + n * Cimg * HW + (p - n * HW);
  float a = 0.f, q = 0.f;
  for (int c = 0; c < Cimg; ++c) {
    const float d = r - px[c * HW];
    a += d;
    q = fmaf(d, d, q);
  }
  *d1 = a, *d2 = q;
}

template <int KT, int VEC, int ACT>
__global__ void __launch_bounds__(256)
    dae_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ w, const float* __restrict__ b,
                   const float* __restrict__ img, double* __restrict__ partial, long npix, long HW, int Krt, int Cimg) {
  const int K = KT ? KT : Krt;
  __shared__ double sh[256];
  __shared__ float sw[PRIOR_KMAX];
  if (threadIdx.x < K) sw[threadIdx.x] = w[threadIdx.x];
  __syncthreads();
  const float bias = b[0];
  double acc = 0.0;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    const float r = dae_act<ACT>(dae_pre<KT, VEC>(logits + p * K, sw, K, bias));
    float d1, d2;
    dae_diff(img, p, HW, Cimg, r, &d1, &d2);
    acc += (double)d2;
  }
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// partial: [K + 1][gridDim.x] f64 -- rows 0..K-1 the block's share of dw, row K of db
template <int KT, int VEC, int ACT>
__global__ void __launch_bounds__(256)
    dae_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ w, const float* __restrict__ b,
                   const float* __restrict__ img, const float* __restrict__ gscale, float* __restrict__ dlogits,
                   double* __restrict__ partial, long npix, long HW, int Krt, int Cimg) {
  const int K = KT ? KT : Krt;
  __shared__ double sh[256];
  __shared__ float sw[PRIOR_KMAX];
  __shared__ float sg[256];
  const int tid = threadIdx.x;
  if (tid < K) sw[tid] = w[tid];
  __syncthreads();
  const float bias = b[0];
  const float gs = (float)(2.0 * (double)gscale[0] / ((double)npix * (double)Cimg));
  const int per = 256 / K, T = per * K;  // working threads of the sweep: thread t < T keeps class t % K
  const int k_own = tid % K, row_own = tid / K;
  const float w_own = sw[k_own];
  double acc_w = 0.0, acc_b = 0.0;
  for (long p0 = blockIdx.x * 256L; p0 < npix; p0 += (long)gridDim.x * 256L) {
    const long p = p0 + tid;
    float g = 0.f;
    if (p < npix) {
      const float r = dae_act<ACT>(dae_pre<KT, VEC>(logits + p * K, sw, K, bias));
      float d1, d2;
      dae_diff(img, p, HW, Cimg, r, &d1, &d2);
      g = gs * dae_dact<ACT>(r) * d1;
    }
    sg[tid] = g;
    acc_b += (double)g;
    __syncthreads();
    const long rest = npix - p0;
    const int rows = rest < 256 ? (int)rest : 256;
    const int nelem = rows * K;
    const long base = p0 * K;
    if (tid < T) {
      int row = row_own;
      for (int e = tid; e < nelem; e += T, row += per) {
        const float gp = sg[row];
        dlogits[base + e] = gp * w_own;
        acc_w = fma((double)gp, (double)logits[base + e], acc_w);
      }
    }
    __syncthreads();
  }
  sh[tid] = tid < T ? acc_w : 0.0;
  __syncthreads();
  if (tid < K) {
    double s = 0.0;
    for (int q = tid; q < T; q += K) s += sh[q];
    partial[(long)tid * gridDim.x + blockIdx.x] = s;
  }
  const double tot = block_sum_d(acc_b, sh);
  if (tid == 0) partial[(long)K * gridDim.x + blockIdx.x] = tot;
}

// block k sums row k of partial [K + 1][nblk] in block order: k < K -> dw[k], k == K -> db[0]
__global__ void __launch_bounds__(256)
    dae_param_finalize_kernel(const double* __restrict__ partial, int nblk, int K, float* __restrict__ dw,
                              float* __restrict__ db) {
  __shared__ double sh[256];
  const int k = blockIdx.x;
  const double tot = sum_partials_d(partial + (long)k * nblk, nblk, 1, sh);
  if (threadIdx.x == 0) {
    if (k < K)
      dw[k] = (float)tot;
    else
      db[0] = (float)tot;
  }
}

// ---------------------------------------------------------------- orthogonality
// rows into LDS, their norms (snorm: the 2-norm, sden: clamped as F.normalize clamps it), then n = v / sden in place
__device__ __forceinline__ void ortho_normalise(const float* __restrict__ V, float* sN, float* snorm, float* sden, int K,
                                                int C, int stride) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int total = K * C;
  for (int e = tid; e < total; e += 256) {
    const int i = e / C;
    sN[i * stride + (e - i * C)] = V[e];
  }
  __syncthreads();
  for (int i = wave; i < K; i += 4) {
    double ss = 0.0;
    for (int c = lane; c < C; c += 64) {
      const double v = (double)sN[i * stride + c];
      ss = fma(v, v, ss);
    }
    ss = wave_sum(ss);
    if (lane == 0) {
      const float nrm = (float)sqrt(ss);
      snorm[i] = nrm;
      sden[i] = fmaxf(nrm, ORTHO_EPS);
    }
  }
  __syncthreads();
  for (int e = tid; e < total; e += 256) {
    const int i = e / C;
    const int at = i * stride + (e - i * C);
    sN[at] = sN[at] / sden[i];
  }
  __syncthreads();
}

// visits every entry (i, j) of G - I once, in f64: `f(e, d)` runs in one thread per entry, e = i * K + j
template <int WAVE, typename F>
__device__ __forceinline__ void ortho_gram(const float* sN, int K, int C, int stride, F f) {
  const int tid = threadIdx.x, KK = K * K;
  if constexpr (WAVE) {
    const int lane = tid & 63;
    for (int e = tid >> 6; e < KK; e += 4) {
      const int i = e / K, j = e - i * K;
      double dot = 0.0;
      for (int c = lane; c < C; c += 64) dot = fma((double)sN[i * stride + c], (double)sN[j * stride + c], dot);
      dot = wave_sum(dot);
      if (lane == 0) f(e, dot - (i == j ? 1.0 : 0.0));
    }
  } else {
    for (int e = tid; e < KK; e += 256) {
      const int i = e / K, j = e - i * K;
      double dot = 0.0;
      for (int c = 0; c < C; ++c) dot = fma((double)sN[i * stride + c], (double)sN[j * stride + c], dot);
      f(e, dot - (i == j ? 1.0 : 0.0));
    }
  }
}

template <int WAVE>
__global__ void __launch_bounds__(256)
    ortho_fwd_kernel(const float* __restrict__ V, float* __restrict__ loss, int K, int C, int stride) {
  extern __shared__ float smem[];
  __shared__ double sh[256];
  __shared__ float snorm[PRIOR_KMAX], sden[PRIOR_KMAX];
  float* sN = smem;  // [K][stride]
  ortho_normalise(V, sN, snorm, sden, K, C, stride);
  double acc = 0.0;
  ortho_gram<WAVE>(sN, K, C, stride, [&](int, double d) { acc = fma(d, d, acc); });
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) loss[0] = (float)(tot / ((double)K * (double)K));
}

// A = G - I;  dL/dn_i = (4 / K^2) sum_j A_ij n_j =: D_i;  n_i . D_i = (4 / K^2) sum_j A_ij G_ij =: t_i;
// dv_i = (D_i - n_i t_i) / max(|v_i|, eps), without the projection where the norm was clamped
template <int WAVE>
__global__ void __launch_bounds__(256)
    ortho_bwd_kernel(const float* __restrict__ V, const float* __restrict__ gscale, float* __restrict__ dV, int K, int C,
                     int stride) {
  extern __shared__ float smem[];
  __shared__ float snorm[PRIOR_KMAX], sden[PRIOR_KMAX], st[PRIOR_KMAX];
  float* sN = smem;              // [K][stride]
  float* sA = smem + K * stride; // [K][K]
  ortho_normalise(V, sN, snorm, sden, K, C, stride);
  ortho_gram<WAVE>(sN, K, C, stride, [&](int e, double d) { sA[e] = (float)d; });
  __syncthreads();
  const int tid = threadIdx.x;
  if (tid < K) {
    double t = 0.0;
    for (int j = 0; j < K; ++j) {
      const double a = (double)sA[tid * K + j];
      t = fma(a, a + (j == tid ? 1.0 : 0.0), t);
    }
    st[tid] = snorm[tid] > ORTHO_EPS ? (float)t : 0.f;
  }
  __syncthreads();
  const double gs = 4.0 * (double)gscale[0] / ((double)K * (double)K);
  const int total = K * C;
  for (int e = tid; e < total; e += 256) {
    const int i = e / C, c = e - i * C;
    double D = 0.0;
    for (int j = 0; j < K; ++j) D = fma((double)sA[i * K + j], (double)sN[j * stride + c], D);
    dV[e] = (float)(gs * (D - (double)sN[i * stride + c] * (double)st[i]) / (double)sden[i]);
  }
}

// ---------------------------------------------------------------- the launch rule
// the most dynamic LDS a launch asks for: the backward's rows and Gram matrix at K = 64, C = 256 (80 KB of the CU's 160)
constexpr int ORTHO_LDS_MAX = (ORTHO_ELEMS + PRIOR_KMAX * PRIOR_KMAX) * 4;

// the one place every launch takes its kernel form, grid and LDS from; a status as the launches return it, and nothing
// is written to `pl` before the last refusal
int prior_plan(int form, long n, int K, int C, int align, cy_prior_plan_t* pl) {
  if (!pl) return CY_ERR_ARG;
  if (form == CY_PRIOR_DAE) {
    if (n < 1 || align < 1 || align % 4 != 0) return CY_ERR_ARG;
    if (K < 2 || K > PRIOR_KMAX || C < 1 || C > DAE_CIMG_MAX) return CY_ERR_SHAPE;
    if (K == 2 && align % 8 == 0)
      pl->variant = 2, pl->vec = 2;
    else if ((K == 4 || K == 8) && align % 16 == 0)
      pl->variant = K, pl->vec = 4;
    else
      pl->variant = 0, pl->vec = (K % 4 == 0 && align % 16 == 0) ? 4 : 1;
    pl->k_chunks = pl->variant ? 1 : (K + DAE_CHUNK - 1) / DAE_CHUNK;
    pl->fwd_grid = pl->bwd_grid = cy_blocks(n, 256, LOSS_GRID_CAP);
    pl->fwd_trips = pl->bwd_trips = cy_trips(n, pl->fwd_grid, 256);
    pl->fwd_lds = 256 * 8 + PRIOR_KMAX * 4;
    pl->bwd_lds = pl->fwd_lds + 256 * 4;
    pl->aux = (256 / K) * K;
    return CY_OK;
  }
  if (form == CY_PRIOR_ORTHO) {
    if (C < 1) return CY_ERR_ARG;
    if (K < 2 || K > PRIOR_KMAX || (long)K * C > ORTHO_ELEMS) return CY_ERR_SHAPE;
    pl->variant = C > ORTHO_WAVE_C ? 1 : 0;
    pl->vec = 1;
    pl->fwd_grid = pl->bwd_grid = 1;
    pl->fwd_trips = pl->variant ? (K * K + 3) / 4 : (K * K + 255) / 256;  // of the Gram loop
    pl->bwd_trips = (K * C + 255) / 256;                                  // of the sweeps over [K][C]
    pl->k_chunks = 0;
    pl->aux = pl->variant ? C : (C | 1);  // floats between two rows in LDS (odd for the thread form: no bank conflicts)
    pl->fwd_lds = K * pl->aux * 4;
    pl->bwd_lds = pl->fwd_lds + K * K * 4;
    return CY_OK;
  }
  return CY_ERR_ARG;
}

#define CY_DAE_LAUNCH_ACT(KERNEL, KT_, VEC_, ACT_, GRID, ST, ...)                                                    \
  do {                                                                                                               \
    if ((ACT_) == CY_PRIOR_ACT_TANH)                                                                                 \
      hipLaunchKernelGGL((KERNEL<KT_, VEC_, CY_PRIOR_ACT_TANH>), dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);         \
    else                                                                                                             \
      hipLaunchKernelGGL((KERNEL<KT_, VEC_, CY_PRIOR_ACT_SIGMOID>), dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);      \
  } while (0)

// launch `KERNEL<variant, vec, act>` for the plan
#define CY_DAE_LAUNCH(KERNEL, PL, ACT_, GRID, ST, ...)                          \
  do {                                                                          \
    if ((PL).variant == 2)                                                      \
      CY_DAE_LAUNCH_ACT(KERNEL, 2, 2, ACT_, GRID, ST, __VA_ARGS__);             \
    else if ((PL).variant == 4)                                                 \
      CY_DAE_LAUNCH_ACT(KERNEL, 4, 4, ACT_, GRID, ST, __VA_ARGS__);             \
    else if ((PL).variant == 8)                                                 \
      CY_DAE_LAUNCH_ACT(KERNEL, 8, 4, ACT_, GRID, ST, __VA_ARGS__);             \
    else if ((PL).vec == 4)                                                     \
      CY_DAE_LAUNCH_ACT(KERNEL, 0, 4, ACT_, GRID, ST, __VA_ARGS__);             \
    else                                                                        \
      CY_DAE_LAUNCH_ACT(KERNEL, 0, 1, ACT_, GRID, ST, __VA_ARGS__);             \
    CY_CHECK_LAUNCH();                                                          \
  } while (0)

inline size_t dae_ws_bytes(long npix, int K, int backward) {
  if (npix < 1 || K < 1) return 0;
  return (size_t)cy_blocks(npix, 256, LOSS_GRID_CAP) * sizeof(double) * (backward ? (size_t)K + 1 : 1);
}

inline bool dae_act_ok(int act) { return act == CY_PRIOR_ACT_SIGMOID || act == CY_PRIOR_ACT_TANH; }

}  // namespace

extern "C" {

int cy_prior_plan(int form, long n, int K, int C, int align, cy_prior_plan_t* out) {
  return prior_plan(form, n, K, C, align, out);  // (a NULL `out` is the rule's first refusal)
}

size_t cy_dae_ws_bytes(long npix, int K, int backward) { return dae_ws_bytes(npix, K, backward); }

int cy_dae_fwd(const float* logits, const float* w, const float* b, const float* image, float* loss, int N, long HW,
               int K, int Cimg, int act, void* ws, size_t ws_bytes, void* stream) {
  if (!logits || !w || !b || !image || !loss || !ws || N < 1 || HW < 1) return CY_ERR_ARG;
  const long npix = (long)N * HW;
  cy_prior_plan_t pl;
  const int rc = prior_plan(CY_PRIOR_DAE, npix, K, Cimg, min_int(ptr_align(logits), 16), &pl);
  if (rc != CY_OK) return rc;
  if (!dae_act_ok(act)) return CY_ERR_SHAPE;
  if (ptr_align(w) < 4 || ptr_align(b) < 4 || ptr_align(image) < 4) return CY_ERR_ARG;
  if (ws_bytes < dae_ws_bytes(npix, K, 0)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  CY_DAE_LAUNCH(dae_fwd_kernel, pl, act, pl.fwd_grid, st, logits, w, b, image, (double*)ws, npix, HW, K, Cimg);
  hipLaunchKernelGGL(mean_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, pl.fwd_grid,
                     (double)npix * (double)Cimg, loss);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_dae_bwd(const float* logits, const float* w, const float* b, const float* image, const float* gscale,
               float* dlogits, float* dw, float* db, int N, long HW, int K, int Cimg, int act, void* ws,
               size_t ws_bytes, void* stream) {
  if (!logits || !w || !b || !image || !gscale || !dlogits || !dw || !db || !ws || N < 1 || HW < 1) return CY_ERR_ARG;
  const long npix = (long)N * HW;
  cy_prior_plan_t pl;
  const int rc = prior_plan(CY_PRIOR_DAE, npix, K, Cimg, min_int(ptr_align(logits), 16), &pl);
  if (rc != CY_OK) return rc;
  if (!dae_act_ok(act)) return CY_ERR_SHAPE;
  if (ptr_align(w) < 4 || ptr_align(b) < 4 || ptr_align(image) < 4 || ptr_align(dlogits) < 4) return CY_ERR_ARG;
  if (ws_bytes < dae_ws_bytes(npix, K, 1)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  CY_DAE_LAUNCH(dae_bwd_kernel, pl, act, pl.bwd_grid, st, logits, w, b, image, gscale, dlogits, (double*)ws, npix, HW,
                K, Cimg);
  hipLaunchKernelGGL(dae_param_finalize_kernel, dim3(K + 1), dim3(256), 0, st, (const double*)ws, pl.bwd_grid, K, dw,
                     db);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_ortho_fwd(const float* prototypes, float* loss, int K, int C, void* stream) {
  if (!prototypes || !loss) return CY_ERR_ARG;
  cy_prior_plan_t pl;
  const int rc = prior_plan(CY_PRIOR_ORTHO, 0, K, C, 4, &pl);
  if (rc != CY_OK) return rc;
  if (ptr_align(prototypes) < 4) return CY_ERR_ARG;
  if (!cy_lds_limit_once<ortho_fwd_kernel<0>, ortho_fwd_kernel<1>>(ORTHO_LDS_MAX)) return CY_ERR_LAUNCH;
  hipStream_t st = (hipStream_t)stream;
  if (pl.variant)
    hipLaunchKernelGGL(ortho_fwd_kernel<1>, dim3(1), dim3(256), pl.fwd_lds, st, prototypes, loss, K, C, pl.aux);
  else
    hipLaunchKernelGGL(ortho_fwd_kernel<0>, dim3(1), dim3(256), pl.fwd_lds, st, prototypes, loss, K, C, pl.aux);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_ortho_bwd(const float* prototypes, const float* gscale, float* dprototypes, int K, int C, void* stream) {
  if (!prototypes || !gscale || !dprototypes) return CY_ERR_ARG;
  cy_prior_plan_t pl;
  const int rc = prior_plan(CY_PRIOR_ORTHO, 0, K, C, 4, &pl);
  if (rc != CY_OK) return rc;
  if (ptr_align(prototypes) < 4 || ptr_align(dprototypes) < 4) return CY_ERR_ARG;
  if (!cy_lds_limit_once<ortho_bwd_kernel<0>, ortho_bwd_kernel<1>>(ORTHO_LDS_MAX)) return CY_ERR_LAUNCH;
  hipStream_t st = (hipStream_t)stream;
  if (pl.variant)
    hipLaunchKernelGGL(ortho_bwd_kernel<1>, dim3(1), dim3(256), pl.bwd_lds, st, prototypes, gscale, dprototypes, K, C,
                       pl.aux);
  else
    hipLaunchKernelGGL(ortho_bwd_kernel<0>, dim3(1), dim3(256), pl.bwd_lds, st, prototypes, gscale, dprototypes, K, C,
                       pl.aux);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

}  // extern "C"
