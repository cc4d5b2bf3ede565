// MixUp and interpolation-consistency training (ICT): the mixed input batch and the two losses against a mixed target.
//   mixup_data: lam * x + (1 - lam) * x[index]                      semi_seg/hooks/utils.py:284-297
//   MixUp:  KL_div()(softmax(logits), lam * onehot(y) + (1 - lam) * onehot(y)[index])     semi_seg/hooks/mixup.py:49-58
//   ICT:    MSELoss(softmax(student), lam * softmax(teacher) + (1 - lam) * softmax(teacher)[index]).mean()
//                                                                                         semi_seg/hooks/mt.py:301-319
// `index` [N] int32 is a gather: image n is mixed with image index[n] (any values in [0, N); the binding checks the
// range before it uploads).  The two weights arrive as f32, rounded from lam and 1 - lam on the host; no kernel forms
// 1 - w.  The mixed one-hot target has at most two non-zero classes per pixel, so the MixUp loss reads two labels and
// never a [N,K,H,W] target; the ICT target is recomputed in registers from the two teacher rows.  The losses are of the
// family of cy_pixel_reg.hip: one thread per pixel, grid-stride, f64 per-block partials summed in block order by a
// one-block launch (no atomics: two runs give the same bits), one launch for the backward.
#include "cy_common.h"
#include "cy_pixel_loss.h"
#include "cy_reduce.h"

namespace {

constexpr int IMG_GRID_CAP = 2048;  // blocks of cy_mix_images
constexpr int IMG_ROWS_CAP = 1024;  // of them along the images

// ---------------------------------------------------------------- images
// two correctly rounded products and one correctly rounded sum, never contracted to an FMA: the bits of torch's CPU
// f32 `lam * x + (1 - lam) * x[index]`.  (HIP's __fmul_rn / __fadd_rn are inline functions around the plain operators,
// which device code contracts by default; the pragma on the operators themselves is what keeps the three roundings.)
__device__ __forceinline__ float mix2(float ws, float a, float wo, float b) {
#pragma clang fp contract(off)
  const float pa = ws * a;
  const float pb = wo * b;
  return pa + pb;
}

// grid (gx, gy): blockIdx.y strides over the images, blockIdx.x over the `per` accesses of an image
template <int VEC>
__global__ void __launch_bounds__(256)
    mix_images_kernel(const float* __restrict__ x, const int32_t* __restrict__ index, float ws, float wo,
                      float* __restrict__ out, int N, long per) {
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const long self = (long)n * per, other = (long)index[n] * per;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < per; e += (long)gridDim.x * 256L) {
      if constexpr (VEC == 4) {
        const f32x4 a = reinterpret_cast<const f32x4*>(x)[self + e];
        const f32x4 b = reinterpret_cast<const f32x4*>(x)[other + e];
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = mix2(ws, a[k], wo, b[k]);
        reinterpret_cast<f32x4*>(out)[self + e] = o;
      } else {
        out[self + e] = mix2(ws, x[self + e], wo, x[other + e]);
      }
    }
  }
}

// ---------------------------------------------------------------- shared by the two losses
// the partner of pixel p: the same position of image index[n]
__device__ __forceinline__ long partner_pixel(const int32_t* __restrict__ index, long p, long HW) {
  const long n = p / HW;
  return (long)index[n] * HW + (p - n * HW);
}

// p[t], or 0 for a label outside [0, K) (it selects no class)
__device__ __forceinline__ float pick_k(const float* p, int K, long t) {
  float v = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K && k == t) v = p[k];
  return v;
}

// -t log((p + eps) / (t + eps)); a weight of exactly 0 adds exactly 0, and p == 0 stays finite
__device__ __forceinline__ float kl_term(float t, float p, float eps) {
  return t == 0.f ? 0.f : -t * logf((p + eps) / (t + eps));
}

// ---------------------------------------------------------------- MixUp: KL against the two-label target
template <int KT>
__global__ void __launch_bounds__(256)
    softmax_mixkl_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                             const int32_t* __restrict__ index, float ws, float wo, double* __restrict__ partial,
                             long npix, long HW, int Krt, float eps) {
  const int K = KT ? KT : Krt;
  __shared__ double sh[256];
  double acc = 0.0;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float z[KMAX], pr[KMAX];
    load_row<KT>(logits, p, K, z);
    softmax_k(z, pr, K);
    const long a = target[p], b = target[partner_pixel(index, p, HW)];
    const float pa = pick_k(pr, K, a);
    float l;
    if (a == b)
      l = kl_term(ws + wo, pa, eps);
    else
      l = kl_term(ws, pa, eps) + kl_term(wo, pick_k(pr, K, b), eps);
    acc += (double)l;
  }
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

template <int KT>
__global__ void __launch_bounds__(256)
    softmax_mixkl_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                             const int32_t* __restrict__ index, float ws, float wo, const float* __restrict__ gscale,
                             float* __restrict__ dlogits, long npix, long HW, int Krt, float eps) {
  const int K = KT ? KT : Krt;
  const float gs = gscale[0] / (float)npix;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float z[KMAX], pr[KMAX];
    load_row<KT>(logits, p, K, z);
    softmax_k(z, pr, K);
    const long a = target[p], b = target[partner_pixel(index, p, HW)];
    // c_k = t_k p_k / (p_k + eps);  dz_j = gs ((c_a + c_b) p_j - c_a [j == a] - c_b [j == b])
    const float pa = pick_k(pr, K, a), pb = pick_k(pr, K, b);
    const float ta = a == b ? ws + wo : ws, tb = a == b ? 0.f : wo;
    const float ca = ta * pa / (pa + eps), cb = tb * pb / (pb + eps);
    const float csum = ca + cb;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) z[k] = gs * (csum * pr[k] - (k == a ? ca : 0.f) - (k == b ? cb : 0.f));
    store_row<KT>(dlogits, p, K, z);
  }
}

// ---------------------------------------------------------------- ICT: MSE against the blend of two teacher softmaxes
// m = ws softmax(t[p]) + wo softmax(t[partner]), in registers
template <int KT>
__device__ __forceinline__ void ict_target(const float* __restrict__ zt, const int32_t* __restrict__ index, long p,
                                           long HW, int K, float ws, float wo, float* m) {
  float z[KMAX], q[KMAX];
  load_row<KT>(zt, p, K, z);
  softmax_k(z, m, K);
  load_row<KT>(zt, partner_pixel(index, p, HW), K, z);
  softmax_k(z, q, K);
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) m[k] = fmaf(wo, q[k], ws * m[k]);
}

template <int KT>
__global__ void __launch_bounds__(256)
    softmax_mixmse_fwd_kernel(const float* __restrict__ zs, const float* __restrict__ zt,
                              const int32_t* __restrict__ index, float ws, float wo, double* __restrict__ partial,
                              long npix, long HW, int Krt) {
  const int K = KT ? KT : Krt;
  __shared__ double sh[256];
  double acc = 0.0;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float m[KMAX], z[KMAX], s[KMAX];
    ict_target<KT>(zt, index, p, HW, K, ws, wo, m);
    load_row<KT>(zs, p, K, z);
    softmax_k(z, s, K);
    float e = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        const float d = s[k] - m[k];
        e = fmaf(d, d, e);
      }
    acc += (double)e;
  }
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

template <int KT>
__global__ void __launch_bounds__(256)
    softmax_mixmse_bwd_kernel(const float* __restrict__ zs, const float* __restrict__ zt,
                              const int32_t* __restrict__ index, float ws, float wo, const float* __restrict__ gscale,
                              float* __restrict__ dzs, long npix, long HW, int Krt) {
  const int K = KT ? KT : Krt;
  const float gs = (float)(2.0 * (double)gscale[0] / ((double)npix * (double)K));
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float m[KMAX], z[KMAX], s[KMAX];
    ict_target<KT>(zt, index, p, HW, K, ws, wo, m);
    load_row<KT>(zs, p, K, z);
    softmax_k(z, s, K);
    // the target is a constant: d = s - m;  dz = gs s (d - sum_j d_j s_j)
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        m[k] = s[k] - m[k];
        dot = fmaf(m[k], s[k], dot);
      }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) m[k] = gs * s[k] * (m[k] - dot);
    store_row<KT>(dzs, p, K, m);
  }
}

// ---------------------------------------------------------------- the launch rule
// the one place the three groups take their kernel form and grid from; a status as the launches return it, and nothing
// is written to `pl` before the last refusal
int mix_plan(int form, int N, long per_image, int K, int align, cy_mix_plan_t* pl) {
  if (!pl || N < 1 || per_image < 1 || align < 1) return CY_ERR_ARG;
  if (form == CY_MIX_IMAGES) {
    if (align % 4 != 0) return CY_ERR_ARG;
    pl->vec = (per_image % 4 == 0 && align % 16 == 0) ? 4 : 1;
    pl->kt = 0;
    const long per = per_image / pl->vec;
    pl->rows = min_int(N, IMG_ROWS_CAP);
    const int gx = cy_blocks(per, 256, IMG_GRID_CAP / pl->rows);
    pl->fwd_grid = gx * pl->rows;
    const long trips = (long)cy_trips(per, gx, 256) * ((N + pl->rows - 1) / pl->rows);
    pl->fwd_trips = trips > INT32_MAX ? INT32_MAX : (int)trips;
    pl->bwd_grid = pl->bwd_trips = 0;
    return CY_OK;
  }
  if (form != CY_MIX_KL && form != CY_MIX_MSE) return CY_ERR_ARG;
  if (K < 2 || K > KMAX) return CY_ERR_SHAPE;
  const int row = K == 2 ? 8 : 16;  // bytes of a row access of the compiled forms
  const int kt = ((K == 2 || K == 4 || K == 8) && align % row == 0) ? K : 0;
  if (K == 4 && !kt) return CY_ERR_ARG;  // K == 4 rows are read 16 bytes at a time in the run-time form too
  if (align % 4 != 0) return CY_ERR_ARG;
  pl->kt = kt;
  pl->vec = pl->kt == 2 ? 2 : pl->kt ? 4 : 1;
  const long npix = (long)N * per_image;
  pl->fwd_grid = cy_blocks(npix, 256, LOSS_GRID_CAP);
  pl->bwd_grid = pl->fwd_grid * 2;
  pl->fwd_trips = cy_trips(npix, pl->fwd_grid, 256);
  pl->bwd_trips = cy_trips(npix, pl->bwd_grid, 256);
  pl->rows = 0;
  return CY_OK;
}

// launch `KERNEL<kt>` for the plan's kt
#define CY_MIX_LAUNCH(KERNEL, KT_, GRID, ST, ...)                                      \
  do {                                                                                 \
    if ((KT_) == 2)                                                                    \
      hipLaunchKernelGGL(KERNEL<2>, dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);        \
    else if ((KT_) == 4)                                                               \
      hipLaunchKernelGGL(KERNEL<4>, dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);        \
    else if ((KT_) == 8)                                                               \
      hipLaunchKernelGGL(KERNEL<8>, dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);        \
    else                                                                               \
      hipLaunchKernelGGL(KERNEL<0>, dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);        \
    CY_CHECK_LAUNCH();                                                                 \
  } while (0)

inline size_t mix_ws_bytes(int N, long HW) {
  if (N < 1 || HW < 1) return 0;
  return (size_t)cy_blocks((long)N * HW, 256, LOSS_GRID_CAP) * sizeof(double);
}

}  // namespace

extern "C" {

int cy_mix_plan(int form, int N, long per_image, int K, int align, cy_mix_plan_t* out) {
  return mix_plan(form, N, per_image, K, align, out);  // (a NULL `out` is the rule's first refusal)
}

int cy_mix_images(const float* x, const int32_t* index, float w_self, float w_other, float* out, int N, long E,
                  void* stream) {
  if (!x || !index || !out || N < 1 || E < 1 || x == out) return CY_ERR_ARG;
  cy_mix_plan_t pl;
  const int rc = mix_plan(CY_MIX_IMAGES, N, E, 0, min_int(ptr_align(x), ptr_align(out)), &pl);
  if (rc != CY_OK) return rc;
  const dim3 grid(pl.fwd_grid / pl.rows, pl.rows);
  hipStream_t st = (hipStream_t)stream;
  if (pl.vec == 4)
    hipLaunchKernelGGL(mix_images_kernel<4>, grid, dim3(256), 0, st, x, index, w_self, w_other, out, N, E / 4);
  else
    hipLaunchKernelGGL(mix_images_kernel<1>, grid, dim3(256), 0, st, x, index, w_self, w_other, out, N, E);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

size_t cy_softmax_mixkl_ws_bytes(int N, long HW) { return mix_ws_bytes(N, HW); }

int cy_softmax_mixkl_fwd(const float* logits, const int64_t* target, const int32_t* index, float w_self, float w_other,
                         float* loss, int N, long HW, int K, float eps, void* ws, size_t ws_bytes, void* stream) {
  if (!logits || !target || !index || !loss || !ws || N < 1 || HW < 1) return CY_ERR_ARG;
  cy_mix_plan_t pl;
  const int rc = mix_plan(CY_MIX_KL, N, HW, K, ptr_align(logits), &pl);
  if (rc != CY_OK) return rc;
  if (ws_bytes < mix_ws_bytes(N, HW)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const long npix = (long)N * HW;
  CY_MIX_LAUNCH(softmax_mixkl_fwd_kernel, pl.kt, pl.fwd_grid, st, logits, target, index, w_self, w_other, (double*)ws,
                npix, HW, K, eps);
  hipLaunchKernelGGL(mean_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, pl.fwd_grid, (double)npix,
                     loss);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_softmax_mixkl_bwd(const float* logits, const int64_t* target, const int32_t* index, float w_self, float w_other,
                         const float* gscale, float* dlogits, int N, long HW, int K, float eps, void* stream) {
  if (!logits || !target || !index || !gscale || !dlogits || N < 1 || HW < 1) return CY_ERR_ARG;
  cy_mix_plan_t pl;
  const int rc = mix_plan(CY_MIX_KL, N, HW, K, min_int(ptr_align(logits), ptr_align(dlogits)), &pl);
  if (rc != CY_OK) return rc;
  CY_MIX_LAUNCH(softmax_mixkl_bwd_kernel, pl.kt, pl.bwd_grid, (hipStream_t)stream, logits, target, index, w_self,
                w_other, gscale, dlogits, (long)N * HW, HW, K, eps);
  return CY_OK;
}

size_t cy_softmax_mixmse_ws_bytes(int N, long HW) { return mix_ws_bytes(N, HW); }

int cy_softmax_mixmse_fwd(const float* student, const float* teacher, const int32_t* index, float w_self,
                          float w_other, float* loss, int N, long HW, int K, void* ws, size_t ws_bytes, void* stream) {
  if (!student || !teacher || !index || !loss || !ws || N < 1 || HW < 1) return CY_ERR_ARG;
  cy_mix_plan_t pl;
  const int rc = mix_plan(CY_MIX_MSE, N, HW, K, min_int(ptr_align(student), ptr_align(teacher)), &pl);
  if (rc != CY_OK) return rc;
  if (ws_bytes < mix_ws_bytes(N, HW)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const long npix = (long)N * HW;
  CY_MIX_LAUNCH(softmax_mixmse_fwd_kernel, pl.kt, pl.fwd_grid, st, student, teacher, index, w_self, w_other,
                (double*)ws, npix, HW, K);
  hipLaunchKernelGGL(mean_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, pl.fwd_grid,
                     (double)npix * (double)K, loss);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_softmax_mixmse_bwd(const float* student, const float* teacher, const int32_t* index, float w_self,
                          float w_other, const float* gscale, float* dstudent, int N, long HW, int K, void* stream) {
  if (!student || !teacher || !index || !gscale || !dstudent || N < 1 || HW < 1) return CY_ERR_ARG;
  cy_mix_plan_t pl;
  const int rc = mix_plan(CY_MIX_MSE, N, HW, K,
                          min_int(min_int(ptr_align(student), ptr_align(teacher)), ptr_align(dstudent)), &pl);
  if (rc != CY_OK) return rc;
  CY_MIX_LAUNCH(softmax_mixmse_bwd_kernel, pl.kt, pl.bwd_grid, (hipStream_t)stream, student, teacher, index, w_self,
                w_other, gscale, dstudent, (long)N * HW, HW, K);
  return CY_OK;
}

}  // extern "C"
