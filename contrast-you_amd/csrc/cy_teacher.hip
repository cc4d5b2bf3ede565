// The differentiable mean teacher's state updates and its consistency term (semi_seg/hooks/dmt.py).
//   Adam:        torch.optim.Adam(amsgrad=False, maximize=False) on one flat f32 buffer           dmt.py:66
//   axpy:        p.data.sub_(g, alpha=l) / p.data.add_(g, alpha=l) on one flat f32 buffer         dmt.py:305-336
//   EMA, multi:  the expression of cy_ema_update over `count` tensors named by a device table     mt.py:49-82
//   gather-MSE:  MSELoss(softmax(student), affine(softmax(teacher))), the warp a gather by an int32 source map with
//                the all-zero vector where the source lies outside the image                       dmt.py:177-197
// All four stream HBM once.  Adam and axpy read and write 16 bytes per lane where every base is 16-byte aligned and
// finish the n % 4 tail one float at a time; otherwise one float at a time throughout.  The multi-tensor EMA is a 2-D
// grid: blockIdx.y names the tensor, blockIdx.x strides over it.  Gather-MSE is of the family of cy_mixup.hip's ICT
// loss: [npix][K] f32 rows, one thread per pixel, grid-stride, one f64 partial per block, a fixed-order finalize, no
// atomics; neither softmax, nor the warped tensor, nor the difference is stored.
#include "cy_common.h"
#include "cy_flat.h"
#include "cy_pixel_loss.h"
#include "cy_reduce.h"

namespace {

constexpr int EMA_MULTI_MAX = 4096;   // tensors of one multi-tensor launch
constexpr int EMA_MULTI_BLOCKS = 8192;  // about this many blocks in all: grid.x = clamp(8192 / count, 2, 64)

// VEC == 4: n4 = n / 4 groups of four, then the n % 4 tail by the first threads of block 0
template <int VEC>
__global__ void __launch_bounds__(256)
    adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                long n, AdamScalars s) {
  const long stride = (long)gridDim.x * 256L;
  if constexpr (VEC == 4) {
    const long n4 = n / 4;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += stride) {
      f32x4 pv = reinterpret_cast<f32x4*>(p)[i], mv = reinterpret_cast<f32x4*>(m)[i];
      f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
      const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pv[j], mj = mv[j], vj = vv[j];
        adam_elem(pj, gv[j], mj, vj, s);
        pv[j] = pj, mv[j] = mj, vv[j] = vj;
      }
      reinterpret_cast<f32x4*>(p)[i] = pv;
      reinterpret_cast<f32x4*>(m)[i] = mv;
      reinterpret_cast<f32x4*>(v)[i] = vv;
    }
    const long i = n4 * 4 + threadIdx.x;
    if (blockIdx.x == 0 && i < n) adam_elem(p[i], g[i], m[i], v[i], s);
  } else {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += stride) adam_elem(p[i], g[i], m[i], v[i], s);
  }
}

template <int VEC>
__global__ void __launch_bounds__(256)
    axpy_kernel(float* __restrict__ y, const float* __restrict__ x, long n, float a) {
  const long stride = (long)gridDim.x * 256L;
  if constexpr (VEC == 4) {
    const long n4 = n / 4;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += stride) {
      f32x4 yv = reinterpret_cast<f32x4*>(y)[i];
      const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) yv[j] = fmaf(a, xv[j], yv[j]);
      reinterpret_cast<f32x4*>(y)[i] = yv;
    }
    const long i = n4 * 4 + threadIdx.x;
    if (blockIdx.x == 0 && i < n) y[i] = fmaf(a, x[i], y[i]);
  } else {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += stride) y[i] = fmaf(a, x[i], y[i]);
  }
}

// table: [count][3] int64 in device memory: the teacher's address, the student's address, the element count.  A row
// with a null address or a count < 1 is skipped.  The expression is ema_kernel's (cy_misc.hip), term for term.
__global__ void __launch_bounds__(256)
    ema_multi_kernel(const int64_t* __restrict__ table, float alpha, float keep) {
  const int64_t* row = table + 3L * blockIdx.y;
  float* __restrict__ teacher = reinterpret_cast<float*>((uintptr_t)row[0]);
  const float* __restrict__ student = reinterpret_cast<const float*>((uintptr_t)row[1]);
  const long n = (long)row[2];
  if (!teacher || !student) return;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L)
    teacher[i] = (alpha * teacher[i] + (1.f - alpha) * student[i]) * keep;
}

// a row of logits: the compiled forms read 8 / 16 bytes at a time on their aligned rows; the run-time form reads one
// float at a time for every K (K == 4 too: its base may be aligned to 4 bytes only)
template <int KT> __device__ __forceinline__ void gather_row(const float* l, long p, int K, float* z) {
  if constexpr (KT == 0) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) z[k] = l[p * K + k];
  } else {
    load_row<KT>(l, p, K, z);
  }
}

// q = softmax(teacher row at the map's source) or 0 where the source is outside (a value outside [0, HW) counts as
// outside: nothing is read out of range)
template <int KT>
__device__ __forceinline__ void gather_target(const float* __restrict__ zt, const int32_t* __restrict__ map, long p,
                                              long HW, int K, float* q) {
  const long src = (long)map[p];
  const bool inside = src >= 0 && src < HW;
  // no branch around the row: an outside pixel reads its image's first row and drops the result
  float z[KMAX];
  gather_row<KT>(zt, (p / HW) * HW + (inside ? src : 0), K, z);
  softmax_k(z, q, K);
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) q[k] = inside ? q[k] : 0.f;
}

template <int KT>
__global__ void __launch_bounds__(256)
    gathermse_fwd_kernel(const float* __restrict__ zt, const int32_t* __restrict__ map, const float* __restrict__ zs,
                         double* __restrict__ partial, long npix, long HW, int Krt) {
  const int K = KT ? KT : Krt;
  __shared__ double sh[256];
  double acc = 0.0;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float q[KMAX], z[KMAX], s[KMAX];
    gather_target<KT>(zt, map, p, HW, K, q);
    gather_row<KT>(zs, p, K, z);
    softmax_k(z, s, K);
    float e = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        const float d = q[k] - s[k];
        e = fmaf(d, d, e);
      }
    acc += (double)e;
  }
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

template <int KT>
__global__ void __launch_bounds__(256)
    gathermse_bwd_kernel(const float* __restrict__ zt, const int32_t* __restrict__ map, const float* __restrict__ zs,
                         const float* __restrict__ gscale, float* __restrict__ dzs, long npix, long HW, int Krt) {
  const int K = KT ? KT : Krt;
  const float gs = (float)(2.0 * (double)gscale[0] / ((double)npix * (double)K));
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float q[KMAX], z[KMAX], s[KMAX];
    gather_target<KT>(zt, map, p, HW, K, q);
    gather_row<KT>(zs, p, K, z);
    softmax_k(z, s, K);
    // the teacher side is a constant here: d = s - q;  dz = gs s (d - sum_j s_j d_j)
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        q[k] = s[k] - q[k];
        dot = fmaf(q[k], s[k], dot);
      }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) q[k] = gs * s[k] * (q[k] - dot);
    store_row<KT>(dzs, p, K, q);
  }
}

// ---------------------------------------------------------------- the launch rule
// the one place the four families take their kernel form and grid from; a status as the launches return it, and nothing
// is written to `pl` before the last refusal
int teacher_plan(int form, long n, int K, int align, cy_teacher_plan_t* pl) {
  if (!pl || n < 1 || align < 1 || align % 4 != 0) return CY_ERR_ARG;
  if (form < CY_TEACHER_ADAM || form > CY_TEACHER_GATHERMSE) return CY_ERR_ARG;
  if (form == CY_TEACHER_EMA_MULTI && n > EMA_MULTI_MAX) return CY_ERR_SHAPE;
  if (form == CY_TEACHER_GATHERMSE && (K < 2 || K > KMAX)) return CY_ERR_SHAPE;
  pl->variant = 0, pl->bwd_grid = pl->bwd_trips = 0, pl->rows = 0;
  if (form == CY_TEACHER_ADAM || form == CY_TEACHER_AXPY) {
    FlatPlan fp;  // cy_flat.h: the rule cy_optim_plan gives too
    flat_plan(n, align, &fp);
    pl->vec = fp.vec, pl->fwd_grid = fp.grid, pl->fwd_trips = fp.trips;
    return CY_OK;
  }
  if (form == CY_TEACHER_EMA_MULTI) {  // n: the tensors
    long gx = EMA_MULTI_BLOCKS / n;
    gx = gx < 2 ? 2 : gx > 64 ? 64 : gx;
    pl->vec = 1;
    pl->fwd_grid = (int)gx;
    pl->rows = (int)n;
    pl->fwd_trips = (int)gx * 256;  // elements of a tensor that one trip covers
    return CY_OK;
  }
  // CY_TEACHER_GATHERMSE, n: the pixels
  const int row = K == 2 ? 8 : 16;  // bytes of a row access of the compiled forms
  pl->variant = ((K == 2 || K == 4 || K == 8) && align % row == 0) ? K : 0;
  pl->vec = pl->variant == 2 ? 2 : pl->variant ? 4 : 1;
  pl->fwd_grid = cy_blocks(n, 256, LOSS_GRID_CAP);
  pl->bwd_grid = pl->fwd_grid * 2;
  pl->fwd_trips = cy_trips(n, pl->fwd_grid, 256);
  pl->bwd_trips = cy_trips(n, pl->bwd_grid, 256);
  return CY_OK;
}

// launch `KERNEL<variant>` of the gather-MSE pair
#define CY_GATHER_LAUNCH(KERNEL, KT_, GRID, ST, ...)                                   \
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

inline size_t gather_ws_bytes(int N, long HW) {
  if (N < 1 || HW < 1) return 0;
  return (size_t)cy_blocks((long)N * HW, 256, LOSS_GRID_CAP) * sizeof(double);
}

}  // namespace

extern "C" {

int cy_teacher_plan(int form, long n, int K, int align, cy_teacher_plan_t* out) {
  return teacher_plan(form, n, K, align, out);  // (a NULL `out` is the rule's first refusal)
}

int cy_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1,
                 float beta2, float eps, float weight_decay, long step, void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || step < 1) return CY_ERR_ARG;
  const int align =
      min_int(min_int(ptr_align(param), ptr_align(grad)), min_int(ptr_align(exp_avg), ptr_align(exp_avg_sq)));
  cy_teacher_plan_t pl;
  const int rc = teacher_plan(CY_TEACHER_ADAM, n, 0, align, &pl);
  if (rc != CY_OK) return rc;
  const AdamScalars s = adam_scalars(lr, beta1, beta2, eps, weight_decay, step);
  hipStream_t st = (hipStream_t)stream;
  if (pl.vec == 4)
    hipLaunchKernelGGL(adam_kernel<4>, dim3(pl.fwd_grid), dim3(256), 0, st, param, grad, exp_avg, exp_avg_sq, n, s);
  else
    hipLaunchKernelGGL(adam_kernel<1>, dim3(pl.fwd_grid), dim3(256), 0, st, param, grad, exp_avg, exp_avg_sq, n, s);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_axpy(float* y, const float* x, long n, float a, void* stream) {
  if (!y || !x || n <= 0) return CY_ERR_ARG;
  cy_teacher_plan_t pl;
  const int rc = teacher_plan(CY_TEACHER_AXPY, n, 0, min_int(ptr_align(y), ptr_align(x)), &pl);
  if (rc != CY_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (pl.vec == 4)
    hipLaunchKernelGGL(axpy_kernel<4>, dim3(pl.fwd_grid), dim3(256), 0, st, y, x, n, a);
  else
    hipLaunchKernelGGL(axpy_kernel<1>, dim3(pl.fwd_grid), dim3(256), 0, st, y, x, n, a);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_ema_update_multi(const int64_t* table, int count, float alpha, float weight_decay, void* stream) {
  if (!table) return CY_ERR_ARG;
  if (count < 1 || count > EMA_MULTI_MAX) return CY_ERR_SHAPE;
  if (ptr_align(table) < 8) return CY_ERR_ARG;
  cy_teacher_plan_t pl;
  const int rc = teacher_plan(CY_TEACHER_EMA_MULTI, count, 0, 4, &pl);
  if (rc != CY_OK) return rc;
  hipLaunchKernelGGL(ema_multi_kernel, dim3(pl.fwd_grid, pl.rows), dim3(256), 0, (hipStream_t)stream, table, alpha,
                     1.f - weight_decay);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

size_t cy_softmax_gathermse_ws_bytes(int N, long HW) { return gather_ws_bytes(N, HW); }

int cy_softmax_gathermse_fwd(const float* teacher, const int32_t* map, const float* student, float* loss, int N,
                             long HW, int K, void* ws, size_t ws_bytes, void* stream) {
  if (!teacher || !map || !student || !loss || !ws || N < 1 || HW < 1) return CY_ERR_ARG;
  const long npix = (long)N * HW;
  cy_teacher_plan_t pl;
  const int rc = teacher_plan(CY_TEACHER_GATHERMSE, npix, K, min_int(ptr_align(teacher), ptr_align(student)), &pl);
  if (rc != CY_OK) return rc;
  if (ptr_align(map) < 4 || ptr_align(ws) < 8) return CY_ERR_ARG;
  if (ws_bytes < gather_ws_bytes(N, HW)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  CY_GATHER_LAUNCH(gathermse_fwd_kernel, pl.variant, pl.fwd_grid, st, teacher, map, student, (double*)ws, npix, HW, K);
  hipLaunchKernelGGL(mean_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, pl.fwd_grid,
                     (double)npix * (double)K, loss);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_softmax_gathermse_bwd(const float* teacher, const int32_t* map, const float* student, const float* gscale,
                             float* dstudent, int N, long HW, int K, void* stream) {
  if (!teacher || !map || !student || !gscale || !dstudent || N < 1 || HW < 1) return CY_ERR_ARG;
  const long npix = (long)N * HW;
  cy_teacher_plan_t pl;
  const int rc = teacher_plan(CY_TEACHER_GATHERMSE, npix, K,
                              min_int(min_int(ptr_align(teacher), ptr_align(student)), ptr_align(dstudent)), &pl);
  if (rc != CY_OK) return rc;
  if (ptr_align(map) < 4 || ptr_align(gscale) < 4) return CY_ERR_ARG;
  CY_GATHER_LAUNCH(gathermse_bwd_kernel, pl.variant, pl.bwd_grid, (hipStream_t)stream, teacher, map, student, gscale,
                   dstudent, npix, HW, K);
  return CY_OK;
}

}  // extern "C"
