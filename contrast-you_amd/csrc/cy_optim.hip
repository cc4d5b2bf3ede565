// The optimizers of Optim.name next to RAdam, on one flat f32 buffer per parameter group (contrastyou/optim):
//   SGD:      torch.optim.SGD(maximize=False): weight decay, momentum, dampening, nesterov   trainer/base.py:66-75
//   Adam(W):  torch.optim.Adam / AdamW(maximize=False), amsgrad where a max_exp_avg_sq buffer is given
// Both stream HBM once and are bound by it: 20 B/element for SGD with momentum (12 without), 28 for Adam(W), 36 with
// amsgrad.  The form is cy_teacher.hip's Adam (cy_flat.h holds the launch rule and the element both share): 16 bytes per
// lane where every base is 16-byte aligned, the n % 4 tail one float at a time; one float per lane on a base that is only
// 4-byte aligned -- a run of touched parameters starts at an arbitrary parameter offset, so ordinary training reaches
// that form.  At most 2048 blocks of 256, grid-stride beyond.  The gradient is read only; no atomics, so two runs give
// the same bits.
#include "cy_common.h"
#include "cy_flat.h"

namespace {

struct SgdScalars {
  float lr, momentum, wd;
  float keep;  // 1 - dampening
  int has_buf, nesterov, first;
};

// one element of torch's single-tensor SGD; `b` is read unless `first`, written when there is a buffer
__device__ __forceinline__ void sgd_elem(float& p, float g, float& b, const SgdScalars& s) {
  if (s.wd != 0.f) g = fmaf(s.wd, p, g);
  if (s.has_buf) {
    b = s.first ? g : s.momentum * b + s.keep * g;
    g = s.nesterov ? fmaf(s.momentum, b, g) : b;
  }
  p = fmaf(-s.lr, g, p);
}

// VEC == 4: n4 = n / 4 groups of four, then the n % 4 tail by the first threads of block 0.  `b` may be null
// (momentum == 0): nothing of it is read or written then.
template <int VEC>
__global__ void __launch_bounds__(256)
    sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ b, long n, SgdScalars s) {
  const long stride = (long)gridDim.x * 256L;
  const bool load_b = s.has_buf && !s.first;
  if constexpr (VEC == 4) {
    const long n4 = n / 4;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += stride) {
      f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
      const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
      f32x4 bv = {0.f, 0.f, 0.f, 0.f};
      if (load_b) bv = reinterpret_cast<f32x4*>(b)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pv[j], bj = bv[j];
        sgd_elem(pj, gv[j], bj, s);
        pv[j] = pj, bv[j] = bj;
      }
      reinterpret_cast<f32x4*>(p)[i] = pv;
      if (s.has_buf) reinterpret_cast<f32x4*>(b)[i] = bv;
    }
    const long i = n4 * 4 + threadIdx.x;
    if (blockIdx.x == 0 && i < n) {
      float pj = p[i], bj = load_b ? b[i] : 0.f;
      sgd_elem(pj, g[i], bj, s);
      p[i] = pj;
      if (s.has_buf) b[i] = bj;
    }
  } else {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += stride) {
      float pj = p[i], bj = load_b ? b[i] : 0.f;
      sgd_elem(pj, g[i], bj, s);
      p[i] = pj;
      if (s.has_buf) b[i] = bj;
    }
  }
}

// one element of torch's single-tensor Adam / AdamW.  DECOUPLED: p *= decay = 1 - lr wd first (s.wd is then 0, so no
// L2 term follows); a compiled flag, so that the Adam form carries no multiply the compiler could contract into the
// update: without amsgrad it is adam_elem itself, to the bit.
template <bool AMSGRAD, bool DECOUPLED>
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float& vmax, float decay,
                                           const AdamScalars& s) {
  if constexpr (DECOUPLED) p = p * decay;
  if constexpr (!AMSGRAD) {
    adam_elem(p, g, m, v, s);
  } else {
    if (s.wd != 0.f) g = fmaf(s.wd, p, g);
    m = m + (g - m) * (1.f - s.beta1);
    v = s.beta2 * v + (1.f - s.beta2) * g * g;
    vmax = fmaxf(vmax, v);
    const float denom = sqrtf(vmax) / s.sqrt_bc2 + s.eps;
    p = p - s.step_size * (m / denom);
  }
}

template <int VEC, bool AMSGRAD, bool DECOUPLED>
__global__ void __launch_bounds__(256)
    adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                 float* __restrict__ vmax, long n, float decay, AdamScalars s) {
  const long stride = (long)gridDim.x * 256L;
  if constexpr (VEC == 4) {
    const long n4 = n / 4;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += stride) {
      f32x4 pv = reinterpret_cast<f32x4*>(p)[i], mv = reinterpret_cast<f32x4*>(m)[i];
      f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
      const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
      f32x4 xv = {0.f, 0.f, 0.f, 0.f};
      if constexpr (AMSGRAD) xv = reinterpret_cast<f32x4*>(vmax)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pv[j], mj = mv[j], vj = vv[j], xj = xv[j];
        adamw_elem<AMSGRAD, DECOUPLED>(pj, gv[j], mj, vj, xj, decay, s);
        pv[j] = pj, mv[j] = mj, vv[j] = vj, xv[j] = xj;
      }
      reinterpret_cast<f32x4*>(p)[i] = pv;
      reinterpret_cast<f32x4*>(m)[i] = mv;
      reinterpret_cast<f32x4*>(v)[i] = vv;
      if constexpr (AMSGRAD) reinterpret_cast<f32x4*>(vmax)[i] = xv;
    }
  }
  // VEC == 4: the n % 4 tail by the first threads of block 0; VEC == 1: everything, grid-stride
  const long first = VEC == 4 ? (n / 4) * 4 + threadIdx.x : blockIdx.x * 256L + threadIdx.x;
  if (VEC == 4 && blockIdx.x != 0) return;
  for (long i = first; i < n; i += stride) {
    float xj = 0.f;
    if constexpr (AMSGRAD) xj = vmax[i];
    adamw_elem<AMSGRAD, DECOUPLED>(p[i], g[i], m[i], v[i], xj, decay, s);
    if constexpr (AMSGRAD) vmax[i] = xj;
  }
}

int optim_plan(int form, long n, int align, FlatPlan* pl) {
  if (form != CY_OPTIM_SGD && form != CY_OPTIM_ADAMW) return CY_ERR_ARG;
  return flat_plan(n, align, pl);
}

}  // namespace

extern "C" {

int cy_optim_plan(int form, long n, int align, cy_optim_plan_t* out) {
  if (!out) return CY_ERR_ARG;
  FlatPlan pl;
  const int rc = optim_plan(form, n, align, &pl);
  if (rc != CY_OK) return rc;
  out->vec = pl.vec, out->grid = pl.grid, out->trips = pl.trips, out->tail = pl.vec == 4 ? (int)(n % 4) : 0;
  return CY_OK;
}

int cy_sgd_step(float* param, const float* grad, float* momentum_buf, long n, float lr, float momentum,
                float dampening, float weight_decay, int nesterov, int first, void* stream) {
  if (!param || !grad || n <= 0) return CY_ERR_ARG;
  if ((momentum_buf == nullptr) != (momentum == 0.f)) return CY_ERR_ARG;
  int align = min_int(ptr_align(param), ptr_align(grad));
  if (momentum_buf) align = min_int(align, ptr_align(momentum_buf));
  FlatPlan pl;
  const int rc = optim_plan(CY_OPTIM_SGD, n, align, &pl);
  if (rc != CY_OK) return rc;
  SgdScalars s;
  s.lr = lr, s.momentum = momentum, s.wd = weight_decay;
  s.keep = (float)(1.0 - (double)dampening);
  s.has_buf = momentum_buf != nullptr, s.nesterov = nesterov != 0, s.first = first != 0;
  hipStream_t st = (hipStream_t)stream;
  if (pl.vec == 4)
    hipLaunchKernelGGL(sgd_kernel<4>, dim3(pl.grid), dim3(256), 0, st, param, grad, momentum_buf, n, s);
  else
    hipLaunchKernelGGL(sgd_kernel<1>, dim3(pl.grid), dim3(256), 0, st, param, grad, momentum_buf, n, s);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, long n,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled, long step,
                  void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || step < 1) return CY_ERR_ARG;
  int align = min_int(min_int(ptr_align(param), ptr_align(grad)), min_int(ptr_align(exp_avg), ptr_align(exp_avg_sq)));
  if (max_exp_avg_sq) align = min_int(align, ptr_align(max_exp_avg_sq));
  FlatPlan pl;
  const int rc = optim_plan(CY_OPTIM_ADAMW, n, align, &pl);
  if (rc != CY_OK) return rc;
  // AdamW: p *= 1 - lr wd (formed in f64 as torch's Python scalar is, rounded to f32 once) and no L2 term
  const float decay = decoupled ? (float)(1.0 - (double)lr * (double)weight_decay) : 1.f;
  const AdamScalars s = adam_scalars(lr, beta1, beta2, eps, decoupled ? 0.f : weight_decay, step);
  hipStream_t st = (hipStream_t)stream;
#define CY_ADAMW_LAUNCH(VEC_, AMS_)                                                                                \
  do {                                                                                                             \
    if (decoupled)                                                                                                 \
      hipLaunchKernelGGL((adamw_kernel<VEC_, AMS_, true>), dim3(pl.grid), dim3(256), 0, st, param, grad, exp_avg,  \
                         exp_avg_sq, max_exp_avg_sq, n, decay, s);                                                 \
    else                                                                                                           \
      hipLaunchKernelGGL((adamw_kernel<VEC_, AMS_, false>), dim3(pl.grid), dim3(256), 0, st, param, grad, exp_avg, \
                         exp_avg_sq, max_exp_avg_sq, n, decay, s);                                                 \
  } while (0)
  if (pl.vec == 4 && max_exp_avg_sq)
    CY_ADAMW_LAUNCH(4, true);
  else if (pl.vec == 4)
    CY_ADAMW_LAUNCH(4, false);
  else if (max_exp_avg_sq)
    CY_ADAMW_LAUNCH(1, true);
  else
    CY_ADAMW_LAUNCH(1, false);
#undef CY_ADAMW_LAUNCH
  CY_CHECK_LAUNCH();
  return CY_OK;
}

}  // extern "C"
