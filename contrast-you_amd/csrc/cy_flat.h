// What the sweeps over flat f32 buffers share (cy_teacher.hip: Adam, axpy; cy_optim.hip: SGD, Adam(W), amsgrad): the
// launch rule and one element of torch's Adam.  Each exists once, so that cy_teacher_plan and cy_optim_plan cannot drift
// apart and cy_adamw_step(decoupled = 0, no amsgrad) is cy_adam_step's expression term for term.
#pragma once
#include "cy_common.h"

namespace {

constexpr int FLAT_GRID_CAP = 2048;  // blocks of the flat sweeps (256 CUs x 8), the rest is grid-stride

struct FlatPlan {
  int vec, grid, trips;
};

// 16 bytes per lane where every base is 16-byte aligned and there are four floats (the n % 4 tail goes one float at a
// time, by the first threads of block 0); otherwise one float per lane.  A status as the launches return it.
inline int flat_plan(long n, int align, FlatPlan* pl) {
  if (!pl || n < 1 || align < 1 || align % 4 != 0) return CY_ERR_ARG;
  pl->vec = (align % 16 == 0 && n >= 4) ? 4 : 1;
  const long groups = n / pl->vec;
  pl->grid = cy_blocks(groups, 256, FLAT_GRID_CAP);
  pl->trips = cy_trips(groups, pl->grid, 256);
  return CY_OK;
}

struct AdamScalars {
  float beta1, beta2, eps, wd;
  float step_size;  // lr / (1 - beta1^t)
  float sqrt_bc2;   // sqrt(1 - beta2^t)
};

// bias corrections in f64 on the host, lr / bc1 and sqrt(bc2) rounded to f32 once
inline AdamScalars adam_scalars(float lr, float beta1, float beta2, float eps, float wd, long step) {
  AdamScalars s;
  s.beta1 = beta1, s.beta2 = beta2, s.eps = eps, s.wd = wd;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  s.step_size = (float)((double)lr / bc1);
  s.sqrt_bc2 = (float)sqrt(bc2);
  return s;
}

// one element of torch's single-tensor Adam: lerp for the first moment, sqrt(v) / sqrt(bc2) + eps for the denominator
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamScalars& s) {
  if (s.wd != 0.f) g = fmaf(s.wd, p, g);
  m = m + (g - m) * (1.f - s.beta1);
  v = s.beta2 * v + (1.f - s.beta2) * g * g;
  const float denom = sqrtf(v) / s.sqrt_bc2 + s.eps;
  p = p - s.step_size * (m / denom);
}

}  // namespace
