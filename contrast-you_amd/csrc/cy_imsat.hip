// IMSAT: the two entropies of a set of probability rows p [R][K] f32 (contrastyou/losses/discreteMI.py:20-87,275-297,
// with the module-level entropy_criterion = Entropy(eps=1e-8) of semi_seg/hooks/midl.py:13):
//   cond = (1/R) sum_r -sum_k p_rk log(p_rk + eps)          m_k = (1/R) sum_r p_rk
//   marg = -sum_k m_k log(m_k + eps)                        c_k = dmarg/dp_rk = -(log(m_k + eps) + m_k/(m_k + eps)) / R
// Three groups of entries, all f32 and all without atomics (two runs give the same bits):
//   cy_imsat_*          probability rows, 2 <= K <= 64
//   cy_imsat_pair_*     two views of the same shape and their MSE (what _DiscreteIMSATEpochHook evaluates per sub-head)
//   cy_softmax_imsat_*  from logits, 2 <= K <= 16, on the one-thread-per-pixel helpers of cy_pixel_loss.h
//
// Probability rows are swept flat, not row by row: the [R][K] buffer is R*K contiguous floats, thread t of a block
// reads the V floats at V*t of every chunk, and chunks follow each other at a stride of V*T floats, where the T
// <= 256 working threads are chosen with (V*T) % K == 0.  A thread therefore keeps the same V columns for the whole
// sweep: its column sums and its coefficients c_k live in registers, a wave's access is one contiguous run of memory
// whatever K is, and there is no index arithmetic per element and no LDS in the loop.  V = 4 (16-byte accesses) where
// every base pointer is 16-byte aligned, V = 1 otherwise: the two halves of a [2R][K] tensor with R and K odd are only
// 4-byte aligned.  The last chunk is read element by element under a bound check.  Sums run in f64: per thread, then
// per block through LDS (one partial per block and slot into the workspace, slot-major), then one block adds the
// partials of every slot in an order fixed by the grid alone and writes {marg, cond}, c_k and m_k.
#include <initializer_list>

#include "cy_common.h"
#include "cy_pixel_loss.h"
#include "cy_reduce.h"

namespace {

constexpr int IMSAT_KMAX = 64;
constexpr int IMSAT_DEPTH = 4;       // chunks a thread has in flight
constexpr int IMSAT_FWD_CAP = 1024;  // blocks; the forward writes one row of partials per block
constexpr int IMSAT_BWD_CAP = 2048;

// ---------------------------------------------------------------- the launch rule (host)
// what cy_imsat_plan answers: `status`, then the fields of cy_imsat_plan_t
struct ImsatPlan {
  int32_t status, vec, kt, threads, tile, fwd_grid, fwd_trips, bwd_grid, bwd_trips, slots;
};

inline int gcd_i(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b, b = t;
  }
  return a;
}

// bytes every pointer of the list is aligned to, capped at 16
inline int common_align(std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 16;
  for (const void* p : ptrs) bits |= (uintptr_t)p;
  return (int)(bits & (~bits + 1));
}

int plan_fill(int form, long R, int K, int align, ImsatPlan* o) {
  if (!o || form < CY_IMSAT_ROWS || form > CY_IMSAT_LOGITS || R < 1 || align < 1) return CY_ERR_ARG;
  *o = ImsatPlan{};
  const int kmax = form == CY_IMSAT_LOGITS ? KMAX : IMSAT_KMAX;
  if (K < 2 || K > kmax) {
    o->status = CY_ERR_SHAPE;
    return CY_OK;
  }
  long tiles;
  if (form == CY_IMSAT_LOGITS) {
    // K = 2, 4, 8 are compiled with K known and read a row 8 / 16 bytes at a time; rows that are not aligned for that
    // take the run-time form, one float at a time -- except K == 4, whose rows the shared load_logits reads 16 bytes
    // at a time in every form: those are refused (CY_ERR_ARG, as the other entries on these helpers do)
    const bool compiled = K == 2 || K == 4 || K == 8;
    o->kt = (compiled && align % (K == 2 ? 8 : 16) == 0) ? K : 0;
    o->vec = o->kt ? (K == 2 ? 2 : 4) : 1;
    if (K == 4 && !o->kt) {
      o->status = CY_ERR_ARG;
      return CY_OK;
    }
    o->threads = 256;
    o->tile = 256;
    o->slots = 1 + K;
    tiles = (R + 255) / 256;
  } else {
    o->vec = align % 16 == 0 ? 4 : 1;
    const int q = K / gcd_i(K, o->vec);
    o->threads = (256 / q) * q;
    o->tile = o->threads * o->vec * IMSAT_DEPTH;
    o->slots = form == CY_IMSAT_PAIR ? 3 + 2 * K : 1 + K;
    tiles = (R * (long)K + o->tile - 1) / o->tile;
  }
  o->fwd_grid = cy_blocks(tiles, 1, IMSAT_FWD_CAP);  // a block takes whole tiles
  o->bwd_grid = cy_blocks(tiles, 1, IMSAT_BWD_CAP);
  o->fwd_trips = cy_trips(tiles, o->fwd_grid, 1);
  o->bwd_trips = cy_trips(tiles, o->bwd_grid, 1);
  return CY_OK;
}

size_t plan_ws_bytes(int form, long R, int K) {
  ImsatPlan p;
  // sized for the 4-byte form of the sweep: the slots do not depend on the alignment, and its tile is the smaller one,
  // so its grid is never the smaller (the pixel form's grid does not depend on the alignment at all)
  if (plan_fill(form, R, K, form == CY_IMSAT_LOGITS ? 16 : 4, &p) != CY_OK || p.status != CY_OK) return 0;
  return (size_t)p.slots * (size_t)p.fwd_grid * sizeof(double);
}

// ---------------------------------------------------------------- flat sweep
template <int V>
__device__ __forceinline__ void load_chunk(const float* __restrict__ x, long e, long n, float* v) {
  if (V == 4 && e + 4 <= n) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + e);
    v[0] = a[0], v[1] = a[1], v[2] = a[2], v[3] = a[3];
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = (e + i < n) ? x[e + i] : 0.f;  // p = 0 adds exactly 0 to every sum
  }
}

template <int V>
__device__ __forceinline__ void store_chunk(float* __restrict__ d, long e, long n, const float* v) {
  if (V == 4 && e + 4 <= n) {
    f32x4 o;
    o[0] = v[0], o[1] = v[1], o[2] = v[2], o[3] = v[3];
    *reinterpret_cast<f32x4*>(d + e) = o;
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i)
      if (e + i < n) d[e + i] = v[i];
  }
}

// the K column sums of a block: element f = V*tid + i of the block's chunk belongs to column f % K
template <int V>
__device__ __forceinline__ void column_sums(const double* acc, double* sh, int K, int threads, double* __restrict__ ws,
                                            int slot0) {
  __syncthreads();
#pragma unroll
  for (int i = 0; i < V; ++i) sh[threadIdx.x * V + i] = acc[i];
  __syncthreads();
  if ((int)threadIdx.x < K) {
    double s = 0.0;
    for (int f = threadIdx.x; f < threads * V; f += K) s += sh[f];
    ws[(size_t)(slot0 + threadIdx.x) * gridDim.x + blockIdx.x] = s;
  }
}

__device__ __forceinline__ void scalar_sum(double v, double* sh, double* __restrict__ ws, int slot) {
  const double tot = block_sum_d(v, sh);
  if (threadIdx.x == 0) ws[(size_t)slot * gridDim.x + blockIdx.x] = tot;
}

// slots (slot-major, one value per block): rows {cond, col[K]}; pair {cond1, cond2, sum (x1-x2)^2, col1[K], col2[K]}
template <int V, bool PAIR>
__global__ void __launch_bounds__(256)
    imsat_fwd_kernel(const float* __restrict__ x1, const float* __restrict__ x2, double* __restrict__ ws, long n, int K,
                     int threads, float eps) {
  __shared__ double sh[256 * V];
  const int tid = threadIdx.x;
  double cond1 = 0.0, cond2 = 0.0, sq = 0.0, col1[V], col2[V];
#pragma unroll
  for (int i = 0; i < V; ++i) col1[i] = col2[i] = 0.0;
  if (tid < threads) {
    const long step = (long)threads * V;
    const long tile = step * IMSAT_DEPTH;
    const long ntile = (n + tile - 1) / tile;
    for (long t = blockIdx.x; t < ntile; t += gridDim.x) {
      const long e0 = t * tile + (long)tid * V;
      float a[IMSAT_DEPTH][V], b[IMSAT_DEPTH][V];
#pragma unroll
      for (int u = 0; u < IMSAT_DEPTH; ++u) {
        load_chunk<V>(x1, e0 + u * step, n, a[u]);
        if (PAIR) load_chunk<V>(x2, e0 + u * step, n, b[u]);
      }
#pragma unroll
      for (int u = 0; u < IMSAT_DEPTH; ++u)
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const float p = a[u][i];
          cond1 += (double)(-p * logf(p + eps));
          col1[i] += (double)p;
          if (PAIR) {
            const float q = b[u][i];
            cond2 += (double)(-q * logf(q + eps));
            col2[i] += (double)q;
            const float d = p - q;
            sq += (double)(d * d);
          }
        }
    }
  }
  scalar_sum(cond1, sh, ws, 0);
  if (PAIR) {
    scalar_sum(cond2, sh, ws, 1);
    scalar_sum(sq, sh, ws, 2);
  }
  column_sums<V>(col1, sh, K, threads, ws, PAIR ? 3 : 1);
  if (PAIR) column_sums<V>(col2, sh, K, threads, ws, 3 + K);
}

// one block: slot s is summed by wave s % 4, lane l taking the blocks l, l + 64, ... and the lanes folding at
// offsets 32 .. 1 -- an order the grid alone decides.  nin inputs: out = {marg, cond} per input (+ the MSE for two),
// coef / mean [nin][K].
__global__ void __launch_bounds__(256)
    imsat_finalize_kernel(const double* __restrict__ ws, int nblk, int K, int nin, double R, float eps,
                          float* __restrict__ out, float* __restrict__ coef, float* __restrict__ mean) {
  __shared__ double tot[3 + 2 * IMSAT_KMAX];
  __shared__ double term[2 * IMSAT_KMAX];
  const int nscal = nin == 1 ? 1 : 3;
  const int slots = nscal + nin * K;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s = wave; s < slots; s += 4) {
    double acc = 0.0;
    for (int b = lane; b < nblk; b += 64) acc += ws[(size_t)s * nblk + b];
    acc = wave_sum(acc);
    if (lane == 0) tot[s] = acc;
  }
  __syncthreads();
  const double e = (double)eps;
  for (int k = threadIdx.x; k < nin * K; k += 256) {
    const double m = tot[nscal + k] / R;
    const double lg = log(m + e);
    mean[k] = (float)m;
    coef[k] = (float)(-(lg + m / (m + e)) / R);
    term[k] = -m * lg;
  }
  __syncthreads();
  if ((int)threadIdx.x < nin) {
    double marg = 0.0;
    for (int k = 0; k < K; ++k) marg += term[threadIdx.x * K + k];
    out[2 * threadIdx.x] = (float)marg;
    out[2 * threadIdx.x + 1] = (float)(tot[threadIdx.x] / R);
  }
  if (nin == 2 && threadIdx.x == 2) out[4] = (float)(tot[2] / (R * (double)K));
}

// dp = g[1] dcond/dp + g[0] c_k;  pair: g = {marg1, cond1, marg2, cond2, mse}, d(mse)/dx1 = 2 (x1 - x2) / (R K)
template <int V, bool PAIR>
__global__ void __launch_bounds__(256)
    imsat_bwd_kernel(const float* __restrict__ x1, const float* __restrict__ x2, const float* __restrict__ coef,
                     const float* __restrict__ g, float* __restrict__ d1, float* __restrict__ d2, long n, int K,
                     int threads, float eps, float inv_r) {
  const int tid = threadIdx.x;
  if (tid >= threads) return;
  float c1[V], c2[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int k = (tid * V + i) % K;
    c1[i] = g[0] * coef[k];
    c2[i] = PAIR ? g[2] * coef[K + k] : 0.f;
  }
  const float gc1 = g[1] * inv_r;
  const float gc2 = PAIR ? g[3] * inv_r : 0.f;
  const float gm = PAIR ? g[4] * 2.f * inv_r / (float)K : 0.f;
  const long step = (long)threads * V;
  const long tile = step * IMSAT_DEPTH;
  const long ntile = (n + tile - 1) / tile;
  for (long t = blockIdx.x; t < ntile; t += gridDim.x) {
    const long e0 = t * tile + (long)tid * V;
    float a[IMSAT_DEPTH][V], b[IMSAT_DEPTH][V];
#pragma unroll
    for (int u = 0; u < IMSAT_DEPTH; ++u) {
      load_chunk<V>(x1, e0 + u * step, n, a[u]);
      if (PAIR) load_chunk<V>(x2, e0 + u * step, n, b[u]);
    }
#pragma unroll
    for (int u = 0; u < IMSAT_DEPTH; ++u) {
      float o1[V], o2[V];
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const float p = a[u][i], pe = p + eps;
        o1[i] = fmaf(gc1, -(logf(pe) + p / pe), c1[i]);
        if (PAIR) {
          const float q = b[u][i], qe = q + eps;
          const float dm = gm * (p - q);
          o1[i] += dm;
          o2[i] = fmaf(gc2, -(logf(qe) + q / qe), c2[i]) - dm;
        }
      }
      store_chunk<V>(d1, e0 + u * step, n, o1);
      if (PAIR) store_chunk<V>(d2, e0 + u * step, n, o2);
    }
  }
}

// ---------------------------------------------------------------- from logits, one thread per pixel
template <int KT>
__global__ void __launch_bounds__(256)
    softmax_imsat_fwd_kernel(const float* __restrict__ logits, double* __restrict__ ws, long npix, int Krt, float eps) {
  const int K = KT ? KT : Krt;
  __shared__ double sh[256];
  double cond = 0.0, col[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) col[k] = 0.0;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float z[KMAX], pr[KMAX];
    load_row<KT>(logits, p, K, z);
    softmax_k(z, pr, K);
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        cond += (double)(-pr[k] * logf(pr[k] + eps));
        col[k] += (double)pr[k];
      }
  }
  scalar_sum(cond, sh, ws, 0);
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) scalar_sum(col[k], sh, ws, 1 + k);
}

// a_k = g[1] dcond/dp_k + g[0] c_k;  dz_k = p_k (a_k - sum_j p_j a_j)
template <int KT>
__global__ void __launch_bounds__(256)
    softmax_imsat_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ coef,
                             const float* __restrict__ g, float* __restrict__ dlogits, long npix, int Krt, float eps,
                             float inv_r) {
  const int K = KT ? KT : Krt;
  // g[0] c_k through LDS: as sixteen wave-uniform values they sit in scalar registers, which the run-time form then
  // runs out of
  __shared__ float c[KMAX];
  if ((int)threadIdx.x < K) c[threadIdx.x] = g[0] * coef[threadIdx.x];
  __syncthreads();
  const float gc = g[1] * inv_r;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float z[KMAX], pr[KMAX], a[KMAX];
    load_row<KT>(logits, p, K, z);
    softmax_k(z, pr, K);
    // a is shifted by its value at the most probable class before the projection: sum_j p_j = 1, so the shift changes
    // nothing, and the difference a_k - sum_j p_j a_j no longer cancels where one class holds almost all the mass or
    // where the a_k are nearly equal (balanced marginals under g[0] alone)
    float pmax = -1.f, shift = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        const float q = pr[k] + eps;
        a[k] = fmaf(gc, -(logf(q) + pr[k] / q), c[k]);
        if (pr[k] > pmax) pmax = pr[k], shift = a[k];
      } else {
        pr[k] = a[k] = 0.f;  // absent classes: the two loops below run over all KMAX without a test (p = 0 adds 0)
      }
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      a[k] -= shift;
      dot = fmaf(pr[k], a[k], dot);
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k) a[k] = pr[k] * (a[k] - dot);
    store_row<KT>(dlogits, p, K, a);
  }
}

#define IMSAT_LAUNCH_BY_KT(KERNEL, KTV, GRID, ST, ...)                                  \
  do {                                                                                 \
    if ((KTV) == 2)                                                                    \
      hipLaunchKernelGGL(KERNEL<2>, dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);        \
    else if ((KTV) == 4)                                                               \
      hipLaunchKernelGGL(KERNEL<4>, dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);        \
    else if ((KTV) == 8)                                                               \
      hipLaunchKernelGGL(KERNEL<8>, dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);        \
    else                                                                               \
      hipLaunchKernelGGL(KERNEL<0>, dim3(GRID), dim3(256), 0, ST, __VA_ARGS__);        \
    CY_CHECK_LAUNCH();                                                                 \
  } while (0)

template <bool PAIR>
int sweep_fwd(const float* x1, const float* x2, float* out, float* coef, float* mean, long R, int K, float eps,
              void* ws, size_t ws_bytes, void* stream) {
  const int form = PAIR ? CY_IMSAT_PAIR : CY_IMSAT_ROWS;
  if (!x1 || (PAIR && !x2) || !out || !coef || !mean || !ws || R < 1) return CY_ERR_ARG;
  ImsatPlan p;
  plan_fill(form, R, K, PAIR ? common_align({x1, x2}) : common_align({x1}), &p);
  if (p.status != CY_OK) return p.status;
  if (ws_bytes < plan_ws_bytes(form, R, K)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const long n = R * (long)K;
  if (p.vec == 4)
    hipLaunchKernelGGL((imsat_fwd_kernel<4, PAIR>), dim3(p.fwd_grid), dim3(256), 0, st, x1, x2, (double*)ws, n, K,
                       p.threads, eps);
  else
    hipLaunchKernelGGL((imsat_fwd_kernel<1, PAIR>), dim3(p.fwd_grid), dim3(256), 0, st, x1, x2, (double*)ws, n, K,
                       p.threads, eps);
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(imsat_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, p.fwd_grid, K, PAIR ? 2 : 1,
                     (double)R, eps, out, coef, mean);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

template <bool PAIR>
int sweep_bwd(const float* x1, const float* x2, const float* coef, const float* g, float* d1, float* d2, long R, int K,
              float eps, void* stream) {
  if (!x1 || (PAIR && (!x2 || !d2)) || !coef || !g || !d1 || R < 1) return CY_ERR_ARG;
  ImsatPlan p;
  plan_fill(PAIR ? CY_IMSAT_PAIR : CY_IMSAT_ROWS, R, K, PAIR ? common_align({x1, x2, d1, d2}) : common_align({x1, d1}),
            &p);
  if (p.status != CY_OK) return p.status;
  const long n = R * (long)K;
  const float inv_r = (float)(1.0 / (double)R);
  if (p.vec == 4)
    hipLaunchKernelGGL((imsat_bwd_kernel<4, PAIR>), dim3(p.bwd_grid), dim3(256), 0, (hipStream_t)stream, x1, x2, coef,
                       g, d1, d2, n, K, p.threads, eps, inv_r);
  else
    hipLaunchKernelGGL((imsat_bwd_kernel<1, PAIR>), dim3(p.bwd_grid), dim3(256), 0, (hipStream_t)stream, x1, x2, coef,
                       g, d1, d2, n, K, p.threads, eps, inv_r);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

}  // namespace

extern "C" {

int cy_imsat_plan(int form, long R, int K, int align, cy_imsat_plan_t* out) {
  ImsatPlan p;
  if (!out) return CY_ERR_ARG;
  const int rc = plan_fill(form, R, K, align, &p);
  if (rc != CY_OK || p.status != CY_OK) return rc != CY_OK ? rc : p.status;
  out->vec = p.vec, out->kt = p.kt, out->threads = p.threads, out->tile = p.tile, out->slots = p.slots;
  out->fwd_grid = p.fwd_grid, out->fwd_trips = p.fwd_trips, out->bwd_grid = p.bwd_grid, out->bwd_trips = p.bwd_trips;
  return CY_OK;
}

size_t cy_imsat_ws_bytes(long R, int K) { return plan_ws_bytes(CY_IMSAT_ROWS, R, K); }

int cy_imsat_fwd(const float* p, float* out, float* coef, float* mean, long R, int K, float eps, void* ws,
                 size_t ws_bytes, void* stream) {
  return sweep_fwd<false>(p, nullptr, out, coef, mean, R, K, eps, ws, ws_bytes, stream);
}

int cy_imsat_bwd(const float* p, const float* coef, const float* g, float* dp, long R, int K, float eps, void* stream) {
  return sweep_bwd<false>(p, nullptr, coef, g, dp, nullptr, R, K, eps, stream);
}

size_t cy_imsat_pair_ws_bytes(long R, int K) { return plan_ws_bytes(CY_IMSAT_PAIR, R, K); }

int cy_imsat_pair_fwd(const float* x1, const float* x2, float* out, float* coef, float* mean, long R, int K, float eps,
                      void* ws, size_t ws_bytes, void* stream) {
  return sweep_fwd<true>(x1, x2, out, coef, mean, R, K, eps, ws, ws_bytes, stream);
}

int cy_imsat_pair_bwd(const float* x1, const float* x2, const float* coef, const float* g, float* dx1, float* dx2,
                      long R, int K, float eps, void* stream) {
  return sweep_bwd<true>(x1, x2, coef, g, dx1, dx2, R, K, eps, stream);
}

size_t cy_softmax_imsat_ws_bytes(long npix, int K) { return plan_ws_bytes(CY_IMSAT_LOGITS, npix, K); }

int cy_softmax_imsat_fwd(const float* logits, float* out, float* coef, float* mean, long npix, int K, float eps,
                         void* ws, size_t ws_bytes, void* stream) {
  if (!logits || !out || !coef || !mean || !ws || npix < 1) return CY_ERR_ARG;
  ImsatPlan p;
  plan_fill(CY_IMSAT_LOGITS, npix, K, common_align({logits}), &p);
  if (p.status != CY_OK) return p.status;
  if (ws_bytes < plan_ws_bytes(CY_IMSAT_LOGITS, npix, K)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  IMSAT_LAUNCH_BY_KT(softmax_imsat_fwd_kernel, p.kt, p.fwd_grid, st, logits, (double*)ws, npix, K, eps);
  hipLaunchKernelGGL(imsat_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, p.fwd_grid, K, 1,
                     (double)npix, eps, out, coef, mean);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_softmax_imsat_bwd(const float* logits, const float* coef, const float* g, float* dlogits, long npix, int K,
                         float eps, void* stream) {
  if (!logits || !coef || !g || !dlogits || npix < 1) return CY_ERR_ARG;
  ImsatPlan p;
  plan_fill(CY_IMSAT_LOGITS, npix, K, common_align({logits, dlogits}), &p);
  if (p.status != CY_OK) return p.status;
  IMSAT_LAUNCH_BY_KT(softmax_imsat_bwd_kernel, p.kt, p.bwd_grid, (hipStream_t)stream, logits, coef, g, dlogits, npix,
                     K, eps, (float)(1.0 / (double)npix));
  return CY_OK;
}

}  // extern "C"
