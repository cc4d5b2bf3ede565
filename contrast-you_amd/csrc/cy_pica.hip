// PICA losses, Jensen-Shannon divergence and entropy prior on probability maps.
//   PUILoss / PUISegLoss        contrastyou/losses/pica_loss.py:10-85
//   JSD_div / EntropyPrior      contrastyou/losses/kl.py:63-78,142-174
// The two PICA losses take their joints from cy_joint_fwd / cy_joint_bwd (csrc/cy_mi.hip); here are the single-block
// finishing kernels (f64 inside, forward plus analytic dJ, in the style of iid_loss_kernel) and the streaming kernels of
// the balance terms.  JSD and the entropy prior are one streaming pass each way: one thread per position, f64 block
// partials, a fixed-order final sum.  No atomics anywhere.
#include "cy_common.h"
#include "cy_reduce.h"

namespace {

constexpr int PK_KMAX = 64;  // max classes (J_KMAX of cy_mi.hip)
constexpr int JSD_MMAX = 8;  // max maps of JSD_div

constexpr int STREAM_GRID_CAP = 1024;  // blocks of 256 positions (= f64 partials) of the streaming kernels

// ---------------------------------------------------------------- PUILoss on [N][K] rows
// stats[0][K] = sum_n x^2, stats[1][K] = sum_n y^2, stats[2][K] = sum_n x.  One block: thread (slice, column), rows
// slice-strided, the slices added in order.
__global__ void __launch_bounds__(256)
    pui_stats_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ stats, long N, int K) {
  __shared__ double sred[3][256];
  const int nsl = 256 / K, sl = threadIdx.x / K, c = threadIdx.x - sl * K;
  double a = 0.0, b = 0.0, s = 0.0;
  if (sl < nsl)
    for (long n = sl; n < N; n += nsl) {
      const double xv = x[n * K + c], yv = y[n * K + c];
      a += xv * xv;
      b += yv * yv;
      s += xv;
    }
  sred[0][threadIdx.x] = a;
  sred[1][threadIdx.x] = b;
  sred[2][threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < K) {
    for (int w = 0; w < 3; ++w) {
      double t = 0.0;
      for (int u = 0; u < nsl; ++u) t += sred[w][u * K + threadIdx.x];
      stats[w * K + threadIdx.x] = (float)t;
    }
  }
}

// J[K][K] = sum_n x_ni y_nj.  a_i = max(|x_.i|, 1e-12), b_j likewise, pui = J / (a b);
// out[0] = mean_i [logsumexp_j pui_ij - pui_ii] + lamda (log K + sum_i p_i log p_i), p = mean_n x.
// dJ = dloss/dJ; coef[0][K]: dloss/dx_ni = ... + x_ni coef0_i + coef2_i, coef[1][K]: dloss/dy_nj = ... + y_nj coef1_j
// (through the norms; a clamped norm is a constant), coef[2][K] = lamda (log p_i + 1) / N.
__global__ void __launch_bounds__(256)
    pui_loss_kernel(const float* __restrict__ J, const float* __restrict__ stats, float* __restrict__ out,
                    float* __restrict__ dJ, float* __restrict__ coef, long N, int K, float lamda) {
  __shared__ double sred[256];
  __shared__ double a[PK_KMAX], b[PK_KMAX], lse[PK_KMAX], ga[PK_KMAX], gb[PK_KMAX];
  const int tid = threadIdx.x;
  if (tid < K) {
    a[tid] = fmax(sqrt((double)stats[tid]), 1e-12);
    b[tid] = fmax(sqrt((double)stats[K + tid]), 1e-12);
  }
  __syncthreads();
  if (tid < K) {
    double mx = -1e300;
    for (int j = 0; j < K; ++j) mx = fmax(mx, (double)J[tid * K + j] / (a[tid] * b[j]));
    double s = 0.0;
    for (int j = 0; j < K; ++j) s += exp((double)J[tid * K + j] / (a[tid] * b[j]) - mx);
    lse[tid] = mx + log(s);
  }
  __syncthreads();
  double l = 0.0;
  if (tid < K) {
    const double p = (double)stats[2 * K + tid] / (double)N;
    l = (lse[tid] - (double)J[tid * K + tid] / (a[tid] * b[tid])) / (double)K + (double)lamda * p * log(p);
    if (coef) coef[2 * K + tid] = (float)((double)lamda * (log(p) + 1.0) / (double)N);
  }
  l = block_sum_d(l, sred);
  if (tid == 0) out[0] = (float)(l + (double)lamda * log((double)K));
  if (!dJ) return;
  // dpui_ij = (softmax_ij - delta_ij) / K;  dJ_ij = dpui_ij / (a_i b_j);  da_i = -sum_j dpui_ij pui_ij / a_i
  for (int e = tid; e < K * K; e += 256) {
    const int i = e / K, j = e - i * K;
    const double pui = (double)J[e] / (a[i] * b[j]);
    const double dp = (exp(pui - lse[i]) - (i == j ? 1.0 : 0.0)) / (double)K;
    dJ[e] = (float)(dp / (a[i] * b[j]));
  }
  if (tid < K) {
    double sa = 0.0, sb = 0.0;
    for (int o = 0; o < K; ++o) {
      const double pr = (double)J[tid * K + o] / (a[tid] * b[o]);  // row tid: towards a_tid
      sa += (exp(pr - lse[tid]) - (o == tid ? 1.0 : 0.0)) / (double)K * pr;
      const double pc = (double)J[o * K + tid] / (a[o] * b[tid]);  // column tid: towards b_tid
      sb += (exp(pc - lse[o]) - (o == tid ? 1.0 : 0.0)) / (double)K * pc;
    }
    // a = sqrt(s): da/dx_n = x_n / a, so dloss/dx_n = -(sa / a) x_n / a; zero where the norm is clamped
    ga[tid] = sqrt((double)stats[tid]) > 1e-12 ? -sa / (a[tid] * a[tid]) : 0.0;
    gb[tid] = sqrt((double)stats[K + tid]) > 1e-12 ? -sb / (b[tid] * b[tid]) : 0.0;
    coef[tid] = (float)ga[tid];
    coef[K + tid] = (float)gb[tid];
  }
}

// dx[r][c] += g[0] * (x[r][c] * a[c] + b[c])   (b may be NULL)
__global__ void __launch_bounds__(256)
    rows_axpb_kernel(const float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ b,
                     const float* __restrict__ g, float* __restrict__ dx, long total, int K) {
  const float gs = g[0];
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const int c = (int)(e % K);
    dx[e] += gs * (x[e] * a[c] + (b ? b[c] : 0.f));
  }
}

// ---------------------------------------------------------------- PUISegLoss
// the balance term over the permuted tensor: p_m = (1/k) sum_c x[m][c] per pixel; part[block] = sum_m p_m log p_m
__global__ void __launch_bounds__(256)
    pixmean_entropy_fwd_kernel(const float* __restrict__ x, double* __restrict__ part, long M, int k) {
  __shared__ double sred[256];
  double s = 0.0;
  for (long m = blockIdx.x * 256L + threadIdx.x; m < M; m += (long)gridDim.x * 256L) {
    double p = 0.0;
    for (int c = 0; c < k; ++c) p += (double)x[m * k + c];
    p /= (double)k;
    s += p * log(p);
  }
  s = block_sum_d(s, sred);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// dx[m][c] += g[0] * lamda * (log p_m + 1) / k
__global__ void __launch_bounds__(256)
    pixmean_entropy_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ dx, long M,
                               int k, float lamda) {
  const double gs = (double)g[0] * (double)lamda / (double)k;
  for (long m = blockIdx.x * 256L + threadIdx.x; m < M; m += (long)gridDim.x * 256L) {
    double p = 0.0;
    for (int c = 0; c < k; ++c) p += (double)x[m * k + c];
    p /= (double)k;
    const float v = (float)(gs * (log(p) + 1.0));
    for (int c = 0; c < k; ++c) dx[m * k + c] += v;
  }
}

// J[TT][k][k] displaced joint.  q_d = (J_d - min J + 1e-16) / S_d, S_d its sum; P = mean_d (q_d + q_d^T) / 2 (only its
// diagonal is read, on which the symmetrisation changes nothing); ce = -(1/k^2) sum_i log(P_ii + 1e-16);
// out[0] = ce + lamda (log M + sum of part[nblk]);  dJ = dce/dJ (the minimum is a constant, as the reference detaches it).
// ws: TT + k doubles.
__global__ void __launch_bounds__(256)
    puiseg_loss_kernel(const float* __restrict__ J, const double* __restrict__ part, int nblk, float* __restrict__ out,
                       float* __restrict__ dJ, double* __restrict__ ws, int TT, int k, long M, float lamda) {
  __shared__ double sred[256];
  __shared__ double diag[PK_KMAX], dP[PK_KMAX];
  const int tid = threadIdx.x, kk = k * k, n = TT * kk;
  double* S = ws;  // [TT]
  double mn = 1e300;
  for (int e = tid; e < n; e += 256) mn = fmin(mn, (double)J[e]);
  mn = block_min_d(mn, sred);
  for (int d = 0; d < TT; ++d) {
    double s = 0.0;
    for (int e = tid; e < kk; e += 256) s += (double)J[d * kk + e] - mn + 1e-16;
    s = block_sum_d(s, sred);
    if (tid == 0) S[d] = s;
  }
  __syncthreads();
  if (tid < k) {
    double t = 0.0;
    for (int d = 0; d < TT; ++d) t += ((double)J[d * kk + tid * k + tid] - mn + 1e-16) / S[d];
    diag[tid] = t / (double)TT;
    dP[tid] = -1.0 / ((double)kk * (diag[tid] + 1e-16));
  }
  __syncthreads();
  double l = tid < k ? -log(diag[tid] + 1e-16) / (double)kk : 0.0;
  double ne = 0.0;
  for (int b = tid; b < nblk; b += 256) ne += part[b];
  l = block_sum_d(l, sred);
  ne = block_sum_d(ne, sred);
  if (tid == 0) out[0] = (float)(l + (double)lamda * (log((double)M) + ne));
  if (!dJ) return;
  // dq_d[i][j] = delta_ij dP_i / TT;  dJ_d = (dq_d - <dq_d, q_d>) / S_d
  for (int d = tid; d < TT; d += 256) {
    double dot = 0.0;
    for (int i = 0; i < k; ++i) dot += dP[i] / (double)TT * ((double)J[d * kk + i * k + i] - mn + 1e-16) / S[d];
    ws[TT + d] = dot;
  }
  __syncthreads();
  for (int e = tid; e < n; e += 256) {
    const int d = e / kk, r = e - d * kk, i = r / k, j = r - i * k;
    dJ[e] = (float)(((i == j ? dP[i] / (double)TT : 0.0) - ws[TT + d]) / S[d]);
  }
}

// ---------------------------------------------------------------- JSD_div, EntropyPrior
struct maps_t {
  const float* p[JSD_MMAX];
};
struct grads_t {
  float* p[JSD_MMAX];
};

// position r of R, class c of C: element (r / S) * C * S + c * S + r % S of an NCHW map (S positions per image), or
// r * C + c of rows / an NHWC map (S = 1)
__device__ __forceinline__ long pos_base(long r, int C, long S) { return S == 1 ? r * C : (r / S) * C * S + r % S; }

// v_r = H(mean_i x_i[r]) - mean_i H(x_i[r]), H(p) = -sum_c p log(p + eps).  out_map[r] = v_r (reduction "none"), or
// part[block] = sum of the block's v_r
__global__ void __launch_bounds__(256)
    jsd_fwd_kernel(maps_t x, int m, float* __restrict__ out_map, double* __restrict__ part, long R, int C, long S,
                   double eps) {
  __shared__ double sred[256];
  double s = 0.0;
  for (long r = blockIdx.x * 256L + threadIdx.x; r < R; r += (long)gridDim.x * 256L) {
    const long base = pos_base(r, C, S);
    double hm = 0.0, he = 0.0;
    for (int c = 0; c < C; ++c) {
      double mean = 0.0;
      for (int i = 0; i < m; ++i) {
        const double v = (double)x.p[i][base + c * S];
        mean += v;
        he -= v * log(v + eps);
      }
      mean /= (double)m;
      hm -= mean * log(mean + eps);
    }
    const double v = hm - he / (double)m;
    if (out_map) out_map[r] = (float)v;
    s += v;
  }
  if (part) {
    s = block_sum_d(s, sred);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
  }
}

// out[0] = add + scale * sum of part[n], in a fixed order
__global__ void __launch_bounds__(256)
    final_sum_kernel(const double* __restrict__ part, int n, float* __restrict__ out, double scale, double add) {
  __shared__ double sred[256];
  const double s = sum_partials_d(part, n, 1, sred);
  if (threadIdx.x == 0) out[0] = (float)(add + scale * s);
}

// dv_r/dx_i[c] = (1/m) [(log(x + eps) + x / (x + eps)) - (log(mean + eps) + mean / (mean + eps))];
// upstream g[r] (per_pos) or g[0], times scale
__global__ void __launch_bounds__(256)
    jsd_bwd_kernel(maps_t x, grads_t dx, int m, const float* __restrict__ g, int per_pos, double scale, long R, int C,
                   long S, double eps) {
  for (long r = blockIdx.x * 256L + threadIdx.x; r < R; r += (long)gridDim.x * 256L) {
    const long base = pos_base(r, C, S);
    const double gs = (double)g[per_pos ? r : 0] * scale / (double)m;
    for (int c = 0; c < C; ++c) {
      double mean = 0.0;
      for (int i = 0; i < m; ++i) mean += (double)x.p[i][base + c * S];
      mean /= (double)m;
      const double tm = log(mean + eps) + mean / (mean + eps);
      for (int i = 0; i < m; ++i) {
        if (!dx.p[i]) continue;
        const double v = (double)x.p[i][base + c * S];
        dx.p[i][base + c * S] = (float)(gs * (log(v + eps) + v / (v + eps) - tm));
      }
    }
  }
}

// EntropyPrior on rows [R][C] with a prior row [C]: part[block] = sum_r sum_c x (log(prior_c + eps) - log(x + eps))
__global__ void __launch_bounds__(256)
    prior_fwd_kernel(const float* __restrict__ x, const float* __restrict__ prior, double* __restrict__ part, long R,
                     int C, double eps) {
  __shared__ double sred[256];
  __shared__ double lp[PK_KMAX];
  if (threadIdx.x < C) lp[threadIdx.x] = log((prior ? (double)prior[threadIdx.x] : 1.0 / (double)C) + eps);
  __syncthreads();
  double s = 0.0;
  for (long r = blockIdx.x * 256L + threadIdx.x; r < R; r += (long)gridDim.x * 256L)
    for (int c = 0; c < C; ++c) {
      const double v = (double)x[r * C + c];
      s += v * (lp[c] - log(v + eps));
    }
  s = block_sum_d(s, sred);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// dx[r][c] = g[0] / R * (log(prior_c + eps) - log(x + eps) - x / (x + eps))
__global__ void __launch_bounds__(256)
    prior_bwd_kernel(const float* __restrict__ x, const float* __restrict__ prior, const float* __restrict__ g,
                     float* __restrict__ dx, long R, int C, double eps) {
  __shared__ double lp[PK_KMAX];
  if (threadIdx.x < C) lp[threadIdx.x] = log((prior ? (double)prior[threadIdx.x] : 1.0 / (double)C) + eps);
  __syncthreads();
  const double gs = (double)g[0] / (double)R;
  const long total = R * C;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const double v = (double)x[e];
    dx[e] = (float)(gs * (lp[e % C] - log(v + eps) - v / (v + eps)));
  }
}

int jsd_args(const float* const* maps, int m, long R, int C, long S, int reduction) {
  if (!maps || R < 1 || S < 1 || reduction < 0 || reduction > 2) return CY_ERR_ARG;
  if (m < 2 || m > JSD_MMAX || C < 1 || C > PK_KMAX) return CY_ERR_SHAPE;
  if (R % S != 0) return CY_ERR_SHAPE;
  for (int i = 0; i < m; ++i)
    if (!maps[i]) return CY_ERR_ARG;
  return CY_OK;
}

}  // namespace

extern "C" {

int cy_pui_stats(const float* x, const float* y, float* stats, long N, int K, void* stream) {
  if (!x || !y || !stats || N < 1) return CY_ERR_ARG;
  if (K < 1 || K > PK_KMAX) return CY_ERR_SHAPE;
  hipLaunchKernelGGL(pui_stats_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, y, stats, N, K);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_pui_loss(const float* J, const float* stats, float* out, float* dJ, float* coef, long N, int K, float lamda,
                void* stream) {
  if (!J || !stats || !out || !coef || N < 1) return CY_ERR_ARG;
  if (K < 1 || K > PK_KMAX) return CY_ERR_SHAPE;
  hipLaunchKernelGGL(pui_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, J, stats, out, dJ, coef, N, K, lamda);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_rows_axpb(const float* x, const float* a, const float* b, const float* g, float* dx, long R, int K,
                 void* stream) {
  if (!x || !a || !g || !dx || R < 1) return CY_ERR_ARG;
  if (K < 1 || K > PK_KMAX) return CY_ERR_SHAPE;
  hipLaunchKernelGGL(rows_axpb_kernel, dim3(cy_blocks(R * K, 256, STREAM_GRID_CAP)), dim3(256), 0, (hipStream_t)stream,
                     x, a, b, g, dx, R * K, K);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

size_t cy_stream_sum_ws_bytes(long R) {
  return R < 1 ? 0 : (size_t)cy_blocks(R, 256, STREAM_GRID_CAP) * sizeof(double);
}

size_t cy_puiseg_ws_bytes(long M, int TT, int k) {
  if (M < 1 || TT < 1 || k < 1 || k > PK_KMAX) return 0;
  return ((size_t)cy_blocks(M, 256, STREAM_GRID_CAP) + 2 * (size_t)TT) * sizeof(double);
}

int cy_puiseg_loss(const float* J, const float* x, float* out, float* dJ, int TT, int k, long M, float lamda, void* ws,
                   size_t ws_bytes, void* stream) {
  if (!J || !x || !out || TT < 1 || M < 1) return CY_ERR_ARG;
  if (k < 1 || k > PK_KMAX) return CY_ERR_SHAPE;
  if (!ws || ws_bytes < cy_puiseg_ws_bytes(M, TT, k)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = cy_blocks(M, 256, STREAM_GRID_CAP);
  double* part = (double*)ws;
  hipLaunchKernelGGL(pixmean_entropy_fwd_kernel, dim3(nblk), dim3(256), 0, st, x, part, M, k);
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(puiseg_loss_kernel, dim3(1), dim3(256), 0, st, J, (const double*)part, nblk, out, dJ, part + nblk,
                     TT, k, M, lamda);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_puiseg_balance_bwd(const float* x, const float* g, float* dx, long M, int k, float lamda, void* stream) {
  if (!x || !g || !dx || M < 1) return CY_ERR_ARG;
  if (k < 1 || k > PK_KMAX) return CY_ERR_SHAPE;
  hipLaunchKernelGGL(pixmean_entropy_bwd_kernel, dim3(cy_blocks(M, 256, STREAM_GRID_CAP)), dim3(256), 0,
                     (hipStream_t)stream, x, g, dx, M, k, lamda);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_jsd_fwd(const float* const* maps, int m, float* out, long R, int C, long S, int reduction, float eps, void* ws,
               size_t ws_bytes, void* stream) {
  if (!out) return CY_ERR_ARG;
  const int rc = jsd_args(maps, m, R, C, S, reduction);
  if (rc != CY_OK) return rc;
  if (reduction != 0 && (!ws || ws_bytes < cy_stream_sum_ws_bytes(R))) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  maps_t x = {};
  for (int i = 0; i < m; ++i) x.p[i] = maps[i];
  const int nblk = cy_blocks(R, 256, STREAM_GRID_CAP);
  hipLaunchKernelGGL(jsd_fwd_kernel, dim3(nblk), dim3(256), 0, st, x, m, reduction == 0 ? out : (float*)nullptr,
                     reduction == 0 ? (double*)nullptr : (double*)ws, R, C, S, (double)eps);
  CY_CHECK_LAUNCH();
  if (reduction != 0) {
    hipLaunchKernelGGL(final_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, nblk, out,
                       reduction == 1 ? 1.0 / (double)R : 1.0, 0.0);
    CY_CHECK_LAUNCH();
  }
  return CY_OK;
}

int cy_jsd_bwd(const float* const* maps, int m, const float* g, float* const* dmaps, long R, int C, long S,
               int reduction, float eps, void* stream) {
  if (!g || !dmaps) return CY_ERR_ARG;
  const int rc = jsd_args(maps, m, R, C, S, reduction);
  if (rc != CY_OK) return rc;
  maps_t x = {};
  grads_t dx = {};
  for (int i = 0; i < m; ++i) x.p[i] = maps[i], dx.p[i] = dmaps[i];
  hipLaunchKernelGGL(jsd_bwd_kernel, dim3(cy_blocks(R, 256, STREAM_GRID_CAP)), dim3(256), 0, (hipStream_t)stream, x, dx,
                     m, g, reduction == 0, reduction == 1 ? 1.0 / (double)R : 1.0, R, C, S, (double)eps);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_entropy_prior_fwd(const float* x, const float* prior, float* out, long R, int C, float eps, void* ws,
                         size_t ws_bytes, void* stream) {
  if (!x || !out || R < 1) return CY_ERR_ARG;
  if (C < 1 || C > PK_KMAX) return CY_ERR_SHAPE;
  if (!ws || ws_bytes < cy_stream_sum_ws_bytes(R)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = cy_blocks(R, 256, STREAM_GRID_CAP);
  hipLaunchKernelGGL(prior_fwd_kernel, dim3(nblk), dim3(256), 0, st, x, prior, (double*)ws, R, C, (double)eps);
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(final_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, nblk, out, 1.0 / (double)R,
                     log((double)C));
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_entropy_prior_bwd(const float* x, const float* prior, const float* g, float* dx, long R, int C, float eps,
                         void* stream) {
  if (!x || !g || !dx || R < 1) return CY_ERR_ARG;
  if (C < 1 || C > PK_KMAX) return CY_ERR_SHAPE;
  hipLaunchKernelGGL(prior_bwd_kernel, dim3(cy_blocks(R * C, 256, STREAM_GRID_CAP)), dim3(256), 0, (hipStream_t)stream,
                     x, prior, g, dx, R, C, (double)eps);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

}  // extern "C"
