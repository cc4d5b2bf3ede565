// The kernels around the GEMMs of the adversarial baseline's discriminator (contrastyou/arch/discriminator.py:17-43,
// semi_seg/epochers/comparable.py:141-187), f32 over NHWC rows:
//   softmax of the logits, concatenated behind the image            torch.cat([image, logits.softmax(1)], 1)
//   train-mode BatchNorm2d + LeakyReLU over rows [M][C]             nn.BatchNorm2d(C), nn.LeakyReLU(0.2)
//   plain LeakyReLU                                                 the layer behind the first convolution
//   sigmoid + binary cross-entropy against a constant label         nn.Sigmoid(), nn.BCELoss()
// The conventions of cy_pixel_reg.hip: grid-stride loops; every forward reduction writes f64 partials per block and a
// later launch sums them in a fixed order (no floating-point atomics: two runs give the same bits); arguments are
// checked before any launch.
#include "cy_common.h"
#include "cy_pixel_loss.h"
#include "cy_reduce.h"

namespace {

constexpr int CI_MAX = 4;        // image channels in front of the class probabilities
constexpr int BN_C_MAX = 1024;   // channels of a BatchNorm row
constexpr int BN_CHUNKS_MAX = 256;
constexpr int BN_ROWS_PER_LANE = 8;

// ---------------------------------------------------------------- softmax + concat
template <int KT>
__global__ void __launch_bounds__(256)
    softmax_cat_fwd_kernel(const float* __restrict__ image, const float* __restrict__ logits, float* __restrict__ out,
                           long npix, int Ci, int Krt) {
  const int K = KT ? KT : Krt;
  const int ld = Ci + K;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float z[KMAX], pr[KMAX];
    load_logits(logits, p, K, z);
    softmax_k(z, pr, K);
    float* o = out + p * ld;
#pragma unroll
    for (int c = 0; c < CI_MAX; ++c)
      if (c < Ci) o[c] = image[p * Ci + c];
    if (KT == 4 && Ci == 0) {
      f32x4 v;
      v[0] = pr[0], v[1] = pr[1], v[2] = pr[2], v[3] = pr[3];
      *reinterpret_cast<f32x4*>(o) = v;
    } else {
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) o[Ci + k] = pr[k];
    }
  }
}

template <int KT>
__global__ void __launch_bounds__(256)
    softmax_cat_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ dout,
                           float* __restrict__ dlogits, long npix, int Ci, int Krt) {
  const int K = KT ? KT : Krt;
  const int ld = Ci + K;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    float z[KMAX], pr[KMAX], g[KMAX];
    load_logits(logits, p, K, z);
    softmax_k(z, pr, K);
    const float* d = dout + p * ld + Ci;
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        g[k] = d[k];
        dot = fmaf(pr[k], g[k], dot);
      }
    if (KT == 4) {
      f32x4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = pr[k] * (g[k] - dot);
      *reinterpret_cast<f32x4*>(dlogits + p * 4) = v;
    } else {
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) dlogits[p * K + k] = pr[k] * (g[k] - dot);
    }
  }
}

// ---------------------------------------------------------------- BatchNorm + LeakyReLU over rows [M][C]
// Thread layout of every kernel of this family: a lane owns V adjacent channels (V = 4: one 16-byte access, when
// C % 4 == 0; else V = 1); `lpr` lanes (a power of two <= 64) cover a row segment, the 256 / lpr row lanes of a block
// take consecutive rows; blockIdx.x is the column tile, blockIdx.y the row chunk (grid-stride over the rows).
struct BnGeom {
  int V, ncv, lpr, rl, tiles, chunks;
};

inline BnGeom bn_geom(long M, int C) {
  BnGeom g;
  g.V = (C % 4 == 0) ? 4 : 1;
  g.ncv = C / g.V;
  g.lpr = 1;
  while (g.lpr < g.ncv && g.lpr < 64) g.lpr *= 2;
  g.rl = 256 / g.lpr;
  g.tiles = (g.ncv + g.lpr - 1) / g.lpr;
  long ch = (M + (long)g.rl * BN_ROWS_PER_LANE - 1) / ((long)g.rl * BN_ROWS_PER_LANE);
  g.chunks = (int)(ch < 1 ? 1 : (ch > BN_CHUNKS_MAX ? BN_CHUNKS_MAX : ch));
  return g;
}

template <int V> __device__ __forceinline__ void ld_v(const float* p, float* f) {
  if constexpr (V == 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
    f[0] = v[0], f[1] = v[1], f[2] = v[2], f[3] = v[3];
  } else {
    f[0] = p[0];
  }
}

template <int V> __device__ __forceinline__ void st_v(float* p, const float* f) {
  if constexpr (V == 4) {
    f32x4 v;
    v[0] = f[0], v[1] = f[1], v[2] = f[2], v[3] = f[3];
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
    p[0] = f[0];
  }
}

__device__ __forceinline__ float inv_std(float var, float eps) { return 1.f / sqrtf(var + eps); }

// sum of a[0..V), b[0..V) over the row lanes of the block, in a fixed tree order; the result is in row lane 0
template <int V>
__device__ __forceinline__ void bn_block_sum(double* a, double* b, double* sh, int lpr) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    sh[(2 * v) * 256 + tid] = a[v];
    sh[(2 * v + 1) * 256 + tid] = b[v];
  }
  __syncthreads();
  for (int o = 128; o >= lpr; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int q = 0; q < 2 * V; ++q) sh[q * 256 + tid] += sh[q * 256 + tid + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int v = 0; v < V; ++v) {
    a[v] = sh[(2 * v) * 256 + tid];
    b[v] = sh[(2 * v + 1) * 256 + tid];
  }
}

// partial[chunk][0][c] = sum (x - x[0][c]), partial[chunk][1][c] = sum (x - x[0][c])^2 over the chunk's rows: the
// differences are exact in f64, and the shift keeps the variance free of the cancellation of E[x^2] - E[x]^2
template <int V>
__global__ void __launch_bounds__(256)
    bn_rows_stats_kernel(const float* __restrict__ x, double* __restrict__ partial, long M, int C, int ncv, int lpr) {
  __shared__ double sh[2 * V * 256];
  const int cl = threadIdx.x & (lpr - 1), rl = threadIdx.x / lpr, nrl = 256 / lpr;
  const int cv = blockIdx.x * lpr + cl;
  const bool live = cv < ncv;
  double s1[V], s2[V];
  float x0[V];
#pragma unroll
  for (int v = 0; v < V; ++v) s1[v] = 0.0, s2[v] = 0.0, x0[v] = 0.f;
  if (live) {
    ld_v<V>(x + (long)cv * V, x0);
    for (long r = (long)blockIdx.y * nrl + rl; r < M; r += (long)gridDim.y * nrl) {
      float f[V];
      ld_v<V>(x + r * C + (long)cv * V, f);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const double d = (double)f[v] - (double)x0[v];
        s1[v] += d;
        s2[v] = fma(d, d, s2[v]);
      }
    }
  }
  bn_block_sum<V>(s1, s2, sh, lpr);
  if (live && rl == 0) {
    double* p = partial + (long)blockIdx.y * 2 * C + (long)cv * V;
#pragma unroll
    for (int v = 0; v < V; ++v) p[v] = s1[v], p[C + v] = s2[v];
  }
}

// mean, biased variance; nn.BatchNorm2d's running statistics (unbiased variance) and batch counter when given
__global__ void __launch_bounds__(256)
    bn_rows_stats_finalize_kernel(const float* __restrict__ x, const double* __restrict__ partial, int chunks, long M,
                                  int C, float* __restrict__ mean, float* __restrict__ var,
                                  float* __restrict__ running_mean, float* __restrict__ running_var,
                                  long long* __restrict__ tracked, float momentum) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < C) {
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < chunks; ++k) {
      s1 += partial[(long)k * 2 * C + c];
      s2 += partial[(long)k * 2 * C + C + c];
    }
    const double m = s1 / (double)M;
    double v = s2 / (double)M - m * m;
    if (v < 0.0) v = 0.0;
    const double mu = (double)x[c] + m;
    mean[c] = (float)mu;
    var[c] = (float)v;
    if (running_mean) {
      const double mom = (double)momentum;
      running_mean[c] = (float)((1.0 - mom) * (double)running_mean[c] + mom * mu);
      running_var[c] = (float)((1.0 - mom) * (double)running_var[c] + mom * v * ((double)M / (double)(M - 1)));
    }
  }
  if (tracked && c == 0) tracked[0] += 1;
}

template <int V>
__global__ void __launch_bounds__(256)
    bn_lrelu_fwd_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ var,
                        const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ y, long M,
                        int C, int ncv, int lpr, float eps, float slope) {
  const int cl = threadIdx.x & (lpr - 1), rl = threadIdx.x / lpr, nrl = 256 / lpr;
  const int cv = blockIdx.x * lpr + cl;
  if (cv >= ncv) return;
  float mu[V], sc[V], be[V];
  ld_v<V>(mean + (long)cv * V, mu);
  ld_v<V>(var + (long)cv * V, sc);
  ld_v<V>(beta + (long)cv * V, be);
  {
    float ga[V];
    ld_v<V>(gamma + (long)cv * V, ga);
#pragma unroll
    for (int v = 0; v < V; ++v) sc[v] = ga[v] * inv_std(sc[v], eps);
  }
  for (long r = (long)blockIdx.y * nrl + rl; r < M; r += (long)gridDim.y * nrl) {
    float f[V];
    ld_v<V>(x + r * C + (long)cv * V, f);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const float pre = fmaf(f[v] - mu[v], sc[v], be[v]);
      f[v] = pre > 0.f ? pre : pre * slope;
    }
    st_v<V>(y + r * C + (long)cv * V, f);
  }
}

// partial[chunk][0][c] = sum dz * xhat, partial[chunk][1][c] = sum dz, dz = dy * lrelu'(gamma * xhat + beta)
template <int V>
__global__ void __launch_bounds__(256)
    bn_lrelu_bwd_reduce_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                               const float* __restrict__ mean, const float* __restrict__ var,
                               const float* __restrict__ gamma, const float* __restrict__ beta,
                               double* __restrict__ partial, long M, int C, int ncv, int lpr, float eps, float slope) {
  __shared__ double sh[2 * V * 256];
  const int cl = threadIdx.x & (lpr - 1), rl = threadIdx.x / lpr, nrl = 256 / lpr;
  const int cv = blockIdx.x * lpr + cl;
  const bool live = cv < ncv;
  double s1[V], s2[V];
#pragma unroll
  for (int v = 0; v < V; ++v) s1[v] = 0.0, s2[v] = 0.0;
  if (live) {
    float mu[V], is[V], ga[V], be[V];
    ld_v<V>(mean + (long)cv * V, mu);
    ld_v<V>(var + (long)cv * V, is);
    ld_v<V>(gamma + (long)cv * V, ga);
    ld_v<V>(beta + (long)cv * V, be);
#pragma unroll
    for (int v = 0; v < V; ++v) is[v] = inv_std(is[v], eps);
    for (long r = (long)blockIdx.y * nrl + rl; r < M; r += (long)gridDim.y * nrl) {
      float f[V], g[V];
      ld_v<V>(x + r * C + (long)cv * V, f);
      ld_v<V>(dy + r * C + (long)cv * V, g);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const float xh = (f[v] - mu[v]) * is[v];
        const float pre = fmaf(ga[v], xh, be[v]);
        const float dz = pre > 0.f ? g[v] : g[v] * slope;
        s1[v] = fma((double)dz, (double)xh, s1[v]);
        s2[v] += (double)dz;
      }
    }
  }
  bn_block_sum<V>(s1, s2, sh, lpr);
  if (live && rl == 0) {
    double* p = partial + (long)blockIdx.y * 2 * C + (long)cv * V;
#pragma unroll
    for (int v = 0; v < V; ++v) p[v] = s1[v], p[C + v] = s2[v];
  }
}

__global__ void __launch_bounds__(256)
    bn_lrelu_bwd_finalize_kernel(const double* __restrict__ partial, int chunks, int C, float* __restrict__ dgamma,
                                 float* __restrict__ dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0;
  for (int k = 0; k < chunks; ++k) {
    s1 += partial[(long)k * 2 * C + c];
    s2 += partial[(long)k * 2 * C + C + c];
  }
  dgamma[c] = (float)s1;
  dbeta[c] = (float)s2;
}

// batch statistics: dx = gamma * invstd * (dz - dbeta / M - xhat * dgamma / M); running statistics: gamma * invstd * dz
template <int V>
__global__ void __launch_bounds__(256)
    bn_lrelu_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ mean,
                              const float* __restrict__ var, const float* __restrict__ gamma,
                              const float* __restrict__ beta, const float* __restrict__ dgamma,
                              const float* __restrict__ dbeta, float* __restrict__ dx, long M, int C, int ncv, int lpr,
                              float eps, float slope, int batch_stats) {
  const int cl = threadIdx.x & (lpr - 1), rl = threadIdx.x / lpr, nrl = 256 / lpr;
  const int cv = blockIdx.x * lpr + cl;
  if (cv >= ncv) return;
  float mu[V], is[V], ga[V], be[V], mg[V], mb[V];
  ld_v<V>(mean + (long)cv * V, mu);
  ld_v<V>(var + (long)cv * V, is);
  ld_v<V>(gamma + (long)cv * V, ga);
  ld_v<V>(beta + (long)cv * V, be);
#pragma unroll
  for (int v = 0; v < V; ++v) is[v] = inv_std(is[v], eps), mg[v] = 0.f, mb[v] = 0.f;
  if (batch_stats) {
    ld_v<V>(dgamma + (long)cv * V, mg);
    ld_v<V>(dbeta + (long)cv * V, mb);
    const float inv_m = (float)(1.0 / (double)M);
#pragma unroll
    for (int v = 0; v < V; ++v) mg[v] *= inv_m, mb[v] *= inv_m;
  }
  for (long r = (long)blockIdx.y * nrl + rl; r < M; r += (long)gridDim.y * nrl) {
    float f[V], g[V];
    ld_v<V>(x + r * C + (long)cv * V, f);
    ld_v<V>(dy + r * C + (long)cv * V, g);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const float xh = (f[v] - mu[v]) * is[v];
      const float pre = fmaf(ga[v], xh, be[v]);
      const float dz = pre > 0.f ? g[v] : g[v] * slope;
      f[v] = ga[v] * is[v] * (dz - mb[v] - xh * mg[v]);
    }
    st_v<V>(dx + r * C + (long)cv * V, f);
  }
}

// ---------------------------------------------------------------- plain LeakyReLU
// BWD: y = (x > 0 ? dy : dy * slope), from the input; else y = (x > 0 ? x : x * slope)
template <bool BWD, int V>
__global__ void __launch_bounds__(256)
    leaky_relu_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ y, long first,
                      long count, float slope) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < count; i += (long)gridDim.x * 256L) {
    const long e = first + i * V;
    float f[V], g[V];
    ld_v<V>(x + e, f);
    if (BWD) ld_v<V>(dy + e, g);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const float a = BWD ? g[v] : f[v];
      f[v] = f[v] > 0.f ? a : a * slope;
    }
    st_v<V>(y + e, f);
  }
}

// ---------------------------------------------------------------- sigmoid + BCE against a constant label
// -log(sigmoid(s)) = softplus(-s), -log(1 - sigmoid(s)) = softplus(s): no 1 - sigmoid(s) is ever formed
__device__ __forceinline__ float softplus_f(float t) { return fmaxf(t, 0.f) + log1pf(expf(-fabsf(t))); }

__device__ __forceinline__ float sigmoid_f(float t) {
  const float e = expf(-fabsf(t));
  return t >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

constexpr float BCE_CLAMP = 100.f;  // torch's BCELoss clamps the logarithms at -100

__global__ void __launch_bounds__(256)
    sigmoid_bce_fwd_kernel(const float* __restrict__ s, double* __restrict__ partial, long n, int positive) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
    const float t = positive ? -s[i] : s[i];
    acc += (double)fminf(softplus_f(t), BCE_CLAMP);
  }
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(256)
    sigmoid_bce_bwd_kernel(const float* __restrict__ s, const float* __restrict__ gscale, float* __restrict__ ds,
                           long n, int positive) {
  const float gs = (float)((double)gscale[0] / (double)n);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
    const float t = positive ? -s[i] : s[i];
    // d softplus(t) / dt = sigmoid(t); dt / ds = -1 for label 1: sigmoid(s) - 1 = -sigmoid(-s)
    const float d = softplus_f(t) > BCE_CLAMP ? 0.f : sigmoid_f(t);
    ds[i] = gs * (positive ? -d : d);
  }
}

inline bool bad_k(int K) { return K < 2 || K > KMAX; }
inline bool bad_ci(int Ci) { return Ci < 0 || Ci > CI_MAX; }
inline bool bad_c(int C) { return C < 1 || C > BN_C_MAX; }
inline bool bad_label(float l) { return !(l == 0.f || l == 1.f); }
inline bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }
constexpr int FLAT_GRID_CAP = 2048;  // blocks of 256 of the flat sweeps (256 CUs x 8); the rest is grid-stride

// launch KERNEL<4> or KERNEL<1> over the BatchNorm geometry `G`
#define CY_BN_LAUNCH(KERNEL, G, ST, ...)                                                                   \
  do {                                                                                                     \
    if ((G).V == 4)                                                                                        \
      hipLaunchKernelGGL(KERNEL<4>, dim3((G).tiles, (G).chunks), dim3(256), 0, ST, __VA_ARGS__);           \
    else                                                                                                   \
      hipLaunchKernelGGL(KERNEL<1>, dim3((G).tiles, (G).chunks), dim3(256), 0, ST, __VA_ARGS__);           \
    CY_CHECK_LAUNCH();                                                                                     \
  } while (0)

}  // namespace

extern "C" {

int cy_softmax_cat_fwd(const float* image, const float* logits, float* out, long npix, int Ci, int K, void* stream) {
  if (!logits || !out || npix <= 0 || bad_k(K) || bad_ci(Ci) || (Ci > 0) != (image != nullptr)) return CY_ERR_ARG;
  if (K == 4 && (misaligned(logits) || (Ci == 0 && misaligned(out)))) return CY_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (K == 4)
    hipLaunchKernelGGL(softmax_cat_fwd_kernel<4>, dim3(cy_blocks(npix, 256, FLAT_GRID_CAP)), dim3(256), 0, st, image,
                       logits, out, npix, Ci, K);
  else
    hipLaunchKernelGGL(softmax_cat_fwd_kernel<0>, dim3(cy_blocks(npix, 256, FLAT_GRID_CAP)), dim3(256), 0, st, image,
                       logits, out, npix, Ci, K);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_softmax_cat_bwd(const float* logits, const float* dout, float* dlogits, long npix, int Ci, int K,
                       void* stream) {
  if (!logits || !dout || !dlogits || npix <= 0 || bad_k(K) || bad_ci(Ci)) return CY_ERR_ARG;
  if (K == 4 && (misaligned(logits) || misaligned(dlogits))) return CY_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (K == 4)
    hipLaunchKernelGGL(softmax_cat_bwd_kernel<4>, dim3(cy_blocks(npix, 256, FLAT_GRID_CAP)), dim3(256), 0, st, logits,
                       dout, dlogits, npix, Ci, K);
  else
    hipLaunchKernelGGL(softmax_cat_bwd_kernel<0>, dim3(cy_blocks(npix, 256, FLAT_GRID_CAP)), dim3(256), 0, st, logits,
                       dout, dlogits, npix, Ci, K);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

size_t cy_bn_rows_ws_bytes(long M, int C) {
  if (M < 1 || bad_c(C)) return 0;
  return (size_t)bn_geom(M, C).chunks * 2 * (size_t)C * sizeof(double);
}

int cy_bn_rows_stats(const float* x, float* mean, float* var, long M, int C, float* running_mean, float* running_var,
                     long long* num_batches_tracked, float momentum, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !mean || !var || !ws || M < 2 || bad_c(C) || (running_mean != nullptr) != (running_var != nullptr))
    return CY_ERR_ARG;
  if (C % 4 == 0 && misaligned(x)) return CY_ERR_ARG;
  if (ws_bytes < cy_bn_rows_ws_bytes(M, C)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const BnGeom g = bn_geom(M, C);
  CY_BN_LAUNCH(bn_rows_stats_kernel, g, st, x, (double*)ws, M, C, g.ncv, g.lpr);
  hipLaunchKernelGGL(bn_rows_stats_finalize_kernel, dim3(cy_cdiv(C, 256)), dim3(256), 0, st, x, (const double*)ws,
                     g.chunks, M, C, mean, var, running_mean, running_var, num_batches_tracked, momentum);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_bn_lrelu_fwd(const float* x, const float* mean, const float* var, const float* gamma, const float* beta,
                    float* y, long M, int C, float eps, float slope, void* stream) {
  if (!x || !mean || !var || !gamma || !beta || !y || M < 1 || bad_c(C)) return CY_ERR_ARG;
  if (C % 4 == 0 && (misaligned(x) || misaligned(y) || misaligned(mean) || misaligned(var) || misaligned(gamma) ||
                     misaligned(beta)))
    return CY_ERR_ARG;
  const BnGeom g = bn_geom(M, C);
  CY_BN_LAUNCH(bn_lrelu_fwd_kernel, g, (hipStream_t)stream, x, mean, var, gamma, beta, y, M, C, g.ncv, g.lpr, eps,
               slope);
  return CY_OK;
}

int cy_bn_lrelu_bwd_reduce(const float* x, const float* dy, const float* mean, const float* var, const float* gamma,
                           const float* beta, float* dgamma, float* dbeta, long M, int C, float eps, float slope,
                           void* ws, size_t ws_bytes, void* stream) {
  if (!x || !dy || !mean || !var || !gamma || !beta || !dgamma || !dbeta || !ws || M < 1 || bad_c(C))
    return CY_ERR_ARG;
  if (C % 4 == 0 && (misaligned(x) || misaligned(dy) || misaligned(mean) || misaligned(var) || misaligned(gamma) ||
                     misaligned(beta)))
    return CY_ERR_ARG;
  if (ws_bytes < cy_bn_rows_ws_bytes(M, C)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const BnGeom g = bn_geom(M, C);
  CY_BN_LAUNCH(bn_lrelu_bwd_reduce_kernel, g, st, x, dy, mean, var, gamma, beta, (double*)ws, M, C, g.ncv, g.lpr, eps,
               slope);
  hipLaunchKernelGGL(bn_lrelu_bwd_finalize_kernel, dim3(cy_cdiv(C, 256)), dim3(256), 0, st, (const double*)ws,
                     g.chunks, C, dgamma, dbeta);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_bn_lrelu_bwd_apply(const float* x, const float* dy, const float* mean, const float* var, const float* gamma,
                          const float* beta, const float* dgamma, const float* dbeta, float* dx, long M, int C,
                          float eps, float slope, int batch_stats, void* stream) {
  if (!x || !dy || !mean || !var || !gamma || !beta || !dx || M < 1 || bad_c(C)) return CY_ERR_ARG;
  if (batch_stats && (!dgamma || !dbeta || M < 2)) return CY_ERR_ARG;
  if (C % 4 == 0 && (misaligned(x) || misaligned(dy) || misaligned(dx) || misaligned(mean) || misaligned(var) ||
                     misaligned(gamma) || misaligned(beta) ||
                     (batch_stats && (misaligned(dgamma) || misaligned(dbeta)))))
    return CY_ERR_ARG;
  const BnGeom g = bn_geom(M, C);
  CY_BN_LAUNCH(bn_lrelu_bwd_apply_kernel, g, (hipStream_t)stream, x, dy, mean, var, gamma, beta, dgamma, dbeta, dx, M,
               C, g.ncv, g.lpr, eps, slope, batch_stats);
  return CY_OK;
}

int cy_leaky_relu_fwd(const float* x, float* y, long n, float slope, void* stream) {
  if (!x || !y || n <= 0) return CY_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const long nv = (misaligned(x) || misaligned(y)) ? 0 : n / 4;
  if (nv) {
    hipLaunchKernelGGL((leaky_relu_kernel<false, 4>), dim3(cy_blocks(nv, 256, FLAT_GRID_CAP)), dim3(256), 0, st, x,
                       (const float*)nullptr, y, 0L, nv, slope);
    CY_CHECK_LAUNCH();
  }
  if (n - 4 * nv) {
    hipLaunchKernelGGL((leaky_relu_kernel<false, 1>), dim3(cy_blocks(n - 4 * nv, 256, FLAT_GRID_CAP)), dim3(256), 0, st,
                       x, (const float*)nullptr, y, 4 * nv, n - 4 * nv, slope);
    CY_CHECK_LAUNCH();
  }
  return CY_OK;
}

int cy_leaky_relu_bwd(const float* x, const float* dy, float* dx, long n, float slope, void* stream) {
  if (!x || !dy || !dx || n <= 0) return CY_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const long nv = (misaligned(x) || misaligned(dy) || misaligned(dx)) ? 0 : n / 4;
  if (nv) {
    hipLaunchKernelGGL((leaky_relu_kernel<true, 4>), dim3(cy_blocks(nv, 256, FLAT_GRID_CAP)), dim3(256), 0, st, x, dy,
                       dx, 0L, nv, slope);
    CY_CHECK_LAUNCH();
  }
  if (n - 4 * nv) {
    hipLaunchKernelGGL((leaky_relu_kernel<true, 1>), dim3(cy_blocks(n - 4 * nv, 256, FLAT_GRID_CAP)), dim3(256), 0, st,
                       x, dy, dx, 4 * nv, n - 4 * nv, slope);
    CY_CHECK_LAUNCH();
  }
  return CY_OK;
}

size_t cy_sigmoid_bce_ws_bytes(long n) { return n < 1 ? 0 : (size_t)cy_blocks(n, 256, LOSS_GRID_CAP) * sizeof(double); }

int cy_sigmoid_bce_fwd(const float* scores, float label, float* loss, long n, void* ws, size_t ws_bytes,
                       void* stream) {
  if (!scores || !loss || !ws || n <= 0 || bad_label(label)) return CY_ERR_ARG;
  if (ws_bytes < cy_sigmoid_bce_ws_bytes(n)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = cy_blocks(n, 256, LOSS_GRID_CAP);
  hipLaunchKernelGGL(sigmoid_bce_fwd_kernel, dim3(nblk), dim3(256), 0, st, scores, (double*)ws, n,
                     label == 1.f ? 1 : 0);
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(mean_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, nblk, (double)n, loss);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_sigmoid_bce_bwd(const float* scores, float label, const float* gscale, float* dscores, long n, void* stream) {
  if (!scores || !gscale || !dscores || n <= 0 || bad_label(label)) return CY_ERR_ARG;
  hipLaunchKernelGGL(sigmoid_bce_bwd_kernel, dim3(cy_blocks(n, 256, FLAT_GRID_CAP)), dim3(256), 0, (hipStream_t)stream,
                     scores, gscale, dscores, n, label == 1.f ? 1 : 0);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

}  // extern "C"
