// Cross-correlation regulariser (semi_seg/hooks/ccblock.py:242-309, semi_seg/hooks/cc.py:108-142,
// contrastyou/losses/cross_correlation.py:10-74), f32:
//   edge map     d = mean_c sqrt((x - roll(x,1,H))^2 + (x - roll(x,1,W))^2), per-slice min/max normalisation, pow
//   entropy map  -sum_c p log(p + 1e-16), min/max normalisation per slice or over the batch, and its backward
//   CCLoss       -mean(cross^2 / (I_var * J_var)) over zero-padded k x k windows, and its backward
// Every reduction runs in a fixed order (per-workgroup partials, then one ordered sum; extrema are order-free):
// two runs give the same bits.  Nothing is kept between forward and backward but the inputs: the backward
// recomputes the five window sums on a tile with a halo of 2*(k/2) and box-sums the per-window derivatives.
#include "cy_common.h"
#include "cy_reduce.h"

#include <math.h>

namespace {

constexpr int CC_T = 32;         // output tile edge of the CCLoss kernels
constexpr int EXT_BLOCKS = 32;   // workgroups (= extrema partials) per slice of the map kernels
constexpr int CC_WIN_MIN = 3, CC_WIN_MAX = 15;
constexpr int ENT_KMAX = 128;
constexpr size_t LDS_LIMIT = 160 * 1024;

// min / max over a 256-thread workgroup, result in every thread
__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* sh /* [8] */) {
  mn = wave_min(mn);
  mx = wave_max(mx);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    sh[wave] = mn;
    sh[4 + wave] = mx;
  }
  __syncthreads();
  mn = fminf(fminf(sh[0], sh[1]), fminf(sh[2], sh[3]));
  mx = fmaxf(fmaxf(sh[4], sh[5]), fmaxf(sh[6], sh[7]));
}

// ---------------------------------------------------------------- edge strength, raw (ccblock.py:287-293)
// grid (EXT_BLOCKS, N).  VEC: C == 1 and W % 4 == 0, four pixels of a row per thread with 16-byte accesses.
template <bool VEC>
__global__ void __launch_bounds__(256)
    edge_raw_kernel(const float* __restrict__ img, float* __restrict__ out, float* __restrict__ partial, int H,
                    int W, int C) {
  __shared__ float sh[8];
  const int n = blockIdx.y;
  const long HW = (long)H * W;
  const float* x = img + (long)n * HW * C;
  float* o = out + (long)n * HW;
  float mn = INFINITY, mx = -INFINITY;
  if (VEC) {
    const long nq = HW / 4;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < nq; q += EXT_BLOCKS * 256L) {
      const long p = q * 4;
      const int h = (int)(p / W), w = (int)(p % W);
      const int hu = h == 0 ? H - 1 : h - 1;
      const f32x4 c = *reinterpret_cast<const f32x4*>(x + p);
      const f32x4 u = *reinterpret_cast<const f32x4*>(x + (long)hu * W + w);
      float left = x[(long)h * W + (w == 0 ? W - 1 : w - 1)];
      f32x4 d;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float dx = c[i] - u[i], dy = c[i] - left;
        d[i] = sqrtf(dx * dx + dy * dy);
        left = c[i];
        mn = fminf(mn, d[i]);
        mx = fmaxf(mx, d[i]);
      }
      *reinterpret_cast<f32x4*>(o + p) = d;
    }
  } else {
    const float invC = 1.f / (float)C;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < HW; p += EXT_BLOCKS * 256L) {
      const int h = (int)(p / W), w = (int)(p % W);
      const long pu = (long)(h == 0 ? H - 1 : h - 1) * W + w;
      const long pl = (long)h * W + (w == 0 ? W - 1 : w - 1);
      float s = 0.f;
      for (int c = 0; c < C; ++c) {
        const float v = x[p * C + c];
        const float dx = v - x[pu * C + c], dy = v - x[pl * C + c];
        s += sqrtf(dx * dx + dy * dy);
      }
      s *= invC;
      o[p] = s;
      mn = fminf(mn, s);
      mx = fmaxf(mx, s);
    }
  }
  block_minmax(mn, mx, sh);
  if (threadIdx.x == 0) {
    partial[((long)n * EXT_BLOCKS + blockIdx.x) * 2] = mn;
    partial[((long)n * EXT_BLOCKS + blockIdx.x) * 2 + 1] = mx;
  }
}

// ---------------------------------------------------------------- entropy, raw (losses/kl.py:31-55)
// grid (EXT_BLOCKS, N); p rows [N*HW][K]
__global__ void __launch_bounds__(256)
    entropy_raw_kernel(const float* __restrict__ p, float* __restrict__ out, float* __restrict__ partial, long HW,
                       int K, int vec) {
  __shared__ float sh[8];
  const int n = blockIdx.y;
  float mn = INFINITY, mx = -INFINITY;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < HW; i += EXT_BLOCKS * 256L) {
    const long pix = (long)n * HW + i;
    const float* row = p + pix * K;
    float e = 0.f;
    if (vec) {
      for (int c = 0; c < K; c += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) e -= v[j] * logf(v[j] + 1e-16f);
      }
    } else {
      for (int c = 0; c < K; ++c) {
        const float v = row[c];
        e -= v * logf(v + 1e-16f);
      }
    }
    out[pix] = e;
    mn = fminf(mn, e);
    mx = fmaxf(mx, e);
  }
  block_minmax(mn, mx, sh);
  if (threadIdx.x == 0) {
    partial[((long)n * EXT_BLOCKS + blockIdx.x) * 2] = mn;
    partial[((long)n * EXT_BLOCKS + blockIdx.x) * 2 + 1] = mx;
  }
}

// ---------------------------------------------------------------- (x - min) / (max - min + 1e-6), pow; in place
// grid (EXT_BLOCKS, N).  The extrema come from the raw kernel's partials: this slice's (slicewise) or all N slices'.
// mm (may be NULL) receives the {min, max} slice n was normalised with.
__global__ void __launch_bounds__(256)
    minmax_norm_kernel(float* __restrict__ map, const float* __restrict__ partial, float* __restrict__ mm, int N,
                       long HW, int slicewise, float power) {
  __shared__ float sh[8];
  const int n = blockIdx.y;
  const float* part = slicewise ? partial + (long)n * EXT_BLOCKS * 2 : partial;
  const int np = slicewise ? EXT_BLOCKS : N * EXT_BLOCKS;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < np; i += 256) {
    mn = fminf(mn, part[2 * i]);
    mx = fmaxf(mx, part[2 * i + 1]);
  }
  block_minmax(mn, mx, sh);
  if (mm && blockIdx.x == 0 && threadIdx.x == 0) {
    mm[2 * n] = mn;
    mm[2 * n + 1] = mx;
  }
  const float den = mx - mn + 1e-6f;
  float* m = map + (long)n * HW;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < HW; i += EXT_BLOCKS * 256L) {
    float v = (m[i] - mn) / den;
    if (power != 1.f) v = powf(v, power);
    m[i] = v;
  }
}

// dp = dmap / (max - min + 1e-6) * d(entropy)/dp; the extrema carry no gradient (min().detach(), ccblock.py:282)
__global__ void __launch_bounds__(256)
    entropy_bwd_kernel(const float* __restrict__ p, const float* __restrict__ mm, const float* __restrict__ dmap,
                       float* __restrict__ dp, long HW, long npix, int K, int vec) {
  for (long pix = blockIdx.x * 256L + threadIdx.x; pix < npix; pix += (long)gridDim.x * 256L) {
    const int n = (int)(pix / HW);
    const float g = dmap[pix] / (mm[2 * n + 1] - mm[2 * n] + 1e-6f);
    const float* row = p + pix * K;
    float* drow = dp + pix * K;
    if (vec) {
      for (int c = 0; c < K; c += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + c);
        f32x4 d;
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = -g * (logf(v[j] + 1e-16f) + v[j] / (v[j] + 1e-16f));
        *reinterpret_cast<f32x4*>(drow + c) = d;
      }
    } else {
      for (int c = 0; c < K; ++c) {
        const float v = row[c];
        drow[c] = -g * (logf(v + 1e-16f) + v / (v + 1e-16f));
      }
    }
  }
}

// ---------------------------------------------------------------- CCLoss
// One window: the reference's expressions (cross_correlation.py:63-72) on the five box sums.
struct CCWin {
  double cross, iv, jv, uI, uJ;
  bool mc, mi, mj;  // the clamp passed the raw value (gradient flows)
};
__device__ __forceinline__ CCWin cc_window(double sI, double sJ, double sI2, double sJ2, double sIJ, double n,
                                            double eps) {
  CCWin w;
  w.uI = sI / n;
  w.uJ = sJ / n;
  const double cross = sIJ - w.uJ * sI - w.uI * sJ + w.uI * w.uJ * n;
  const double iv = sI2 - 2.0 * w.uI * sI + w.uI * w.uI * n;
  const double jv = sJ2 - 2.0 * w.uJ * sJ + w.uJ * w.uJ * n;
  w.mc = cross > eps;
  w.mi = iv > eps;
  w.mj = jv > eps;
  w.cross = w.mc ? cross : eps;
  w.iv = w.mi ? iv : eps;
  w.jv = w.mj ? jv : eps;
  return w;
}

// load an E x E tile of a [H][W] map whose corner is (gy0, gx0) into LDS (pitch E + 1), zero outside the image
__device__ __forceinline__ void load_tile(const float* __restrict__ g, float* s, int E, int gy0, int gx0, int H, int W) {
  for (int i = threadIdx.x; i < E * E; i += 256) {
    const int ry = i / E, rx = i - ry * E;
    const int gy = gy0 + ry, gx = gx0 + rx;
    s[ry * (E + 1) + rx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? g[(long)gy * W + gx] : 0.f;
  }
}

// row pass: rs[q][row][x] = sum_dx of {I, J, I^2, J^2, IJ}[row][x + dx], rows of the E-tile, OW output columns.
// The sums are kept in f64: I_var = I2_sum - I_sum^2 / k^2 cancels, and on smooth maps an f32 sum's rounding
// (1e-7 of I2_sum) is not small against the variance that is left.
__device__ __forceinline__ void row_sums(const float* sI, const float* sJ, double* rs, int E, int OW, int win) {
  const int plane = E * OW;
  for (int i = threadIdx.x; i < plane; i += 256) {
    const int row = i / OW, x = i - row * OW;
    const float* a = sI + row * (E + 1) + x;
    const float* b = sJ + row * (E + 1) + x;
    double tI = 0.0, tJ = 0.0, tI2 = 0.0, tJ2 = 0.0, tIJ = 0.0;
    for (int d = 0; d < win; ++d) {
      const double vi = a[d], vj = b[d];
      tI += vi;
      tJ += vj;
      tI2 += vi * vi;
      tJ2 += vj * vj;
      tIJ += vi * vj;
    }
    rs[i] = tI;
    rs[plane + i] = tJ;
    rs[2 * plane + i] = tI2;
    rs[3 * plane + i] = tJ2;
    rs[4 * plane + i] = tIJ;
  }
}

// column pass of one window: the five k x k sums from the row sums (column x of rows y0 .. y0 + win - 1, pitch OW)
__device__ __forceinline__ CCWin window_at(const double* rs, int plane, int OW, int y0, int x, int win, double n,
                                           double eps) {
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int d = 0; d < win; ++d) {
    const int o = (y0 + d) * OW + x;
#pragma unroll
    for (int q = 0; q < 5; ++q) s[q] += rs[q * plane + o];
  }
  return cc_window(s[0], s[1], s[2], s[3], s[4], n, eps);
}

// forward: grid (tiles_x, tiles_y, N), CC_T x CC_T outputs per workgroup; partial[workgroup] = sum of cc over its windows
__global__ void __launch_bounds__(256)
    ccloss_fwd_kernel(const float* __restrict__ I, const float* __restrict__ J, double* __restrict__ partial, int H,
                      int W, int win, float eps) {
  extern __shared__ double lds[];
  constexpr int T = CC_T;
  const int r = win >> 1, E = T + 2 * r;
  const int plane = E * T;
  double* rs = lds;  // [5][E][T]; the workgroup sum's scratch afterwards
  float* sI = reinterpret_cast<float*>(rs + 5 * plane);
  float* sJ = sI + E * (E + 1);
  const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
  const long base = (long)blockIdx.z * H * W;
  load_tile(I + base, sI, E, y0 - r, x0 - r, H, W);
  load_tile(J + base, sJ, E, y0 - r, x0 - r, H, W);
  __syncthreads();
  row_sums(sI, sJ, rs, E, T, win);
  __syncthreads();
  const double n = (double)win * win;
  double acc = 0.0;
  for (int i = threadIdx.x; i < T * T; i += 256) {
    const int y = i / T, x = i - y * T;
    if (y0 + y < H && x0 + x < W) {
      const CCWin w = window_at(rs, plane, T, y, x, win, n, (double)eps);
      acc += w.cross * w.cross / (w.iv * w.jv);
    }
  }
  const double tot = block_sum_d(acc, rs);  // 5 * plane >= 256; its first barrier ends the reads of the row sums
  if (threadIdx.x == 0) partial[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tot;
}

__global__ void __launch_bounds__(256)
    ccloss_final_kernel(const double* __restrict__ partial, int nblk, double count, float* __restrict__ loss) {
  __shared__ double shd[256];
  const double tot = sum_partials_d(partial, nblk, 1, shd);
  if (threadIdx.x == 0) loss[0] = (float)(-tot / count);
}

// backward: grid (tiles_x, tiles_y, N).  With A, B, C = dL/d{I_sum, I2_sum, IJ_sum} per window,
//   dI(q) = box(A)(q) + 2 I(q) box(B)(q) + J(q) box(C)(q)        (the box filter is its own adjoint)
// and the same for J with (A_J, B_J, C).  Windows exist at the image's pixels only.
__global__ void __launch_bounds__(256)
    ccloss_bwd_kernel(const float* __restrict__ I, const float* __restrict__ J, const float* __restrict__ gscale,
                      float* __restrict__ dI, float* __restrict__ dJ, int H, int W, int win, float eps,
                      double inv_count, int T) {
  extern __shared__ double lds[];
  const int r = win >> 1, WE = T + 2 * r, E = T + 4 * r;
  double* rs = lds;                                         // [5][E][WE] window row sums
  float* sI = reinterpret_cast<float*>(rs + 5 * E * WE);
  float* sJ = sI + E * (E + 1);
  float* wm = sJ + E * (E + 1);                             // [5][WE][WE + 1]: A, B, C, A_J, B_J
  float* rw = reinterpret_cast<float*>(rs);                 // [5][WE][T] row sums of wm, once rs is consumed
  const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
  const long base = (long)blockIdx.z * H * W;
  const int nq = dJ ? 5 : 3;
  load_tile(I + base, sI, E, y0 - 2 * r, x0 - 2 * r, H, W);
  load_tile(J + base, sJ, E, y0 - 2 * r, x0 - 2 * r, H, W);
  __syncthreads();
  row_sums(sI, sJ, rs, E, WE, win);
  __syncthreads();
  {
    const double n = (double)win * win;
    const double g = -(double)gscale[0] * inv_count;
    const int wplane = WE * (WE + 1);
    for (int i = threadIdx.x; i < WE * WE; i += 256) {
      const int wy = i / WE, wx = i - wy * WE;
      const int gy = y0 - r + wy, gx = x0 - r + wx;
      float A = 0.f, B = 0.f, Cc = 0.f, AJ = 0.f, BJ = 0.f;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const CCWin w = window_at(rs, E * WE, WE, wy, wx, win, n, (double)eps);
        const double cc = w.cross * w.cross / (w.iv * w.jv);
        const double dcross = w.mc ? g * 2.0 * w.cross / (w.iv * w.jv) : 0.0;
        const double div = w.mi ? -g * cc / w.iv : 0.0;
        const double djv = w.mj ? -g * cc / w.jv : 0.0;
        A = (float)(-dcross * w.uJ - 2.0 * div * w.uI);
        B = (float)div;
        Cc = (float)dcross;
        AJ = (float)(-dcross * w.uI - 2.0 * djv * w.uJ);
        BJ = (float)djv;
      }
      const int o = wy * (WE + 1) + wx;
      wm[o] = A;
      wm[wplane + o] = B;
      wm[2 * wplane + o] = Cc;
      wm[3 * wplane + o] = AJ;
      wm[4 * wplane + o] = BJ;
    }
  }
  __syncthreads();
  {  // row pass over the window maps: rw[q][wy][x] = sum_dx wm[q][wy][x + dx]
    const int plane = WE * T, wplane = WE * (WE + 1);
    for (int i = threadIdx.x; i < plane; i += 256) {
      const int wy = i / T, x = i - wy * T;
      for (int q = 0; q < nq; ++q) {
        const float* a = wm + q * wplane + wy * (WE + 1) + x;
        float t = 0.f;
        for (int d = 0; d < win; ++d) t += a[d];
        rw[q * plane + i] = t;
      }
    }
  }
  __syncthreads();
  {
    const int plane = WE * T;
    for (int i = threadIdx.x; i < T * T; i += 256) {
      const int y = i / T, x = i - y * T;
      if (y0 + y >= H || x0 + x >= W) continue;
      float b[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
      for (int d = 0; d < win; ++d) {
        const int o = (y + d) * T + x;
        for (int q = 0; q < nq; ++q) b[q] += rw[q * plane + o];
      }
      const float vi = sI[(y + 2 * r) * (E + 1) + x + 2 * r], vj = sJ[(y + 2 * r) * (E + 1) + x + 2 * r];
      const long o = base + (long)(y0 + y) * W + x0 + x;
      if (dI) dI[o] = b[0] + 2.f * vi * b[1] + vj * b[2];
      if (dJ) dJ[o] = b[3] + 2.f * vj * b[4] + vi * b[2];
    }
  }
}

inline size_t ccloss_fwd_lds(int win, int T) {
  const size_t r = win / 2, E = T + 2 * r;
  return 5 * E * T * sizeof(double) + 2 * E * (E + 1) * sizeof(float);
}
inline size_t ccloss_bwd_lds(int win, int T) {
  const size_t r = win / 2, WE = T + 2 * r, E = T + 4 * r;
  return 5 * E * WE * sizeof(double) + (2 * E * (E + 1) + 5 * WE * (WE + 1)) * sizeof(float);
}
// the backward's tile: 32 x 32 outputs where its LDS image fits (windows up to 11), 16 x 16 for 13 and 15
constexpr size_t BWD_LDS_MAX = 150 * 1024;
inline int ccloss_bwd_tile(int win) { return ccloss_bwd_lds(win, CC_T) <= BWD_LDS_MAX ? CC_T : CC_T / 2; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool win_ok(int win) { return win >= CC_WIN_MIN && win <= CC_WIN_MAX && (win & 1); }
inline bool map_dims_ok(int N, int H, int W) {
  return N <= 65535 && cy_cdiv(H, CC_T / 2) <= 65535 && (long)H * W < (1L << 31);
}

}  // namespace

extern "C" {

size_t cy_cc_edge_map_ws_bytes(int N) { return N > 0 ? (size_t)N * EXT_BLOCKS * 2 * sizeof(float) : 0; }

int cy_cc_edge_map(const float* img, float* out, int N, int H, int W, int C, float power, void* ws, size_t ws_bytes,
                   void* stream) {
  if (!img || !out || !ws || N <= 0 || H <= 0 || W <= 0) return CY_ERR_ARG;
  if (C < 1 || C > 4 || !map_dims_ok(N, H, W) || !(power >= 0.f)) return CY_ERR_SHAPE;
  if (ws_bytes < cy_cc_edge_map_ws_bytes(N)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(EXT_BLOCKS, N);
  if (C == 1 && (W & 3) == 0 && aligned16(img) && aligned16(out))  // 16-byte accesses where the layout allows
    hipLaunchKernelGGL(edge_raw_kernel<true>, grid, dim3(256), 0, st, img, out, (float*)ws, H, W, C);
  else
    hipLaunchKernelGGL(edge_raw_kernel<false>, grid, dim3(256), 0, st, img, out, (float*)ws, H, W, C);
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(minmax_norm_kernel, grid, dim3(256), 0, st, out, (const float*)ws, (float*)nullptr, N,
                     (long)H * W, 1, power);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

size_t cy_entropy_map_ws_bytes(int N) { return N > 0 ? (size_t)N * EXT_BLOCKS * 2 * sizeof(float) : 0; }

int cy_entropy_map_fwd(const float* p, float* out, float* mm, int N, long HW, int K, int slicewise, void* ws,
                       size_t ws_bytes, void* stream) {
  if (!p || !out || !mm || !ws || N <= 0 || HW <= 0) return CY_ERR_ARG;
  if (K < 1 || K > ENT_KMAX || N > 65535) return CY_ERR_SHAPE;
  if (ws_bytes < cy_entropy_map_ws_bytes(N)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(EXT_BLOCKS, N);
  hipLaunchKernelGGL(entropy_raw_kernel, grid, dim3(256), 0, st, p, out, (float*)ws, HW, K,
                     (K & 3) == 0 && aligned16(p));
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(minmax_norm_kernel, grid, dim3(256), 0, st, out, (const float*)ws, mm, N, HW,
                     slicewise ? 1 : 0, 1.f);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_entropy_map_bwd(const float* p, const float* mm, const float* dmap, float* dp, int N, long HW, int K,
                       void* stream) {
  if (!p || !mm || !dmap || !dp || N <= 0 || HW <= 0) return CY_ERR_ARG;
  if (K < 1 || K > ENT_KMAX) return CY_ERR_SHAPE;
  const long npix = (long)N * HW;
  const int blocks = (int)((npix + 255) / 256 < 4096 ? (npix + 255) / 256 : 4096);
  hipLaunchKernelGGL(entropy_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, mm, dmap, dp, HW, npix,
                     K, (K & 3) == 0 && aligned16(p) && aligned16(dp));
  CY_CHECK_LAUNCH();
  return CY_OK;
}

size_t cy_ccloss_ws_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)N * cy_cdiv(H, CC_T) * cy_cdiv(W, CC_T) * sizeof(double);
}

int cy_ccloss_fwd(const float* I, const float* J, float* loss, int N, int H, int W, int win, float eps, void* ws,
                  size_t ws_bytes, void* stream) {
  if (!I || !J || !loss || !ws || N <= 0 || H <= 0 || W <= 0) return CY_ERR_ARG;
  if (!win_ok(win) || !map_dims_ok(N, H, W) || ccloss_fwd_lds(win, CC_T) > LDS_LIMIT) return CY_ERR_SHAPE;
  if (ws_bytes < cy_ccloss_ws_bytes(N, H, W)) return CY_ERR_WORKSPACE;
  // set on every call (a host-side table write): no once-per-process flag to get wrong across threads or devices
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(ccloss_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)ccloss_fwd_lds(CC_WIN_MAX, CC_T)) != hipSuccess)
    return CY_ERR_LAUNCH;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(cy_cdiv(W, CC_T), cy_cdiv(H, CC_T), N);
  const long nblk = (long)grid.x * grid.y * grid.z;
  if (nblk >= (1L << 31)) return CY_ERR_SHAPE;
  hipLaunchKernelGGL(ccloss_fwd_kernel, grid, dim3(256), ccloss_fwd_lds(win, CC_T), st, I, J, (double*)ws, H, W, win,
                     eps);
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(ccloss_final_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, (int)nblk,
                     (double)N * H * W, loss);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_ccloss_bwd(const float* I, const float* J, const float* gscale, float* dI, float* dJ, int N, int H, int W,
                  int win, float eps, void* stream) {
  if (!I || !J || !gscale || (!dI && !dJ) || N <= 0 || H <= 0 || W <= 0) return CY_ERR_ARG;
  if (!win_ok(win) || !map_dims_ok(N, H, W)) return CY_ERR_SHAPE;
  const int T = ccloss_bwd_tile(win);
  const size_t lds = ccloss_bwd_lds(win, T);
  if (lds > LDS_LIMIT) return CY_ERR_SHAPE;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(ccloss_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)BWD_LDS_MAX) != hipSuccess)
    return CY_ERR_LAUNCH;
  const dim3 grid(cy_cdiv(W, T), cy_cdiv(H, T), N);
  hipLaunchKernelGGL(ccloss_bwd_kernel, grid, dim3(256), lds, (hipStream_t)stream, I, J, gscale, dI, dJ, H, W, win,
                     eps, 1.0 / ((double)N * H * W), T);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

}  // extern "C"
