// Discrete mutual-information losses over cluster-probability maps.
//   DenseClusterHead / ClusterHead softmax(T)     contrastyou/projectors/heads.py:44-78,125-173,
//                                                 contrastyou/projectors/nn.py:35-44
//   compute_joint (vectors)                       contrastyou/losses/discreteMI.py:201-222
//   compute_joint_2D (displaced, padding > 0)     contrastyou/losses/discreteMI.py:225-243
//   compute_joint_2D_with_padding_zeros           contrastyou/losses/discreteMI.py:246-261
//   IIDLoss / IIDSegmentationLoss                 contrastyou/losses/discreteMI.py:90-170
//   IIDSegmentationSmallPathLoss, patch_generator contrastyou/losses/discreteMI.py:173-198,264-272
//
// The k x k joint of two [pixels][k] probability maps is a skinny contraction over N*H*W pixels
// (k = 20): HBM-bound, 2*k*4 bytes read per pixel, k*k FMAs.  It is NOT reshaped into an MFMA
// GEMM: each thread keeps a 4x4 register tile of the joint and walks a slice of the pixels of an
// LDS-staged tile; block partials are reduced in a fixed order (deterministic).
// Layouts: probability maps are NHWC f32 [N][H][W][k]; joints are [T*T][k][k], T = 2*padding+1.
#include "cy_common.h"
#include "cy_reduce.h"

namespace {

constexpr int J_P = 64;      // pixels per staged tile
constexpr int J_KMAX = 64;   // max clusters

constexpr int GRID_CAP = 8192;  // blocks of 256 of the elementwise backward kernels; the rest is grid-stride

// ---------------------------------------------------------------- grouped softmax
// in  [M][S*k] logits  ->  out [S][M][k] probabilities of softmax(logits * invT) per group.
// A block owns GS_PB consecutive rows: the [GS_PB][S*k] logit tile is one contiguous span of
// memory and each [GS_PB][k] output tile is another, so all global traffic is coalesced; the
// (row, group) -> thread transposition happens in LDS (row pitch S*k+1: conflict-free).
constexpr int GS_PB = 64;

__global__ void __launch_bounds__(256)
    group_softmax_fwd_kernel(const float* __restrict__ in, float* __restrict__ out, long M, int S,
                             int k, float invT) {
  extern __shared__ float tile[];  // [GS_PB][S*k + 1]
  const int SK = S * k, pitch = SK + 1;
  const long m0 = (long)blockIdx.x * GS_PB;
  const int rows = (int)min((long)GS_PB, M - m0);
  const float* src = in + m0 * SK;
  for (int e = threadIdx.x; e < rows * SK; e += 256) tile[(e / SK) * pitch + e % SK] = src[e] * invT;
  __syncthreads();
  for (int e = threadIdx.x; e < rows * S; e += 256) {
    float* v = tile + (e % rows) * pitch + (e / rows) * k;
    float mx = -INFINITY;
    for (int i = 0; i < k; ++i) mx = fmaxf(mx, v[i]);
    float sum = 0.f;
    for (int i = 0; i < k; ++i) {
      v[i] = __expf(v[i] - mx);
      sum += v[i];
    }
    const float r = 1.f / sum;
    for (int i = 0; i < k; ++i) v[i] *= r;
  }
  __syncthreads();
  for (int s = 0; s < S; ++s) {
    float* dst = out + ((long)s * M + m0) * k;
    for (int e = threadIdx.x; e < rows * k; e += 256) dst[e] = tile[(e / k) * pitch + s * k + e % k];
  }
}

// dlogits[m][s*k+i] = invT * p_i * (dp_i - sum_j p_j dp_j)
__global__ void __launch_bounds__(256)
    group_softmax_bwd_kernel(const float* __restrict__ p, const float* __restrict__ dp,
                             float* __restrict__ dlogits, long M, int S, int k, float invT, int PB) {
  extern __shared__ float tile[];  // p then dp: 2 x [PB][S*k + 1]; PB = GS_PB, or GS_PB / 2 where two such tiles
                                   // exceed 64 KB (S*k > 127)
  const int SK = S * k, pitch = SK + 1;
  float* tp = tile;
  float* td = tile + PB * pitch;
  const long m0 = (long)blockIdx.x * PB;
  const int rows = (int)min((long)PB, M - m0);
  for (int s = 0; s < S; ++s) {
    const float* sp = p + ((long)s * M + m0) * k;
    const float* sd = dp + ((long)s * M + m0) * k;
    for (int e = threadIdx.x; e < rows * k; e += 256) {
      tp[(e / k) * pitch + s * k + e % k] = sp[e];
      td[(e / k) * pitch + s * k + e % k] = sd[e];
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < rows * S; e += 256) {
    const int off = (e % rows) * pitch + (e / rows) * k;
    float dot = 0.f;
    for (int i = 0; i < k; ++i) dot = fmaf(tp[off + i], td[off + i], dot);
    for (int i = 0; i < k; ++i) td[off + i] = invT * tp[off + i] * (td[off + i] - dot);
  }
  __syncthreads();
  float* dst = dlogits + m0 * SK;
  for (int e = threadIdx.x; e < rows * SK; e += 256) dst[e] = td[(e / SK) * pitch + e % SK];
}

// ---------------------------------------------------------------- joint forward
// Both forward forms work on a WINDOW of the maps, origin (h0, w0) and extent eh x ew, and are written once, as a body:
//   J[q][d][i][j] = sum_n sum_{(h,w) in q, (h+du,w+dv) in q} x1[n][h+du][w+dv][i] * x2[n][h][w][j]
// A displaced read that leaves the window is zero.  The whole image is the window {0, 0, H, W} with q = 0
// (joint_fwd_kernel, joint_fwd_multi_kernel); the patches of the patch-wise loss are P windows of one extent, q the
// patch (joint_patch_fwd1_kernel, joint_patch_fwd_kernel further down).  A block's sums go to
// part[q][d][blockIdx.x][k*k]; where the caller gives J (its one block along x holds the whole sum) they go straight to
// J[q][d][k*k], times scale and rounded as joint_reduce_kernel rounds.
struct joint_window {
  int h0, w0, eh, ew;
};

// thread -> (pixel slice sl of nsl, 4x4 tile (ti, tj) of the kp x kp joint); threads past the last slice idle
struct joint_lanes {
  int kp, nsl, sl, ti, tj;
  bool active;
};
__device__ __forceinline__ joint_lanes joint_lanes_of(int k) {
  joint_lanes L;
  L.kp = (k + 3) & ~3;
  const int k4 = L.kp >> 2, tps = k4 * k4;  // threads per pixel slice
  L.nsl = 256 / tps;                        // slices (>= 1 because k <= 64)
  L.sl = (int)threadIdx.x / tps;
  const int tt = (int)threadIdx.x - L.sl * tps;
  L.ti = tt / k4;
  L.tj = tt - L.ti * k4;
  L.active = L.sl < L.nsl;
  return L;
}

// One joint of the block leaves the registers: the slices meet in red[nsl][kp*kp] and are summed in slice order.
__device__ __forceinline__ void joint_write_out(const float (&acc)[4][4], float* red, const joint_lanes& L,
                                                float* __restrict__ part, float* __restrict__ J, double scale,
                                                size_t qd, int k) {
  const int kp = L.kp;
  __syncthreads();
  if (L.active) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[L.sl * kp * kp + (4 * L.ti + i) * kp + 4 * L.tj + j] = acc[i][j];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < k * k; e += 256) {
    const int i = e / k, j = e - i * k;
    float s = 0.f;
    for (int u = 0; u < L.nsl; ++u) s += red[u * kp * kp + i * kp + j];
    if (J)
      J[qd * (k * k) + e] = (float)((double)s * scale);
    else
      part[(qd * gridDim.x + blockIdx.x) * (k * k) + e] = s;
  }
}

// The per-displacement form: one displacement per block (blockIdx.y), 64-pixel tiles of the window's N*eh*ew pixels
// split evenly over gridDim.x, the displaced read bounds-tested against the window.
// WHOLE: the window is the whole map, so a tile is one contiguous span of both maps and, with pad == 0 and k % 4 == 0
// (the padding-0 segmentation joint), is staged in 16-byte copies.
template <bool WHOLE>
__device__ __forceinline__ void joint_tile_body(const float* __restrict__ x1, const float* __restrict__ x2,
                                                float* __restrict__ part, float* __restrict__ J, double scale, int N,
                                                int H, int W, int k, int pad, const joint_window win, int q) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const joint_lanes L = joint_lanes_of(k);
  const int kp = L.kp;
  float* xs1 = sm;                 // [J_P][kp]
  float* xs2 = sm + J_P * kp;      // [J_P][kp]
  float* red = sm + 2 * J_P * kp;  // [nsl][kp*kp]
  const int tid = threadIdx.x;
  const int T = 2 * pad + 1;
  const int du = (int)blockIdx.y / T - pad, dv = (int)blockIdx.y % T - pad;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  const long npix = (long)N * win.eh * win.ew;
  const long per = ((npix + gridDim.x - 1) / gridDim.x + J_P - 1) / J_P * J_P;
  const long p0 = (long)blockIdx.x * per;
  const long p1 = p0 + per < npix ? p0 + per : npix;
  for (long pt = p0; pt < p1; pt += J_P) {
    __syncthreads();
    if (WHOLE && pad == 0 && kp == k) {
      const long lim = (p1 - pt) * k;  // floats of this tile that exist
      for (int e4 = tid; e4 < J_P * k / 4; e4 += 256) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if (4L * e4 < lim) {
          a = *reinterpret_cast<const f32x4*>(x1 + pt * k + 4 * e4);
          b = *reinterpret_cast<const f32x4*>(x2 + pt * k + 4 * e4);
        }
        *reinterpret_cast<f32x4*>(xs1 + 4 * e4) = a;
        *reinterpret_cast<f32x4*>(xs2 + 4 * e4) = b;
      }
    } else {
      for (int e = tid; e < J_P * kp; e += 256) {
        const int p = e / kp, c = e - p * kp;
        const long pp = pt + p;
        float a = 0.f, b = 0.f;
        if (pp < p1 && c < k) {
          const int wl = (int)(pp % win.ew);
          const long t = pp / win.ew;
          const int hl = (int)(t % win.eh);
          const long n = t / win.eh;
          b = x2[((n * H + win.h0 + hl) * W + win.w0 + wl) * k + c];
          const int hh = hl + du, ww = wl + dv;
          if (hh >= 0 && hh < win.eh && ww >= 0 && ww < win.ew)
            a = x1[((n * H + win.h0 + hh) * W + win.w0 + ww) * k + c];
        }
        xs1[e] = a;
        xs2[e] = b;
      }
    }
    __syncthreads();
    if (L.active) {
      for (int p = L.sl; p < J_P; p += L.nsl) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(xs1 + p * kp + 4 * L.ti);
        const f32x4 b = *reinterpret_cast<const f32x4*>(xs2 + p * kp + 4 * L.tj);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
      }
    }
  }
  joint_write_out(acc, red, L, part, J, scale, (size_t)q * T * T + blockIdx.y, k);
}

// part[blockIdx.y = displacement][blockIdx.x][k*k]
__global__ void __launch_bounds__(256)
    joint_fwd_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                     float* __restrict__ part, int N, int H, int W, int k, int pad) {
  joint_tile_body<true>(x1, x2, part, nullptr, 1.0, N, H, W, k, pad, joint_window{0, 0, H, W}, 0);
}

// The staged form, displaced joints (padding > 0) in ONE pass over the maps: the form above runs per displacement and
// reads both maps (2p+1)^2 times (9 displacements: 266 GB/s of algorithmic traffic).  Here a block owns a group of up to
// JM_D = 9 displacements (blockIdx.y) and walks the (image, tile of R window rows) pairs with stride gridDim.x.  It
// stages the R rows of x2 and the R + 2p rows of x1 around them, with p zero columns on both sides and rows outside the
// window zero (so a displaced read is an address shift, no bounds test), and every thread keeps one 4x4 tile of the
// joint per displacement: up to 144 accumulators.  The reduction buffer lies over the tiles once they are done (72 KB at
// W = 224, k = 20: two workgroups per CU, one stages while the other computes).
// SPAN: the window is as wide as the map, so its R rows of x2 are one span of memory as they are of the staged tile.
constexpr int JM_D = 9;

template <bool SPAN>
__device__ __forceinline__ void joint_staged_body(const float* __restrict__ x1, const float* __restrict__ x2,
                                                  float* __restrict__ part, float* __restrict__ J, double scale, int N,
                                                  int H, int W, int k, int pad, int R, const joint_window win, int q) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const joint_lanes L = joint_lanes_of(k);
  const int kp = L.kp, nsl = L.nsl;
  const int h0 = win.h0, w0 = win.w0, eh = win.eh, ew = win.ew;
  const int Wp = ew + 2 * pad, Rp = R + 2 * pad;
  float* xs1 = sm;                          // [Rp][Wp][kp]
  float* xs2 = xs1 + (size_t)Rp * Wp * kp;  // [R][ew][kp]
  float* red = sm;                          // [nsl][kp*kp]
  const int tid = threadIdx.x;
  const int T = 2 * pad + 1, TT = T * T;
  const int d0 = (int)blockIdx.y * JM_D;
  const int nd = TT - d0 < JM_D ? TT - d0 : JM_D;
  float acc[JM_D][4][4];
#pragma unroll
  for (int d = 0; d < JM_D; ++d)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[d][a][b] = 0.f;
  int doff[JM_D];  // LDS offset (floats) of displacement d relative to the undisplaced pixel
#pragma unroll
  for (int d = 0; d < JM_D; ++d) {
    const int dd = d0 + (d < nd ? d : 0);
    doff[d] = ((dd / T - pad) * Wp + (dd % T - pad)) * kp;
  }
  const int tiles_h = (eh + R - 1) / R;
  const int ntile = N * tiles_h;
  if (kp == k)  // the zero columns left and right of every staged x1 row
    for (int e = tid; e < Rp * 2 * pad * kp; e += 256) {
      const int r = e / (2 * pad * kp), c = e - r * (2 * pad * kp);
      const int col = c / kp < pad ? c / kp : ew + c / kp;  // 0..pad-1 | ew+pad..ew+2pad-1
      xs1[(r * Wp + col) * kp + c % kp] = 0.f;
    }
  for (int t = blockIdx.x; t < ntile; t += gridDim.x) {
    const int n = t / tiles_h, r0 = (t - n * tiles_h) * R;
    const int rows = eh - r0 < R ? eh - r0 : R;
    __syncthreads();
    if (kp == k) {
      // a window row is one contiguous, 16-byte aligned span of ew*k floats in memory and in the staged tile: 16-byte
      // copies (the pad columns were zeroed once, rows outside the window are zeroed here)
      const int row4 = ew * k / 4;
      for (int r = 0; r < Rp; ++r) {
        const int pr = r0 - pad + r;
        const bool ok = r < rows + 2 * pad && pr >= 0 && pr < eh;
        const float* src = x1 + (((long)n * H + h0 + (ok ? pr : 0)) * W + w0) * k;
        float* dst = xs1 + (r * Wp + pad) * kp;
        for (int e4 = tid; e4 < row4; e4 += 256) {
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
          if (ok) v = *reinterpret_cast<const f32x4*>(src + 4 * e4);
          *reinterpret_cast<f32x4*>(dst + 4 * e4) = v;
        }
      }
      const float* src2 = x2 + (((long)n * H + h0 + r0) * W + w0) * k;  // the tile's first row of x2
      for (int e4 = tid; e4 < R * row4; e4 += 256) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (SPAN) {  // the rows follow each other in memory as they do in the tile
          if (e4 < rows * row4) v = *reinterpret_cast<const f32x4*>(src2 + 4 * e4);
        } else {
          const int r = e4 / row4, c4 = e4 - r * row4;
          if (r < rows) v = *reinterpret_cast<const f32x4*>(src2 + (long)r * W * k + 4 * c4);
        }
        *reinterpret_cast<f32x4*>(xs2 + 4 * e4) = v;
      }
    } else {
      for (int e = tid; e < Rp * Wp * kp; e += 256) {
        const int c = e % kp;
        const int p = e / kp;
        const int cw = p % Wp, r = p / Wp;
        const int pr = r0 - pad + r, pc = cw - pad;
        float v = 0.f;
        if (c < k && r < rows + 2 * pad && pr >= 0 && pr < eh && pc >= 0 && pc < ew)
          v = x1[(((long)n * H + h0 + pr) * W + w0 + pc) * k + c];
        xs1[e] = v;
      }
      for (int e = tid; e < R * ew * kp; e += 256) {
        const int c = e % kp;
        const int p = e / kp;
        const int w = p % ew, r = p / ew;
        xs2[e] = (c < k && r < rows) ? x2[(((long)n * H + h0 + r0 + r) * W + w0 + w) * k + c] : 0.f;
      }
    }
    __syncthreads();
    if (L.active) {
      int r = 0, w = L.sl;
      while (w >= ew) w -= ew, ++r;
      for (; r < rows;) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(xs2 + (r * ew + w) * kp + 4 * L.tj);
        const float* a0 = xs1 + ((r + pad) * Wp + (w + pad)) * kp + 4 * L.ti;
#pragma unroll
        for (int d = 0; d < JM_D; ++d) {
          if (d < nd) {  // wave-uniform
            const f32x4 a = *reinterpret_cast<const f32x4*>(a0 + doff[d]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[d][i][j] = fmaf(a[i], b[j], acc[d][i][j]);
          }
        }
        w += nsl;
        while (w >= ew) w -= ew, ++r;
      }
    }
  }
#pragma unroll
  for (int d = 0; d < JM_D; ++d) {  // (no early exit: the accumulators must stay statically indexed = in registers)
    if (d >= nd) continue;          // block-uniform
    joint_write_out(acc[d], red, L, part, J, scale, (size_t)q * TT + d0 + d, k);
  }
}

// part[displacement][blockIdx.x][k*k]
__global__ void __launch_bounds__(256, 2)
    joint_fwd_multi_kernel(const float* __restrict__ x1, const float* __restrict__ x2, float* __restrict__ part,
                           int N, int H, int W, int k, int pad, int R) {
  joint_staged_body<true>(x1, x2, part, nullptr, 1.0, N, H, W, k, pad, R, joint_window{0, 0, H, W}, 0);
}


// J[e] = scale * sum_b part[d][b][r]: 4 elements per block, 64 slices of the block partials each,
// fixed slice order (deterministic)
__global__ void __launch_bounds__(256)
    joint_reduce_kernel(const float* __restrict__ part, float* __restrict__ J, int TT, int nblk,
                        int kk, double scale) {
  __shared__ double sred[64][4];
  const int el = threadIdx.x & 3, sl = threadIdx.x >> 2;
  const int e = blockIdx.x * 4 + el;
  double s = 0.0;
  if (e < TT * kk) {
    const int d = e / kk, r = e - d * kk;
    for (int b = sl; b < nblk; b += 64) s += (double)part[((size_t)d * nblk + b) * kk + r];
  }
  sred[sl][el] = s;
  __syncthreads();
  if (sl == 0 && e < TT * kk) {
    double t = 0.0;
    for (int q = 0; q < 64; ++q) t += sred[q][el];
    J[e] = (float)(t * scale);
  }
}

// ---------------------------------------------------------------- joint backward
// which = 0: dx1[pix][i] = g*scale * sum_{d,j} dJ[d][i][j] * x2[pix - disp(d)][j]
// which = 1: dx2[pix][j] = g*scale * sum_{d,i} dJ[d][i][j] * x1[pix + disp(d)][i]
// dJ is staged in LDS dchunk displacements at a time (the launch plan: as many as fit 64 KB).  With one chunk, which is
// every padding-0 launch and padding 1 up to k = 42, it is staged once per block; otherwise once per chunk and trip of
// the grid-stride loop, whose trip count is the same for every thread of a block (the barriers are block-uniform).

// The product both adjoints (this one and the patch-wise gather) are made of, for one displacement: m = its k x k dJ,
// o = the other map's pixel, c = the thread's first output channel.
//   which = 0: s[u] += sum_j m[c+u][j] * o[j]      which = 1: s[u] += sum_i m[i][c+u] * o[i]
// V = 4 (k % 4 == 0): 16-byte reads of m and o; V = 1: scalar.  s: the thread's V sums.
template <int V>
__device__ __forceinline__ void joint_bwd_dot(float* s, const float* m, const float* o, int k, int c, int which) {
  if (V == 4) {
    for (int j4 = 0; j4 < k / 4; ++j4) {
      const f32x4 ov = *reinterpret_cast<const f32x4*>(o + 4 * j4);
      if (which) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const f32x4 mv = *reinterpret_cast<const f32x4*>(m + (4 * j4 + t) * k + c);
#pragma unroll
          for (int u = 0; u < V; ++u) s[u] = fmaf(mv[u], ov[t], s[u]);
        }
      } else {
#pragma unroll
        for (int u = 0; u < V; ++u) {
          const f32x4 mv = *reinterpret_cast<const f32x4*>(m + (c + u) * k + 4 * j4);
#pragma unroll
          for (int t = 0; t < 4; ++t) s[u] = fmaf(mv[t], ov[t], s[u]);
        }
      }
    }
  } else if (which) {
    for (int i = 0; i < k; ++i) s[0] = fmaf(m[i * k + c], o[i], s[0]);
  } else {
    for (int j = 0; j < k; ++j) s[0] = fmaf(m[c * k + j], o[j], s[0]);
  }
}

// dx[pix][c..c+V) = g * s, as one 16-byte store for V = 4
template <int V>
__device__ __forceinline__ void joint_bwd_store(float* __restrict__ dx, long at, const float (&s)[V], float g) {
  if (V == 4) {
    f32x4 r = {g * s[0], g * s[V > 1 ? 1 : 0], g * s[V > 2 ? 2 : 0], g * s[V > 3 ? 3 : 0]};
    *reinterpret_cast<f32x4*>(dx + at) = r;
  } else {
    dx[at] = g * s[0];
  }
}

template <int V>  // V = 4: one thread per (pixel, 4 channels), k % 4 == 0; V = 1: one thread per (pixel, channel)
__global__ void __launch_bounds__(256)
    joint_bwd_kernel(const float* __restrict__ other, const float* __restrict__ dJ,
                     const float* __restrict__ gscale, float* __restrict__ dx, int N, int H, int W,
                     int k, int pad, float scale, int which, int dchunk) {
  extern __shared__ __attribute__((aligned(16))) float sdj[];  // [min(dchunk, T*T)][k][k]
  const int T = 2 * pad + 1, TT = T * T, kv = k / V, kk = k * k;
  const bool once = dchunk >= TT;
  if (once) {
    for (int e = threadIdx.x; e < TT * kk; e += 256) sdj[e] = dJ[e];
    __syncthreads();
  }
  const float g = gscale[0] * scale;
  const long total = (long)N * H * W * kv;
  for (long base = blockIdx.x * 256L; base < total; base += (long)gridDim.x * 256L) {
    const long e = base + threadIdx.x;
    const bool live = e < total;
    const int c = (int)(e % kv) * V;
    const long pix = e / kv;
    const int w = (int)(pix % W);
    const int h = (int)((pix / W) % H);
    float s[V];
#pragma unroll
    for (int u = 0; u < V; ++u) s[u] = 0.f;
    for (int d0 = 0; d0 < TT; d0 += dchunk) {
      const int d1 = d0 + dchunk < TT ? d0 + dchunk : TT;
      if (!once) {
        __syncthreads();
        for (int q = threadIdx.x; q < (d1 - d0) * kk; q += 256) sdj[q] = dJ[(size_t)d0 * kk + q];
        __syncthreads();
      }
      if (!live) continue;
      for (int d = d0; d < d1; ++d) {
        const int du = d / T - pad, dv = d % T - pad;
        const int hh = which ? h + du : h - du, ww = which ? w + dv : w - dv;
        if (hh < 0 || hh >= H || ww < 0 || ww >= W) continue;
        const long q = which ? pix + (long)du * W + dv : pix - (long)du * W - dv;
        joint_bwd_dot<V>(s, sdj + (d - d0) * kk, other + q * k, k, c, which);
      }
    }
    if (live) joint_bwd_store<V>(dx, pix * k + c, s, g);
  }
}

// ---------------------------------------------------------------- loss on the joint (one block)
// mode 0: segmentation, padding 0 (no normalisation)      mode 1: segmentation, padding > 0
// mode 2: vectors (IIDLoss): symmetrise + normalise to 1
// ws: 4 arrays of TT*kk floats (p1, p2/p, dP, tmp) + (2*TT*k) marginals
// out[0] = loss, out[1] = loss with lambda = 1 (mode 2 only); P = final joint; dJ = dloss/dJ.
// The body is shared by iid_loss_kernel (one joint) and iid_patch_loss_kernel (one block per patch): out0 / out1 (may be
// NULL) take the two loss values, dJ is multiplied by gmul (1 for the single joint, which leaves its bits as they were;
// 1/P for the patch-wise mean).
__device__ __forceinline__ void iid_loss_body(const float* __restrict__ J, float* __restrict__ out0,
                                              float* __restrict__ out1, float* __restrict__ P,
                                              float* __restrict__ dJ, float* __restrict__ ws, int TT, int k, int mode,
                                              int symmetric, float lamda, float eps, double gmul, double* sred) {
  const int tid = threadIdx.x;
  const int kk = k * k, n = TT * kk;
  float* p1 = ws;            // per-displacement normalised (mode 1) / raw
  float* p = ws + n;         // final joint
  float* dP = ws + 2 * n;    // dloss/dp, then dloss/dp2
  float* row = ws + 4 * n;   // r_i  [TT][k]
  float* col = row + TT * k; // c_j  [TT][k]
  float* S = col + TT * k;   // [TT] displacement sums (mode 1)

  // ---- forward normalisations
  double Z = 1.0;
  if (mode == 1) {
    double mn = 1e300;
    for (int e = tid; e < n; e += 256) mn = fmin(mn, (double)J[e]);
    mn = block_min_d(mn, sred);
    for (int d = 0; d < TT; ++d) {
      double s = 0.0;
      for (int e = tid; e < kk; e += 256) s += (double)J[d * kk + e] - mn + 1e-8;
      s = block_sum_d(s, sred);
      if (tid == 0) S[d] = (float)s;
      for (int e = tid; e < kk; e += 256) p1[d * kk + e] = (float)(((double)J[d * kk + e] - mn + 1e-8) / s);
    }
  } else {
    for (int e = tid; e < n; e += 256) p1[e] = J[e];
  }
  __syncthreads();
  {  // symmetrise into p (unnormalised), then global normalisation for modes 1, 2
    double z = 0.0;
    for (int e = tid; e < n; e += 256) {
      const int d = e / kk, r = e - d * kk, i = r / k, j = r - i * k;
      float v = p1[e];
      if (symmetric) v = 0.5f * (v + p1[d * kk + j * k + i]);
      p[e] = v;
      z += (double)v;
    }
    if (mode != 0) {
      Z = block_sum_d(z, sred);
      for (int e = tid; e < n; e += 256) p[e] = (float)((double)p[e] / Z);
    }
  }
  __syncthreads();
  // ---- marginals per displacement
  for (int e = tid; e < TT * k; e += 256) {
    const int d = e / k, a = e - d * k;
    double r = 0.0, c = 0.0;
    for (int b = 0; b < k; ++b) {
      r += (double)p[d * kk + a * k + b];
      c += (double)p[d * kk + b * k + a];
    }
    row[e] = (float)r;
    col[e] = (float)c;
  }
  __syncthreads();
  // ---- loss and dloss/dp
  const double invTT = mode == 1 ? 1.0 / (double)TT : 1.0;
  double l = 0.0, l1 = 0.0;
  for (int e = tid; e < n; e += 256) {
    const int d = e / kk, r = e - d * kk, a = r / k, b = r - a * k;
    const double pv = p[e], ra = row[d * k + a], cb = col[d * k + b];
    const double lp = log(pv + eps), lr = log(ra + eps), lc = log(cb + eps);
    l += -pv * (lp - lamda * lc - lamda * lr);
    l1 += -pv * (lp - lc - lr);
    const double g = -(lp - lamda * lc - lamda * lr) - pv / (pv + eps) + lamda * cb / (cb + eps) +
                     lamda * ra / (ra + eps);
    dP[e] = (float)(g * invTT);
    if (P) P[e] = (float)pv;
  }
  l = block_sum_d(l, sred);
  l1 = block_sum_d(l1, sred);
  if (tid == 0) {
    out0[0] = (float)(l * invTT);
    if (out1) out1[0] = (float)(l1 * invTT);
  }
  if (!dJ) return;
  // ---- backward through the normalisations
  if (mode != 0) {  // p = p2 / Z
    double dot = 0.0;
    for (int e = tid; e < n; e += 256) dot += (double)dP[e] * (double)p[e];
    dot = block_sum_d(dot, sred);
    for (int e = tid; e < n; e += 256) dP[e] = (float)(((double)dP[e] - dot) / Z);
  }
  __syncthreads();
  float* dp1 = ws + 3 * n;
  for (int e = tid; e < n; e += 256) {
    const int d = e / kk, r = e - d * kk, i = r / k, j = r - i * k;
    dp1[e] = symmetric ? 0.5f * (dP[e] + dP[d * kk + j * k + i]) : dP[e];
  }
  __syncthreads();
  if (mode == 1) {
    for (int d = 0; d < TT; ++d) {
      double dot = 0.0;
      for (int e = tid; e < kk; e += 256) dot += (double)dp1[d * kk + e] * (double)p1[d * kk + e];
      dot = block_sum_d(dot, sred);
      const double s = S[d];
      for (int e = tid; e < kk; e += 256) dJ[d * kk + e] = (float)((((double)dp1[d * kk + e] - dot) / s) * gmul);
    }
  } else {
    for (int e = tid; e < n; e += 256) dJ[e] = (float)((double)dp1[e] * gmul);
  }
}

__global__ void __launch_bounds__(256)
    iid_loss_kernel(const float* __restrict__ J, float* __restrict__ out, float* __restrict__ P,
                    float* __restrict__ dJ, float* __restrict__ ws, int TT, int k, int mode,
                    int symmetric, float lamda, float eps) {
  __shared__ double sred[256];
  iid_loss_body(J, out, out + 1, P, dJ, ws, TT, k, mode, symmetric, lamda, eps, 1.0, sred);
}

constexpr int JOINT_PIX = 1024;       // pixels per block of the joint kernels: >= 3 blocks per CU at the config sizes
constexpr int JOINT_GRID_CAP = 2048;  // 256 CUs x 8

// ---------------------------------------------------------------- patch-wise joints
// IIDSegmentationSmallPathLoss / patch_generator (contrastyou/losses/discreteMI.py:173-198,264-272): the loss of
// IIDSegmentationLoss on every square patch of the maps (side `patch`, step patch / 2), averaged.  Patch origins along an
// axis of length L: 0, s, 2s, ... below L - p, then max(L - p, 0); every patch is clipped to the map, so all patches of
// one call have the same extents eh x ew.  A patch is a window of the forward bodies above: the zero padding of a
// displaced read is at the PATCH border.
__host__ __device__ inline int patch_count(int L, int p) {
  const int s = p / 2;
  return L > p ? (L - p + s - 1) / s + 1 : 1;
}
__host__ __device__ inline int patch_origin(int i, int n, int L, int p) {
  return i < n - 1 ? i * (p / 2) : (L > p ? L - p : 0);
}

__device__ __forceinline__ joint_window patch_window(int q, int H, int W, int patch, int nph, int npw, int eh, int ew) {
  return joint_window{patch_origin(q / npw, nph, H, patch), patch_origin(q % npw, npw, W, patch), eh, ew};
}

// The two forward bodies on the window of patch blockIdx.z.  With gridDim.x == 1 the block's sums are the joint and go
// straight to J; otherwise to part[q][d][blockIdx.x][k*k].  The staged form:
__global__ void __launch_bounds__(256, 2)
    joint_patch_fwd_kernel(const float* __restrict__ x1, const float* __restrict__ x2, float* __restrict__ part,
                           float* __restrict__ J, int N, int H, int W, int k, int pad, int R, int patch, int nph,
                           int npw, int eh, int ew, double scale) {
  const int q = (int)blockIdx.z;
  joint_staged_body<false>(x1, x2, part, gridDim.x == 1 ? J : nullptr, scale, N, H, W, k, pad, R,
                           patch_window(q, H, W, patch, nph, npw, eh, ew), q);
}

// The fallback, the per-displacement form:
__global__ void __launch_bounds__(256)
    joint_patch_fwd1_kernel(const float* __restrict__ x1, const float* __restrict__ x2, float* __restrict__ part,
                            float* __restrict__ J, int N, int H, int W, int k, int pad, int patch, int nph, int npw,
                            int eh, int ew, double scale) {
  const int q = (int)blockIdx.z;
  joint_tile_body<false>(x1, x2, part, gridDim.x == 1 ? J : nullptr, scale, N, H, W, k, pad,
                         patch_window(q, H, W, patch, nph, npw, eh, ew), q);
}

// one block per patch on J[P][TT][k][k]: losses[q], Pj[q] (may be NULL) and dJ[q] (may be NULL) = (1/P) dloss_q/dJ_q
__global__ void __launch_bounds__(256)
    iid_patch_loss_kernel(const float* __restrict__ J, float* __restrict__ losses, float* __restrict__ Pj,
                          float* __restrict__ dJ, float* __restrict__ ws, size_t ws_floats, int TT, int k, int mode,
                          float lamda, float eps) {
  __shared__ double sred[256];
  const size_t q = blockIdx.x, n = (size_t)TT * k * k;
  iid_loss_body(J + q * n, losses + q, nullptr, Pj ? Pj + q * n : nullptr, dJ ? dJ + q * n : nullptr,
                ws + q * ws_floats, TT, k, mode, 0, lamda, eps, 1.0 / (double)gridDim.x, sred);
}

// loss[0] = mean of losses[P]: strided f64 sums per thread, then the block tree -- a fixed order
__global__ void __launch_bounds__(256)
    patch_mean_kernel(const float* __restrict__ losses, float* __restrict__ loss, int P) {
  __shared__ double sred[256];
  double s = 0.0;
  for (int q = threadIdx.x; q < P; q += 256) s += (double)losses[q];
  s = block_sum_d(s, sred);
  if (threadIdx.x == 0) loss[0] = (float)(s / (double)P);
}

// Adjoint of the patch joints in gather form: every output pixel walks the patches that contain it in ascending patch
// order and, inside each, the displacements whose other end lies in the same patch.  dJ is read from memory (P joints do
// not fit the LDS); neighbouring pixels read the same rows of it.
//   which = 0: dx1[pix][i] = g*scale * sum_q sum_{d,j} dJ[q][d][i][j] * x2[pix - disp(d)][j]
//   which = 1: dx2[pix][j] = g*scale * sum_q sum_{d,i} dJ[q][d][i][j] * x1[pix + disp(d)][i]
template <int V>  // V = 4: one thread per (pixel, 4 channels), k % 4 == 0; V = 1: one thread per (pixel, channel)
__global__ void __launch_bounds__(256)
    joint_patch_bwd_kernel(const float* __restrict__ other, const float* __restrict__ dJ,
                           const float* __restrict__ gscale, float* __restrict__ dx, int N, int H, int W, int k, int pad,
                           int patch, int nph, int npw, int eh, int ew, float scale, int which) {
  const int T = 2 * pad + 1, TT = T * T, kv = k / V, kk = k * k;
  const float g = gscale[0] * scale;
  const long total = (long)N * H * W * kv;
  const int sgn = which ? 1 : -1;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const int c = (int)(e % kv) * V;
    const long pix = e / kv;
    const int w = (int)(pix % W);
    const int h = (int)((pix / W) % H);
    float s[V];
#pragma unroll
    for (int u = 0; u < V; ++u) s[u] = 0.f;
    for (int ih = 0; ih < nph; ++ih) {
      const int lh = h - patch_origin(ih, nph, H, patch);
      if (lh < 0 || lh >= eh) continue;
      for (int iw = 0; iw < npw; ++iw) {
        const int lw = w - patch_origin(iw, npw, W, patch);
        if (lw < 0 || lw >= ew) continue;
        const float* dq = dJ + (size_t)(ih * npw + iw) * TT * kk;
        // 0 <= lh + sgn*du < eh  and  |du| <= pad
        const int ulo = which ? max(-pad, -lh) : max(-pad, lh - eh + 1), uhi = which ? min(pad, eh - 1 - lh) : min(pad, lh);
        const int vlo = which ? max(-pad, -lw) : max(-pad, lw - ew + 1), vhi = which ? min(pad, ew - 1 - lw) : min(pad, lw);
        for (int du = ulo; du <= uhi; ++du)
          for (int dv = vlo; dv <= vhi; ++dv) {
            joint_bwd_dot<V>(s, dq + ((du + pad) * T + dv + pad) * kk, other + (pix + sgn * ((long)du * W + dv)) * k, k,
                             c, which);
          }
      }
    }
    joint_bwd_store<V>(dx, pix * k + c, s, g);
  }
}

constexpr int JP_TARGET = 1024;   // blocks the staged forward aims at (4 per CU) before a block walks several tiles

struct patch_plan {
  int P, nph, npw, eh, ew, kernel, R, tiles_h, ntile, nbx, grid_y, fwd_lds, fwd_vec, staged_fits, bwd_kernel, bwd_grid;
  size_t ws_bytes;
};

constexpr int J_FWD_LDS = 150 * 1024;  // the staged tile of joint_fwd_multi_kernel (raised limit)
constexpr int J_BWD_LDS = 64 * 1024;   // the dJ chunk of the backward kernels (default limit)
constexpr int GS_LDS = 64 * 1024;      // the softmax tiles (default limit)

// The host's half of the launch rules that the whole-image and the patch-wise plans share (the kernels recompute kp and
// nsl from k, see joint_lanes_of).
struct joint_split {
  int kp, k4, nsl;
  size_t red;   // bytes of the reduction buffer [nsl][kp*kp]
  size_t tile;  // dynamic LDS of the per-displacement form: two 64-pixel tiles and the reduction buffer
};
joint_split joint_split_of(int k) {
  joint_split s;
  s.kp = (k + 3) & ~3;
  s.k4 = s.kp / 4;
  s.nsl = 256 / (s.k4 * s.k4);
  s.red = (size_t)s.nsl * s.kp * s.kp * sizeof(float);
  s.tile = 2 * J_P * s.kp * sizeof(float) + s.red;
  return s;
}

// The staged form on a window of eh x ew pixels: R rows of it per tile and the bytes of the staged tile (the reduction
// buffer lies over it); the form is taken where they fit J_FWD_LDS.
struct joint_staged {
  int R;
  size_t lds;
};
joint_staged joint_staged_of(int eh, int ew, int k, int pad) {
  const joint_split s = joint_split_of(k);
  joint_staged t;
  t.R = 256 / ew;
  t.R = t.R < 1 ? 1 : (t.R > eh ? eh : t.R);
  t.lds = ((size_t)(t.R + 2 * pad) * (ew + 2 * pad) * s.kp + (size_t)t.R * ew * s.kp) * sizeof(float);
  if (t.lds < s.red) t.lds = s.red;
  return t;
}

// The backward kernels, whole-image and patch-wise: the 16-byte form where k % 4 == 0, one thread per (pixel, V channels)
struct joint_bwd_rule {
  int vec, grid;
  long work;  // threads' worth of outputs
};
joint_bwd_rule joint_bwd_rule_of(long npix, int k) {
  joint_bwd_rule b;
  b.vec = (k & 3) == 0;
  b.work = b.vec ? npix * (k / 4) : npix * k;
  b.grid = cy_blocks(b.work, 256, GRID_CAP);
  return b;
}

}  // namespace

extern "C" {

// The launch rule of cy_joint_fwd / _bwd / _ws_bytes, once (the kernels recompute kp, nsl, per and nd from the same
// arguments; everything the host decides is decided here).
int cy_joint_plan(int N, int H, int W, int k, int pad, cy_joint_plan_t* out) {
  if (!out || N <= 0 || H <= 0 || W <= 0) return CY_ERR_ARG;
  if (k < 1 || k > J_KMAX || pad < 0 || pad >= H || pad >= W) return CY_ERR_SHAPE;
  cy_joint_plan_t p = {};
  const long npix = (long)N * H * W;
  const int T = 2 * pad + 1, TT = T * T;
  const joint_split s = joint_split_of(k);
  p.kp = s.kp;
  p.nsl = s.nsl;
  p.idle = 256 - s.nsl * s.k4 * s.k4;
  p.nblk = cy_blocks(npix, JOINT_PIX, JOINT_GRID_CAP);
  p.reduce_trips = cy_cdiv(p.nblk, 64);
  // padding > 0: every displacement from one staged tile of R rows, if it fits the LDS
  const joint_staged st = joint_staged_of(H, W, k, pad);
  if (pad > 0 && st.lds <= (size_t)J_FWD_LDS) {
    p.fwd_kernel = 1;
    p.fwd_vec = s.kp == k;
    p.R = st.R;
    p.tiles_h = cy_cdiv(H, st.R);
    p.ntile = N * p.tiles_h;
    p.grid_y = cy_cdiv(TT, JM_D);
    p.nd_last = TT - (p.grid_y - 1) * JM_D;
    p.fwd_lds = (int)st.lds;
  } else {
    p.fwd_kernel = 0;
    p.fwd_vec = pad == 0 && s.kp == k;
    p.per = (int)(((npix + p.nblk - 1) / p.nblk + J_P - 1) / J_P * J_P);
    p.ntile = cy_cdiv(npix, J_P);
    p.grid_y = TT;
    p.nd_last = 1;
    p.fwd_lds = (int)s.tile;
  }
  const joint_bwd_rule b = joint_bwd_rule_of(npix, k);
  p.bwd_kernel = b.vec;
  p.bwd_grid = b.grid;
  p.bwd_trips = cy_cdiv(b.work, 256L * p.bwd_grid);
  const int fit = J_BWD_LDS / (k * k * (int)sizeof(float));  // >= 4 because k <= 64
  p.bwd_dchunk = fit < TT ? fit : TT;
  p.bwd_nchunk = cy_cdiv(TT, p.bwd_dchunk);
  p.bwd_lds = p.bwd_dchunk * k * k * (int)sizeof(float);
  *out = p;
  return CY_OK;
}

// Forward: GS_PB rows per block.  Backward: two tiles, so GS_PB rows where they fit 64 KB (S*k <= 127) and GS_PB / 2
// beyond.  Both directions accept S*k <= 255 and refuse the rest here, before any launch.
int cy_group_softmax_plan(long M, int S, int k, cy_group_softmax_plan_t* out) {
  if (!out || M <= 0 || S <= 0 || k <= 0) return CY_ERR_ARG;
  if ((long)S * k > 255) return CY_ERR_SHAPE;
  cy_group_softmax_plan_t p = {};
  const int pitch = S * k + 1;
  p.fwd_rows = GS_PB;
  p.fwd_lds = GS_PB * pitch * (int)sizeof(float);
  p.bwd_rows = 2 * GS_PB * pitch * (int)sizeof(float) <= GS_LDS ? GS_PB : GS_PB / 2;
  p.bwd_lds = 2 * p.bwd_rows * pitch * (int)sizeof(float);
  p.fwd_ok = p.fwd_lds <= GS_LDS;
  p.bwd_ok = p.bwd_lds <= GS_LDS;
  if (!p.fwd_ok || !p.bwd_ok) return CY_ERR_SHAPE;
  if ((M + p.bwd_rows - 1) / p.bwd_rows > 0x7fffffffL) return CY_ERR_SHAPE;
  p.fwd_grid = cy_cdiv(M, p.fwd_rows);
  p.bwd_grid = cy_cdiv(M, p.bwd_rows);
  *out = p;
  return CY_OK;
}

int cy_group_softmax_fwd(const float* logits, float* probs, long M, int S, int k, float invT,
                         void* stream) {
  if (!logits || !probs || M <= 0 || S <= 0 || k <= 0) return CY_ERR_ARG;
  cy_group_softmax_plan_t p;
  const int rc = cy_group_softmax_plan(M, S, k, &p);
  if (rc != CY_OK) return rc;
  hipLaunchKernelGGL(group_softmax_fwd_kernel, dim3(p.fwd_grid), dim3(256), (size_t)p.fwd_lds,
                     (hipStream_t)stream, logits, probs, M, S, k, invT);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_group_softmax_bwd(const float* probs, const float* dprobs, float* dlogits, long M, int S,
                         int k, float invT, void* stream) {
  if (!probs || !dprobs || !dlogits || M <= 0 || S <= 0 || k <= 0) return CY_ERR_ARG;
  cy_group_softmax_plan_t p;
  const int rc = cy_group_softmax_plan(M, S, k, &p);
  if (rc != CY_OK) return rc;
  hipLaunchKernelGGL(group_softmax_bwd_kernel, dim3(p.bwd_grid), dim3(256), (size_t)p.bwd_lds,
                     (hipStream_t)stream, probs, dprobs, dlogits, M, S, k, invT, p.bwd_rows);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

size_t cy_joint_ws_bytes(int N, int H, int W, int k, int pad) {
  cy_joint_plan_t p;
  if (cy_joint_plan(N, H, W, k, pad, &p) != CY_OK) return 0;
  const int T = 2 * pad + 1;
  return (size_t)T * T * p.nblk * k * k * sizeof(float);
}

/* J[T*T][k][k] = scale * sum over pixels of x1[shifted] (x) x2 ; scale = 1/(N*H*W) when
 * normalise != 0 (the padding-0 segmentation joint), else 1. */
int cy_joint_fwd(const float* x1, const float* x2, float* J, int N, int H, int W, int k, int pad,
                 int normalise, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !J || N <= 0 || H <= 0 || W <= 0) return CY_ERR_ARG;
  cy_joint_plan_t p;
  const int rc = cy_joint_plan(N, H, W, k, pad, &p);
  if (rc != CY_OK) return rc;
  if (!ws || ws_bytes < cy_joint_ws_bytes(N, H, W, k, pad)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const long npix = (long)N * H * W;
  const int T = 2 * pad + 1;
  if (p.fwd_kernel == 1) {
    if (!cy_lds_limit_once<joint_fwd_multi_kernel>(J_FWD_LDS)) return CY_ERR_LAUNCH;
    hipLaunchKernelGGL(joint_fwd_multi_kernel, dim3(p.nblk, p.grid_y), dim3(256), (size_t)p.fwd_lds, st, x1, x2,
                       (float*)ws, N, H, W, k, pad, p.R);
  } else {
    hipLaunchKernelGGL(joint_fwd_kernel, dim3(p.nblk, p.grid_y), dim3(256), (size_t)p.fwd_lds, st, x1, x2,
                       (float*)ws, N, H, W, k, pad);
  }
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(joint_reduce_kernel, dim3(cy_cdiv((long)T * T * k * k, 4)), dim3(256), 0, st,
                     (const float*)ws, J, T * T, p.nblk, k * k,
                     normalise ? 1.0 / (double)npix : 1.0);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_joint_bwd(const float* x1, const float* x2, const float* dJ, const float* gscale, float* dx1,
                 float* dx2, int N, int H, int W, int k, int pad, int normalise, void* stream) {
  if (!x1 || !x2 || !dJ || !gscale || N <= 0 || H <= 0 || W <= 0) return CY_ERR_ARG;
  cy_joint_plan_t p;
  const int rc = cy_joint_plan(N, H, W, k, pad, &p);
  if (rc != CY_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const long npix = (long)N * H * W;
  const float scale = normalise ? (float)(1.0 / (double)npix) : 1.f;
  for (int which = 0; which < 2; ++which) {
    float* dst = which ? dx2 : dx1;
    const float* other = which ? x1 : x2;
    if (!dst) continue;
    if (p.bwd_kernel)
      hipLaunchKernelGGL(joint_bwd_kernel<4>, dim3(p.bwd_grid), dim3(256), (size_t)p.bwd_lds, st, other, dJ, gscale,
                         dst, N, H, W, k, pad, scale, which, p.bwd_dchunk);
    else
      hipLaunchKernelGGL(joint_bwd_kernel<1>, dim3(p.bwd_grid), dim3(256), (size_t)p.bwd_lds, st, other, dJ, gscale,
                         dst, N, H, W, k, pad, scale, which, p.bwd_dchunk);
    CY_CHECK_LAUNCH();
  }
  return CY_OK;
}

size_t cy_iid_loss_ws_bytes(int TT, int k) {
  return ((size_t)4 * TT * k * k + 2 * (size_t)TT * k + TT) * sizeof(float);
}

int cy_iid_loss(const float* J, float* out2, float* P, float* dJ, int TT, int k, int mode,
                int symmetric, float lamda, float eps, void* ws, size_t ws_bytes, void* stream) {
  if (!J || !out2 || TT <= 0 || k <= 0) return CY_ERR_ARG;
  if (mode < 0 || mode > 2 || k > J_KMAX) return CY_ERR_SHAPE;
  if (!ws || ws_bytes < cy_iid_loss_ws_bytes(TT, k)) return CY_ERR_WORKSPACE;
  hipLaunchKernelGGL(iid_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, J, out2, P, dJ,
                     (float*)ws, TT, k, mode, symmetric, lamda, eps);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

}  // extern "C"

namespace {

// The launch rule of the patch-wise entries, once.  kernel: -1 = the rule's choice, 0 / 1 = that forward kernel.
int patch_plan_of(int N, int H, int W, int k, int pad, int patch, int kernel, patch_plan* out) {
  if (N <= 0 || H <= 0 || W <= 0 || kernel < -1 || kernel > 1) return CY_ERR_ARG;
  if (k < 1 || k > J_KMAX || pad < 0 || patch < 2) return CY_ERR_SHAPE;
  patch_plan p = {};
  p.nph = patch_count(H, patch);
  p.npw = patch_count(W, patch);
  p.eh = H < patch ? H : patch;
  p.ew = W < patch ? W : patch;
  if (pad >= p.eh || pad >= p.ew) return CY_ERR_SHAPE;
  if ((long)p.nph * p.npw > 65535) return CY_ERR_SHAPE;  // gridDim.z
  p.P = p.nph * p.npw;
  const int T = 2 * pad + 1, TT = T * T;
  if ((long)p.P * TT * k * k > 0x7fffffffL) return CY_ERR_SHAPE;  // J is indexed with 32 bits in the reduction
  const joint_split s = joint_split_of(k);
  const joint_staged st = joint_staged_of(p.eh, p.ew, k, pad);
  p.staged_fits = st.lds <= (size_t)J_FWD_LDS;
  if (kernel == 1 && !p.staged_fits) return CY_ERR_SHAPE;
  p.kernel = kernel < 0 ? p.staged_fits : kernel;
  const int tiles_h = cy_cdiv(p.eh, st.R), ntile = N * tiles_h, groups = cy_cdiv(TT, JM_D);
  int nbx1 = cy_cdiv(JP_TARGET, (long)p.P * groups);
  nbx1 = nbx1 > ntile ? ntile : nbx1;
  const int nbx0 = cy_blocks((long)N * p.eh * p.ew, JOINT_PIX, JOINT_GRID_CAP);
  if (p.kernel == 1) {
    p.R = st.R;
    p.tiles_h = tiles_h;
    p.ntile = ntile;
    p.nbx = nbx1;
    p.grid_y = groups;
    p.fwd_lds = (int)st.lds;
    p.fwd_vec = s.kp == k;
  } else {
    p.ntile = cy_cdiv((long)N * p.eh * p.ew, J_P);
    p.nbx = nbx0;
    p.grid_y = TT;
    p.fwd_lds = (int)s.tile;
  }
  // the partial joints of the forward; a forward with one block per (patch, group) writes J itself
  p.ws_bytes = p.nbx > 1 ? (size_t)p.P * TT * p.nbx * k * k * sizeof(float) : 16;
  const joint_bwd_rule b = joint_bwd_rule_of((long)N * H * W, k);
  p.bwd_kernel = b.vec;
  p.bwd_grid = b.grid;
  *out = p;
  return CY_OK;
}

}  // namespace

extern "C" {

int cy_joint_patch_plan(int N, int H, int W, int k, int pad, int patch, int kernel, cy_joint_patch_plan_t* out) {
  if (!out) return CY_ERR_ARG;
  patch_plan p;
  const int rc = patch_plan_of(N, H, W, k, pad, patch, kernel, &p);
  if (rc != CY_OK) return rc;
  out->P = p.P, out->nph = p.nph, out->npw = p.npw, out->eh = p.eh, out->ew = p.ew, out->fwd_kernel = p.kernel;
  out->R = p.R, out->tiles_h = p.tiles_h, out->ntile = p.ntile, out->nbx = p.nbx, out->grid_y = p.grid_y;
  out->fwd_lds = p.fwd_lds, out->fwd_vec = p.fwd_vec, out->staged_fits = p.staged_fits;
  out->bwd_kernel = p.bwd_kernel, out->bwd_grid = p.bwd_grid;
  return CY_OK;
}

size_t cy_joint_patch_ws_bytes(int N, int H, int W, int k, int pad, int patch, int kernel) {
  patch_plan p;
  if (patch_plan_of(N, H, W, k, pad, patch, kernel, &p) != CY_OK) return 0;
  return p.ws_bytes;
}

int cy_joint_patch_fwd(const float* x1, const float* x2, float* J, int N, int H, int W, int k, int pad, int patch,
                       int normalise, int kernel, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !J) return CY_ERR_ARG;
  patch_plan p;
  const int rc = patch_plan_of(N, H, W, k, pad, patch, kernel, &p);
  if (rc != CY_OK) return rc;
  if (!ws || ws_bytes < p.ws_bytes) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int T = 2 * pad + 1, TT = T * T;
  const double scale = normalise ? 1.0 / ((double)N * p.eh * p.ew) : 1.0;
  if (p.kernel == 1) {
    if (!cy_lds_limit_once<joint_patch_fwd_kernel>(J_FWD_LDS)) return CY_ERR_LAUNCH;
    hipLaunchKernelGGL(joint_patch_fwd_kernel, dim3(p.nbx, p.grid_y, p.P), dim3(256), (size_t)p.fwd_lds, st, x1, x2,
                       (float*)ws, J, N, H, W, k, pad, p.R, patch, p.nph, p.npw, p.eh, p.ew, scale);
  } else {
    hipLaunchKernelGGL(joint_patch_fwd1_kernel, dim3(p.nbx, p.grid_y, p.P), dim3(256), (size_t)p.fwd_lds, st, x1, x2,
                       (float*)ws, J, N, H, W, k, pad, patch, p.nph, p.npw, p.eh, p.ew, scale);
  }
  CY_CHECK_LAUNCH();
  if (p.nbx > 1) {
    hipLaunchKernelGGL(joint_reduce_kernel, dim3(cy_cdiv((long)p.P * TT * k * k, 4)), dim3(256), 0, st,
                       (const float*)ws, J, p.P * TT, p.nbx, k * k, scale);
    CY_CHECK_LAUNCH();
  }
  return CY_OK;
}

size_t cy_iid_patch_loss_ws_bytes(int P, int TT, int k) {
  if (P <= 0 || TT <= 0 || k <= 0 || k > J_KMAX) return 0;
  return (size_t)P * cy_iid_loss_ws_bytes(TT, k);
}

int cy_iid_patch_loss(const float* J, float* loss, float* losses, float* Pj, float* dJ, int P, int TT, int k, int mode,
                      float lamda, float eps, void* ws, size_t ws_bytes, void* stream) {
  if (!J || !loss || !losses || P <= 0 || TT <= 0 || k <= 0) return CY_ERR_ARG;
  if (mode < 0 || mode > 1 || k > J_KMAX) return CY_ERR_SHAPE;
  if (!ws || ws_bytes < cy_iid_patch_loss_ws_bytes(P, TT, k)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(iid_patch_loss_kernel, dim3(P), dim3(256), 0, st, J, losses, Pj, dJ, (float*)ws,
                     cy_iid_loss_ws_bytes(TT, k) / sizeof(float), TT, k, mode, lamda, eps);
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(patch_mean_kernel, dim3(1), dim3(256), 0, st, (const float*)losses, loss, P);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_joint_patch_bwd(const float* x1, const float* x2, const float* dJ, const float* gscale, float* dx1, float* dx2,
                       int N, int H, int W, int k, int pad, int patch, int normalise, void* stream) {
  if (!x1 || !x2 || !dJ || !gscale) return CY_ERR_ARG;
  patch_plan p;
  const int rc = patch_plan_of(N, H, W, k, pad, patch, -1, &p);
  if (rc != CY_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const float scale = normalise ? (float)(1.0 / ((double)N * p.eh * p.ew)) : 1.f;
  for (int which = 0; which < 2; ++which) {
    float* dst = which ? dx2 : dx1;
    const float* other = which ? x1 : x2;
    if (!dst) continue;
    if (p.bwd_kernel)
      hipLaunchKernelGGL(joint_patch_bwd_kernel<4>, dim3(p.bwd_grid), dim3(256), 0, st, other, dJ, gscale, dst, N, H, W,
                         k, pad, patch, p.nph, p.npw, p.eh, p.ew, scale, which);
    else
      hipLaunchKernelGGL(joint_patch_bwd_kernel<1>, dim3(p.bwd_grid), dim3(256), 0, st, other, dJ, gscale, dst, N, H, W,
                         k, pad, patch, p.nph, p.npw, p.eh, p.ew, scale, which);
    CY_CHECK_LAUNCH();
  }
  return CY_OK;
}

}  // extern "C"
