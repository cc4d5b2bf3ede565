// On-device SLIC superpixels: Gaussian blur + 16-bit quantisation, windowed k-means on integers, 4-connected
// components with the small ones merged into their left / upper neighbour.  Produces the per-slice id map that
//   semi_seg/hooks/infonce.py:24-27,308-340   (_load_superpixel_image, _SuperPixelInfoNCEEPochHook) reads from
//   script/create_superpixel.py:27             (skimage.segmentation.slic(n_segments=40, sigma=5, compactness=0.1))
// Every sum after the blur is over integers (LDS and global integer atomics), and every choice is defined by an order
// on integers (smallest key, then smallest centre; root = smallest pixel index), so two runs give the same bits and
// the NumPy restatement of tests/slic_cases.py reproduces the device exactly.  No host read, no allocation.
#include <math.h>

#include "cy_common.h"

#define CY_SLIC_TH 16   // blur tile: 16 rows x 64 columns of outputs per block of 256
#define CY_SLIC_TW 64
#define CY_SLIC_MAX_R 64  // int(4 * CY_SLIC_MAX_SIGMA + 0.5)
#define CY_SLIC_SCAN 1024  // threads of the numbering block (one block per image)

namespace {

struct SlicTaps {
  float w[CY_SLIC_MAX_R + 1];  // w[|i|], normalised in f64 over i = -r .. r, then cast
};

struct SlicGeom {
  int r, S, start, Ky, Kx, K, M, min_size;
};

// scipy.ndimage's "reflect" (d c b a | a b c d | d c b a), one fold: exact for -n <= i <= 2n - 1, which covers every
// tap of a real output because r <= n.  Rows / columns of a tile past the image fold further out: clamped, never used.
__device__ __forceinline__ int slic_reflect(int i, int n) {
  i = i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i);
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// floor(clamp(v, 0, 1) * 65535 + 0.5), evaluated in f64: the product of an f32 and 65535 and the sum with 0.5 are
// exact there, so q is the exact quantisation of the f32 value.  A NaN counts as 0.
__device__ __forceinline__ int32_t slic_quant(float v) {
  v = !(v > 0.f) ? 0.f : (v > 1.f ? 1.f : v);
  return (int32_t)floor((double)v * 65535.0 + 0.5);
}

// One pass of the separable blur along AXIS (0: H, 1: W) through an LDS tile with a halo of r on both sides of that
// axis.  Taps run i = -r .. r in order, each product rounded to f32, then added (not fused).  QUANT: the pass writes q.
template <int AXIS, bool QUANT>
__global__ void __launch_bounds__(256)
    slic_blur_kernel(const float* __restrict__ in, void* __restrict__ out, int H, int W, int r, SlicTaps taps) {
  extern __shared__ float s_tile[];
  __shared__ float s_w[CY_SLIC_MAX_R + 1];
  if (threadIdx.x <= CY_SLIC_MAX_R) s_w[threadIdx.x] = taps.w[threadIdx.x];
  const long base = (long)blockIdx.z * H * W;
  const int x0 = blockIdx.x * CY_SLIC_TW, y0 = blockIdx.y * CY_SLIC_TH;
  const int rows = AXIS == 0 ? CY_SLIC_TH + 2 * r : CY_SLIC_TH;
  const int cols = AXIS == 1 ? CY_SLIC_TW + 2 * r : CY_SLIC_TW;
  for (int e = threadIdx.x; e < rows * cols; e += 256) {
    const int ly = e / cols, lx = e % cols;
    int gy = y0 + ly, gx = x0 + lx;
    if (AXIS == 0) gy = slic_reflect(gy - r, H);
    if (AXIS == 1) gx = slic_reflect(gx - r, W);
    s_tile[e] = (gy < H && gx < W) ? in[base + (long)gy * W + gx] : 0.f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < CY_SLIC_TH * CY_SLIC_TW; e += 256) {
    const int ly = e / CY_SLIC_TW, lx = e % CY_SLIC_TW;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    const float* c = s_tile + (AXIS == 0 ? (ly + r) * cols + lx : ly * cols + lx + r);
    const int step = AXIS == 0 ? cols : 1;
    float acc = 0.f;
    {
#pragma clang fp contract(off)  // product and sum each rounded to f32, as the restatement does: no fma
      for (int i = -r; i <= r; ++i) acc = acc + s_w[i < 0 ? -i : i] * c[i * step];
    }
    const long at = base + (long)y * W + x;
    if (QUANT)
      ((int32_t*)out)[at] = slic_quant(acc);
    else
      ((float*)out)[at] = acc;
  }
}

// sigma == 0: no blur, quantise only
__global__ void __launch_bounds__(256)
    slic_quant_kernel(const float* __restrict__ in, int32_t* __restrict__ q, int HW) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const long at = (long)blockIdx.y * HW + p;
  if (p < HW) q[at] = slic_quant(in[at]);
}

// centres on the regular grid (cy, cx, q there), every label 0, the sums of the first round 0
__global__ void __launch_bounds__(256)
    slic_init_kernel(const int32_t* __restrict__ q, int32_t* __restrict__ labels, int32_t* __restrict__ centres,
                     unsigned long long* __restrict__ acc, int H, int W, SlicGeom g) {
  const int HW = H * W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const long n = blockIdx.y;
  if (p < HW) labels[n * HW + p] = 0;
  if (p < g.K) {
    const int cy = g.start + (p / g.Kx) * g.S, cx = g.start + (p % g.Kx) * g.S;
    int32_t* c = centres + (n * g.K + p) * 3;
    c[0] = cy, c[1] = cx, c[2] = q[n * HW + (long)cy * W + cx];
    unsigned long long* a = acc + (n * g.K + p) * 4;
    a[0] = a[1] = a[2] = a[3] = 0ull;
  }
}

// Assignment (a gather: every pixel loops over the K <= 100 centres, smallest key, ties to the smallest k) and the
// block's share of the update sums.  The centres are read with a wave-uniform index straight from global memory
// (scalar loads: the loop leaves the LDS pipe alone).  The sums of a block's 256 pixels go through LDS integer atomics:
// cnt (<= 256, 9 bits), sum y and sum x (<= 256 * 1023, 18 bits each) packed into one 64-bit word, sum q (<= 256 *
// 65535) in a 32-bit one; then one int64 global atomic per touched (centre, sum).  Integer sums, so the order the
// atomics land in does not matter.
#define CY_SLIC_PACK_Y 9
#define CY_SLIC_PACK_X 27
__global__ void __launch_bounds__(256)
    slic_assign_kernel(const int32_t* __restrict__ q, int32_t* __restrict__ labels,
                       const int32_t* __restrict__ centres, unsigned long long* __restrict__ acc, int H, int W, int K,
                       int S, uint32_t S2, uint32_t M2) {
  __shared__ unsigned long long s_cyx[CY_SLIC_MAX_K];
  __shared__ uint32_t s_q[CY_SLIC_MAX_K];
  const int HW = H * W;
  const long n = blockIdx.y;
  const int32_t* c = centres + n * 3 * K;
  for (int i = threadIdx.x; i < K; i += 256) s_cyx[i] = 0ull, s_q[i] = 0u;
  __syncthreads();
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < HW) {
    const int y = p / W, x = p % W;
    const int32_t qq = q[n * HW + p];
    const int reach = 2 * S;
    int best = -1;
    unsigned long long best_key = 0;
    for (int k = 0; k < K; ++k) {
      const int dy = y - c[3 * k], dx = x - c[3 * k + 1];
      if (dy > reach || dy < -reach || dx > reach || dx < -reach) continue;
      // |dc| < 2^16 and |dy|, |dx| < 2^11: 24-bit products; dc^2 < 2^32, S^2 <= 2^20, d^2 < 2^23, M^2 < 2^32, so the
      // key is two 32 x 32 -> 64 bit products (below 2^52 and 2^55)
      const int dc = qq - c[3 * k + 2];
      const uint32_t ay = dy < 0 ? -dy : dy, ax = dx < 0 ? -dx : dx, ac = dc < 0 ? -dc : dc;
      const uint32_t d2 = __umul24(ay, ay) + __umul24(ax, ax);
      const unsigned long long key = (unsigned long long)__umul24(ac, ac) * S2 + (unsigned long long)d2 * M2;
      if (best < 0 || key < best_key) best = k, best_key = key;
    }
    if (best < 0)
      best = labels[n * HW + p];  // no window covers it: the label stays (0 .. K-1 since slic_init_kernel)
    else
      labels[n * HW + p] = best;
    atomicAdd(&s_cyx[best],
              1ull | ((unsigned long long)y << CY_SLIC_PACK_Y) | ((unsigned long long)x << CY_SLIC_PACK_X));
    atomicAdd(&s_q[best], (uint32_t)qq);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += 256) {
    const unsigned long long v = s_cyx[k];
    if (!v) continue;  // cnt == 0
    unsigned long long* a = acc + (n * K + k) * 4;
    atomicAdd(&a[0], v & 511ull);
    atomicAdd(&a[1], (v >> CY_SLIC_PACK_Y) & 0x3ffffull);
    atomicAdd(&a[2], v >> CY_SLIC_PACK_X);
    atomicAdd(&a[3], (unsigned long long)s_q[k]);
  }
}

// Update: c = (2 * sum + cnt) / (2 * cnt) for y, x and q; an empty centre stays.  Clears the sums for the next round.
__global__ void __launch_bounds__(256)
    slic_update_kernel(int32_t* __restrict__ centres, unsigned long long* __restrict__ acc, long NK) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= NK) return;
  unsigned long long* a = acc + i * 4;
  const unsigned long long cnt = a[0];
  if (cnt) {
    int32_t* c = centres + i * 3;
    for (int j = 0; j < 3; ++j) c[j] = (int32_t)((2ull * a[j + 1] + cnt) / (2ull * cnt));
  }
  a[0] = a[1] = a[2] = a[3] = 0ull;
}

// ---- connected components: union-find over global memory.  parent[x] <= x always and a link always goes from the
// larger root to the smaller, so whatever order the threads run in, the root of a component ends as its smallest index.
__device__ __forceinline__ int cc_find(const int32_t* parent, int x) {
  int p;
  while ((p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED)) != x) x = p;
  return x;
}

__device__ __forceinline__ void cc_union(int32_t* parent, int a, int b) {
  for (;;) {
    a = cc_find(parent, a), b = cc_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicMin(&parent[a], b);
    if (old == a) return;  // a was a root and now hangs under b
    a = old;               // a had been linked under `old` meanwhile: old and b are still to be joined
  }
}

// parent[p] = the first pixel of p's horizontal run of equal labels, as far as p's wave of 64 consecutive pixels sees
// it (the pixel before the wave where the run began earlier): the runs are joined without a single union.
__global__ void __launch_bounds__(256)
    cc_init_kernel(const int32_t* __restrict__ labels, int32_t* __restrict__ parent, int32_t* __restrict__ size, int HW,
                   int W) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const long at = (long)blockIdx.y * HW + p;
  const int lane = threadIdx.x & 63;
  const bool same = p < HW && p % W > 0 && labels[at - 1] == labels[at];
  const unsigned long long run = __ballot(same);
  const unsigned long long breaks = ~run & ((2ull << lane) - 1ull);  // lanes 0 .. lane that start a run
  const int back = breaks ? lane - (63 - __clzll((long long)breaks)) : lane + 1;
  if (p < HW) parent[at] = p - back, size[at] = 0;
}

// joins the runs of adjacent rows: one union per stretch of pixels that continue both a run above and their own
__global__ void __launch_bounds__(256)
    cc_merge_kernel(const int32_t* __restrict__ labels, int32_t* __restrict__ parent, int H, int W) {
  const int HW = H * W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < W || p >= HW) return;
  const int32_t* lab = labels + (long)blockIdx.y * HW;
  const int32_t l = lab[p];
  if (lab[p - W] != l) return;
  if (p % W > 0 && lab[p - 1] == l && lab[p - W - 1] == l) return;  // the pixel to the left makes this join
  cc_union(parent + (long)blockIdx.y * HW, p, p - W);
}

// every pixel points at its root; the root's size counts its pixels, one atomic per root and wave
__global__ void __launch_bounds__(256)
    cc_flatten_kernel(int32_t* __restrict__ parent, int32_t* __restrict__ size, int HW) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int32_t* par = parent + (long)blockIdx.y * HW;
  int root = -1;
  if (p < HW) {
    root = cc_find(par, p);
    __atomic_store_n(&par[p], root, __ATOMIC_RELAXED);
  }
  bool todo = p < HW;
  for (unsigned long long left = __ballot(todo); left; left = __ballot(todo)) {
    const int leader = __ffsll((long long)left) - 1;
    const int r0 = __shfl(root, leader);
    const bool mine = todo && root == r0;
    const unsigned long long same = __ballot(mine);
    if (lane == leader) atomicAdd(&size[(long)blockIdx.y * HW + r0], (int)__popcll(same));
    if (mine) todo = false;
  }
}

// One block per image, tiles of 1024 consecutive pixels.  For every root: link[root] = root for a kept component
// (size >= min_size, or root 0), else the root of the component that owns the pixel left of the root (above it in
// column 0) -- a smaller root, so the links form a DAG ordered by root.  The kept roots are numbered 0, 1, ... by
// increasing index (ballot within a wave, the 16 wave totals through LDS, a running base over the tiles).
__global__ void __launch_bounds__(CY_SLIC_SCAN)
    cc_number_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ size, int32_t* __restrict__ link,
                     int32_t* __restrict__ newid, int32_t* __restrict__ count, int HW, int W, int min_size) {
  __shared__ int32_t s_n[CY_SLIC_SCAN / 64];
  const long o = (long)blockIdx.x * HW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;
  for (int p0 = 0; p0 < HW; p0 += CY_SLIC_SCAN) {
    const int p = p0 + threadIdx.x;
    const bool root = p < HW && parent[o + p] == p;
    const bool kept = root && (p == 0 || size[o + p] >= min_size);
    if (root) link[o + p] = kept ? p : parent[o + (p % W > 0 ? p - 1 : p - W)];
    const unsigned long long m = __ballot(kept);
    if (lane == 0) s_n[wave] = (int)__popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < CY_SLIC_SCAN / 64; ++w) {
      before += w < wave ? s_n[w] : 0;
      total += s_n[w];
    }
    if (kept) newid[o + p] = base + before + (int)__popcll(m & ((1ull << lane) - 1ull));
    base += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) count[blockIdx.x] = base;
}

// every pixel follows its root's links down to a kept root (link is read-only here) and takes that root's number
__global__ void __launch_bounds__(256)
    cc_write_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ link,
                    const int32_t* __restrict__ newid, uint8_t* __restrict__ ids, int HW) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const long o = (long)blockIdx.y * HW;
  int f = parent[o + p], nx;
  while ((nx = link[o + f]) != f) f = nx;
  ids[o + p] = (uint8_t)newid[o + f];
}

// ---- host ---------------------------------------------------------------------------------------------------------
inline int slic_check_shape(int N, int H, int W) {
  if (N < 1) return CY_ERR_ARG;
  if (H < 1 || W < 1 || H > CY_SLIC_MAX_SIDE || W > CY_SLIC_MAX_SIDE || N > 65535) return CY_ERR_SHAPE;
  return CY_OK;
}

// the grid of centres (skimage.util.regular_grid for a 2-D slice) and what follows from K
inline int slic_grid(int H, int W, int n_segments, SlicGeom* g) {
  if (n_segments < 1) return CY_ERR_ARG;
  const double s = sqrt((double)H * W / n_segments);
  g->S = (int)nearbyint(s);  // round half to even
  g->start = (int)floor(s / 2.0);
  if (g->S < 1) return CY_ERR_SHAPE;
  g->Ky = g->start < H ? (H - 1 - g->start) / g->S + 1 : 0;
  g->Kx = g->start < W ? (W - 1 - g->start) / g->S + 1 : 0;
  g->K = g->Ky * g->Kx;
  if (g->K < 1 || g->K > CY_SLIC_MAX_K || (long)H * W < 64L * g->K) return CY_ERR_SHAPE;
  g->min_size = (H * W) / (2 * g->K);
  return CY_OK;
}

inline int slic_blur_radius(int H, int W, double sigma, int* r) {
  if (!(sigma >= 0.0)) return CY_ERR_ARG;
  if (sigma > CY_SLIC_MAX_SIGMA) return CY_ERR_SHAPE;
  *r = (int)(4.0 * sigma + 0.5);
  if (*r > (H < W ? H : W)) return CY_ERR_SHAPE;
  return CY_OK;
}

inline int slic_compactness(double compactness, int* M) {
  if (!isfinite(compactness)) return CY_ERR_ARG;
  const double m = nearbyint(compactness * 65535.0);
  if (m < 1.0 || m > 65535.0) return CY_ERR_ARG;
  *M = (int)m;
  return CY_OK;
}

inline size_t slic_align(size_t b) { return (b + 255) / 256 * 256; }
// the workspace: [scratch 4 planes][sums N*K*4 u64][q plane][labels plane][centres N*K*3 i32]; a plane is N*H*W i32
inline size_t slic_plane(int N, int H, int W) { return slic_align((size_t)N * H * W * 4); }
inline size_t slic_acc_bytes(int N, int K) { return slic_align((size_t)N * K * 4 * 8); }

struct SlicWs {
  int32_t *p0, *p1, *p2, *p3, *q, *labels, *centres;
  unsigned long long* acc;
};

inline SlicWs slic_carve(void* ws, int N, int H, int W, int K) {
  uint8_t* b = (uint8_t*)ws;
  const size_t pl = slic_plane(N, H, W);
  SlicWs o;
  o.p0 = (int32_t*)b, o.p1 = (int32_t*)(b + pl), o.p2 = (int32_t*)(b + 2 * pl), o.p3 = (int32_t*)(b + 3 * pl);
  o.acc = (unsigned long long*)(b + 4 * pl);
  b += 4 * pl + slic_acc_bytes(N, K);
  o.q = (int32_t*)b, o.labels = (int32_t*)(b + pl), o.centres = (int32_t*)(b + 2 * pl);
  return o;
}

int slic_blur_launch(const float* images, int32_t* q, int N, int H, int W, double sigma, int r, float* tmp,
                     hipStream_t st) {
  const int HW = H * W;
  if (sigma == 0.0) {
    hipLaunchKernelGGL(slic_quant_kernel, dim3(cy_cdiv(HW, 256), N), dim3(256), 0, st, images, q, HW);
    CY_CHECK_LAUNCH();
    return CY_OK;
  }
  SlicTaps taps;
  double w[CY_SLIC_MAX_R + 1], sum = 0.0;
  for (int i = 0; i <= r; ++i) w[i] = exp(-0.5 * ((double)i / sigma) * ((double)i / sigma));
  for (int i = -r; i <= r; ++i) sum += w[i < 0 ? -i : i];
  for (int i = 0; i <= CY_SLIC_MAX_R; ++i) taps.w[i] = i <= r ? (float)(w[i] / sum) : 0.f;
  const dim3 grid(cy_cdiv(W, CY_SLIC_TW), cy_cdiv(H, CY_SLIC_TH), N);
  const size_t lds_h = (size_t)(CY_SLIC_TH + 2 * r) * CY_SLIC_TW * sizeof(float);
  const size_t lds_w = (size_t)CY_SLIC_TH * (CY_SLIC_TW + 2 * r) * sizeof(float);
  hipLaunchKernelGGL((slic_blur_kernel<0, false>), grid, dim3(256), lds_h, st, images, (void*)tmp, H, W, r, taps);
  hipLaunchKernelGGL((slic_blur_kernel<1, true>), grid, dim3(256), lds_w, st, (const float*)tmp, (void*)q, H, W, r,
                     taps);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int slic_cluster_launch(const int32_t* q, int32_t* labels, int32_t* centres, unsigned long long* acc, int N, int H,
                        int W, const SlicGeom& g, int max_iter, hipStream_t st) {
  const int HW = H * W;
  const dim3 grid(cy_cdiv(HW, 256), N);
  hipLaunchKernelGGL(slic_init_kernel, grid, dim3(256), 0, st, q, labels, centres, acc, H, W, g);
  const long NK = (long)N * g.K;
  for (int it = 0; it < max_iter; ++it) {
    hipLaunchKernelGGL(slic_assign_kernel, grid, dim3(256), 0, st, q, labels, (const int32_t*)centres, acc, H, W, g.K,
                       g.S, (uint32_t)(g.S * g.S), (uint32_t)g.M * (uint32_t)g.M);
    hipLaunchKernelGGL(slic_update_kernel, dim3(cy_cdiv(NK, 256)), dim3(256), 0, st, centres, acc, NK);
  }
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int slic_connect_launch(const int32_t* labels, uint8_t* ids, int32_t* count, int N, int H, int W, int min_size,
                        const SlicWs& w, hipStream_t st) {
  const int HW = H * W;
  const dim3 grid(cy_cdiv(HW, 256), N);
  int32_t *parent = w.p0, *size = w.p1, *link = w.p2, *newid = w.p3;
  hipLaunchKernelGGL(cc_init_kernel, grid, dim3(256), 0, st, labels, parent, size, HW, W);
  hipLaunchKernelGGL(cc_merge_kernel, grid, dim3(256), 0, st, labels, parent, H, W);
  hipLaunchKernelGGL(cc_flatten_kernel, grid, dim3(256), 0, st, parent, size, HW);
  hipLaunchKernelGGL(cc_number_kernel, dim3(N), dim3(CY_SLIC_SCAN), 0, st, (const int32_t*)parent,
                     (const int32_t*)size, link, newid, count, HW, W, min_size);
  hipLaunchKernelGGL(cc_write_kernel, grid, dim3(256), 0, st, (const int32_t*)parent, (const int32_t*)link,
                     (const int32_t*)newid, ids, HW);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

}  // namespace

extern "C" {

size_t cy_slic_ws_bytes(int N, int H, int W, int n_segments) {
  SlicGeom g;
  if (slic_check_shape(N, H, W) != CY_OK || slic_grid(H, W, n_segments, &g) != CY_OK) return 0;
  return 6 * slic_plane(N, H, W) + slic_acc_bytes(N, g.K) + slic_align((size_t)N * g.K * 3 * 4);
}

int cy_slic_plan(int N, int H, int W, int n_segments, double sigma, double compactness, int max_iter,
                 cy_slic_plan_t* out) {
  if (!out) return CY_ERR_ARG;
  *out = {};
  SlicGeom g = {};
  int rc = max_iter < 0 ? CY_ERR_ARG : slic_check_shape(N, H, W);
  if (rc == CY_OK) rc = slic_blur_radius(H, W, sigma, &g.r);
  if (rc == CY_OK) rc = slic_compactness(compactness, &g.M);
  if (rc == CY_OK) rc = slic_grid(H, W, n_segments, &g);
  out->status = rc;
  if (rc != CY_OK) return rc;
  const int HW = H * W;
  out->r = g.r, out->S = g.S, out->start = g.start;
  out->Ky = g.Ky, out->Kx = g.Kx, out->K = g.K;
  out->M = g.M, out->min_size = g.min_size;
  out->blur_form = sigma == 0.0 ? CY_SLIC_BLUR_QUANT : CY_SLIC_BLUR_TWO_PASS;
  out->blur_grid_x = sigma == 0.0 ? cy_cdiv(HW, 256) : cy_cdiv(W, CY_SLIC_TW);
  out->blur_grid_y = sigma == 0.0 ? N : cy_cdiv(H, CY_SLIC_TH);
  out->blur_lds_h = sigma == 0.0 ? 0 : (CY_SLIC_TH + 2 * g.r) * CY_SLIC_TW * 4;
  out->blur_lds_w = sigma == 0.0 ? 0 : CY_SLIC_TH * (CY_SLIC_TW + 2 * g.r) * 4;
  out->pixel_grid_x = cy_cdiv(HW, 256);
  out->assign_lds = 12 * CY_SLIC_MAX_K;
  out->update_grid = cy_cdiv((long)N * g.K, 256);
  out->scan_tiles = cy_cdiv(HW, CY_SLIC_SCAN);
  out->launches = (sigma == 0.0 ? 1 : 2) + 1 + 2 * max_iter + 5;
  return CY_OK;
}

int cy_slic_blur_q(const float* images, int32_t* q, int N, int H, int W, double sigma, void* ws, size_t ws_bytes,
                   void* stream) {
  if (!images || !q || !ws) return CY_ERR_ARG;
  int r = 0;
  int rc = slic_check_shape(N, H, W);
  if (rc == CY_OK) rc = slic_blur_radius(H, W, sigma, &r);
  if (rc != CY_OK) return rc;
  if (ws_bytes < slic_plane(N, H, W)) return CY_ERR_WORKSPACE;
  return slic_blur_launch(images, q, N, H, W, sigma, r, (float*)ws, (hipStream_t)stream);
}

int cy_slic_cluster(const int32_t* q, int32_t* labels, int32_t* centres, int N, int H, int W, int n_segments,
                    double compactness, int max_iter, void* ws, size_t ws_bytes, void* stream) {
  if (!q || !labels || !centres || !ws || max_iter < 0) return CY_ERR_ARG;
  SlicGeom g = {};
  int rc = slic_check_shape(N, H, W);
  if (rc == CY_OK) rc = slic_compactness(compactness, &g.M);
  if (rc == CY_OK) rc = slic_grid(H, W, n_segments, &g);
  if (rc != CY_OK) return rc;
  if (ws_bytes < cy_slic_ws_bytes(N, H, W, n_segments)) return CY_ERR_WORKSPACE;
  const SlicWs w = slic_carve(ws, N, H, W, g.K);
  return slic_cluster_launch(q, labels, centres, w.acc, N, H, W, g, max_iter, (hipStream_t)stream);
}

int cy_slic_connect(const int32_t* labels, uint8_t* ids, int32_t* count, int N, int H, int W, int n_segments, void* ws,
                    size_t ws_bytes, void* stream) {
  if (!labels || !ids || !count || !ws) return CY_ERR_ARG;
  SlicGeom g = {};
  int rc = slic_check_shape(N, H, W);
  if (rc == CY_OK) rc = slic_grid(H, W, n_segments, &g);
  if (rc != CY_OK) return rc;
  if (ws_bytes < cy_slic_ws_bytes(N, H, W, n_segments)) return CY_ERR_WORKSPACE;
  return slic_connect_launch(labels, ids, count, N, H, W, g.min_size, slic_carve(ws, N, H, W, g.K),
                             (hipStream_t)stream);
}

int cy_slic(const float* images, uint8_t* ids, int32_t* count, int N, int H, int W, int n_segments, double sigma,
            double compactness, int max_iter, void* ws, size_t ws_bytes, void* stream) {
  if (!images || !ids || !count || !ws || max_iter < 0) return CY_ERR_ARG;
  SlicGeom g = {};
  int rc = slic_check_shape(N, H, W);
  if (rc == CY_OK) rc = slic_blur_radius(H, W, sigma, &g.r);
  if (rc == CY_OK) rc = slic_compactness(compactness, &g.M);
  if (rc == CY_OK) rc = slic_grid(H, W, n_segments, &g);
  if (rc != CY_OK) return rc;
  if (ws_bytes < cy_slic_ws_bytes(N, H, W, n_segments)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const SlicWs w = slic_carve(ws, N, H, W, g.K);
  rc = slic_blur_launch(images, w.q, N, H, W, sigma, g.r, (float*)w.p0, st);
  if (rc == CY_OK) rc = slic_cluster_launch(w.q, w.labels, w.centres, w.acc, N, H, W, g, max_iter, st);
  if (rc == CY_OK) rc = slic_connect_launch(w.labels, ids, count, N, H, W, g.min_size, w, st);
  return rc;
}

}  // extern "C"
