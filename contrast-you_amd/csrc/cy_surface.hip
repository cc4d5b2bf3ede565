// Surface-distance statistics of two class-index volumes: border voxels, exact squared Euclidean distance transform,
// and per (direction, class) the count / sum of distances / maximum squared distance that ASD, HD and HD95 are made of.
//   contrastyou/meters/surface_meter.py:93-112     (SurfaceMeter._evalue: one surface function per batch entry, class)
//   contrastyou/meters/surface_distance.py:11-31   (hausdorff / mod_hausdorff / average_surface over medpy's
//                                                    __surface_distances: a ^ erosion(a), distance_transform_edt)
// Everything up to the square root is integer arithmetic, so the maps are exact; the sums run in a fixed order.
#include "cy_common.h"

// "no border voxel on this line": 2^30 + (CY_SURFACE_MAX_LINE - 1)^2 = 2^30 + 1023^2 stays below 2^31, and every real
// squared distance, at most 3 * 1023^2, stays below it.  A pass never raises a value (j = i is among the candidates).
#define CY_SURFACE_SENTINEL (1 << 30)
#define CY_SURFACE_LINES 8             // adjacent lines a block takes in the H and D passes: 8 * 1024 * 4 = 32 KB of LDS
#define CY_SURFACE_BLOCKS 1024         // cap of the partial-sum grid (blocks of 256 voxels)

namespace {

// border[dir][v] = a(v) && !(every face neighbour in a); what lies outside the volume is background.  dir 0: a = pred,
// dir 1: a = target.  seed[1 - dir][v] = 0 on the border, the sentinel elsewhere: direction `dir` measures from its own
// border voxels to the nearest border voxel of the other volume, so a border seeds the OTHER direction's map.
__global__ void __launch_bounds__(256)
    surface_border_kernel(const int64_t* __restrict__ pred, const int64_t* __restrict__ target, int64_t cls,
                          uint8_t* __restrict__ border0, uint8_t* __restrict__ border1, int32_t* __restrict__ d2_0,
                          int32_t* __restrict__ d2_1, int D, int H, int W, int depth) {
  const int64_t* vol = blockIdx.y ? target : pred;
  uint8_t* border = blockIdx.y ? border1 : border0;
  int32_t* seed = blockIdx.y ? d2_0 : d2_1;
  const int HW = H * W;
  const int V = D * HW;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < V; e += (long)gridDim.x * 256L) {
    const int v = (int)e;
    const int x = v % W, y = (v / W) % H, z = v / HW;
    bool b = false;
    if (vol[v] == cls) {
      bool inside = x > 0 && x < W - 1 && y > 0 && y < H - 1;
      if (depth) inside = inside && z > 0 && z < D - 1;
      if (inside) {
        inside = vol[v - 1] == cls && vol[v + 1] == cls && vol[v - W] == cls && vol[v + W] == cls;
        if (depth) inside = inside && vol[v - HW] == cls && vol[v + HW] == cls;
      }
      b = !inside;
    }
    border[v] = b ? 1 : 0;
    seed[v] = b ? 0 : CY_SURFACE_SENTINEL;
  }
}

// One separable min-plus pass, in place: out[i] = min_j (f[j] + (i - j)^2) along lines of length L.  Element k of line
// (o, n) lives at o * outer_stride + k * line_stride + n, n < inner.  A block stages TL lines with adjacent n in LDS
// (s[k * TL + l]), then every thread takes the minimum over the whole staged line for its outputs.  The block owns its
// lines, so writing back in place after the barrier is safe.  blockIdx.y = direction.
template <int TL>
__global__ void __launch_bounds__(256)
    surface_minplus_kernel(int32_t* __restrict__ d2_0, int32_t* __restrict__ d2_1, int L, int inner, long line_stride,
                           long outer_stride, int chunks_per_outer, long nchunks) {
  extern __shared__ int32_t s[];
  int32_t* d2 = blockIdx.y ? d2_1 : d2_0;
  const int total = L * TL;
  for (long c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const long o = c / chunks_per_outer;
    const int n0 = (int)(c % chunks_per_outer) * TL;
    int32_t* base = d2 + o * outer_stride + n0;
    const int lines = inner - n0 < TL ? inner - n0 : TL;
    for (int e = threadIdx.x; e < total; e += 256) {
      const int l = e % TL, k = e / TL;
      s[e] = l < lines ? base[k * line_stride + l] : CY_SURFACE_SENTINEL;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < total; e += 256) {
      const int l = e % TL, i = e / TL;
      if (l < lines) {
        int32_t m = CY_SURFACE_SENTINEL;
        for (int j = 0; j < L; ++j) {
          const int dj = i - j;
          const int32_t c2 = s[j * TL + l] + dj * dj;
          m = c2 < m ? c2 : m;
        }
        base[i * line_stride + l] = m;
      }
    }
    __syncthreads();
  }
}

struct SurfacePartial {
  double sum;
  int64_t count;
  int32_t maxd2;
  int32_t pad;
};

// over the border voxels of direction blockIdx.y: count, sum of sqrt(d2) in f64, max of d2.  A thread adds its
// grid-strided voxels in order, the block adds its 256 threads by a fixed tree: one partial per block.
__global__ void __launch_bounds__(256)
    surface_gather_kernel(const uint8_t* __restrict__ border0, const uint8_t* __restrict__ border1,
                          const int32_t* __restrict__ d2_0, const int32_t* __restrict__ d2_1,
                          SurfacePartial* __restrict__ partials, int V) {
  __shared__ double s_sum[256];
  __shared__ int64_t s_cnt[256];
  __shared__ int32_t s_max[256];
  const uint8_t* border = blockIdx.y ? border1 : border0;
  const int32_t* d2 = blockIdx.y ? d2_1 : d2_0;
  double sum = 0.0;
  int64_t cnt = 0;
  int32_t mx = 0;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < V; e += (long)gridDim.x * 256L) {
    if (border[e]) {
      const int32_t v = d2[e];
      sum += sqrt((double)v);
      cnt += 1;
      mx = v > mx ? v : mx;
    }
  }
  const int t = threadIdx.x;
  s_sum[t] = sum, s_cnt[t] = cnt, s_max[t] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      s_sum[t] += s_sum[t + o];
      s_cnt[t] += s_cnt[t + o];
      s_max[t] = s_max[t + o] > s_max[t] ? s_max[t + o] : s_max[t];
    }
    __syncthreads();
  }
  if (t == 0) {
    SurfacePartial p;
    p.sum = s_sum[0], p.count = s_cnt[0], p.maxd2 = s_max[0], p.pad = 0;
    partials[blockIdx.y * CY_SURFACE_BLOCKS + blockIdx.x] = p;
  }
}

// the fixed-order final sum: block d (one per direction) adds the nb <= 1024 partials of its direction, thread t the
// partials t, t + 256, ... in order, then the same tree
__global__ void __launch_bounds__(256)
    surface_final_kernel(const SurfacePartial* __restrict__ partials, int nb, int64_t* __restrict__ count,
                         double* __restrict__ sum, int32_t* __restrict__ maxd2, int R, int r) {
  __shared__ double s_sum[256];
  __shared__ int64_t s_cnt[256];
  __shared__ int32_t s_max[256];
  const int t = threadIdx.x;
  const SurfacePartial* p = partials + blockIdx.x * CY_SURFACE_BLOCKS;
  double a = 0.0;
  int64_t c = 0;
  int32_t mx = 0;
  for (int i = t; i < nb; i += 256) {
    a += p[i].sum;
    c += p[i].count;
    mx = p[i].maxd2 > mx ? p[i].maxd2 : mx;
  }
  s_sum[t] = a, s_cnt[t] = c, s_max[t] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      s_sum[t] += s_sum[t + o];
      s_cnt[t] += s_cnt[t + o];
      s_max[t] = s_max[t + o] > s_max[t] ? s_max[t + o] : s_max[t];
    }
    __syncthreads();
  }
  if (t == 0) {
    const int at = blockIdx.x * R + r;
    count[at] = s_cnt[0], sum[at] = s_sum[0], maxd2[at] = s_max[0];
  }
}

inline size_t surface_border_bytes(long V) { return (size_t)((2 * V + 15) / 16 * 16); }

// every refusal of the family, before any launch
inline int surface_check(int D, int H, int W) {
  if (D < 1 || H < 1 || W < 1) return CY_ERR_ARG;
  if ((long)D * H * W > 2147483647L) return CY_ERR_ARG;
  if (D > CY_SURFACE_MAX_LINE || H > CY_SURFACE_MAX_LINE || W > CY_SURFACE_MAX_LINE) return CY_ERR_SHAPE;
  return CY_OK;
}

template <int TL>
inline void launch_minplus(hipStream_t st, int32_t* d2_0, int32_t* d2_1, int L, int inner, long line_stride,
                           long outer_stride, long outer) {
  const int cpo = (inner + TL - 1) / TL;
  const long nchunks = outer * cpo;
  const int grid = (int)(nchunks > 65535 ? 65535 : nchunks);
  hipLaunchKernelGGL(surface_minplus_kernel<TL>, dim3(grid, 2), dim3(256), (size_t)L * TL * sizeof(int32_t), st, d2_0,
                     d2_1, L, inner, line_stride, outer_stride, cpo, nchunks);
}

}  // namespace

extern "C" {

size_t cy_surface_ws_bytes(int D, int H, int W) {
  if (surface_check(D, H, W) != CY_OK) return 0;
  const long V = (long)D * H * W;
  return surface_border_bytes(V) + (size_t)8 * V + (size_t)2 * CY_SURFACE_BLOCKS * sizeof(SurfacePartial);
}

int cy_surface_stats(const int64_t* pred, const int64_t* target, const int32_t* classes, int R, int D, int H, int W,
                     int ndim, int64_t* count, double* sum, int32_t* maxd2, int32_t* d2_maps, uint8_t* border_maps,
                     void* ws, size_t ws_bytes, void* stream) {
  if (!pred || !target || !classes || !count || !sum || !maxd2 || !ws) return CY_ERR_ARG;
  const int rc = surface_check(D, H, W);
  if (rc != CY_OK) return rc;
  if (R < 1 || R > CY_SURFACE_MAX_CLASSES) return CY_ERR_SHAPE;
  if ((ndim != 2 && ndim != 3) || (ndim == 2 && D != 1)) return CY_ERR_SHAPE;
  if (ws_bytes < cy_surface_ws_bytes(D, H, W)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const long V = (long)D * H * W;
  const long HW = (long)H * W;
  uint8_t* ws_border = (uint8_t*)ws;
  int32_t* ws_d2 = (int32_t*)((uint8_t*)ws + surface_border_bytes(V));
  SurfacePartial* partials = (SurfacePartial*)(ws_d2 + 2 * V);
  const int nb = cy_blocks(V, 256, CY_SURFACE_BLOCKS);  // V >= 1 (surface_check)
  for (int r = 0; r < R; ++r) {
    // with map output the passes work in the caller's buffers ([direction][class][voxel]), else in the workspace
    uint8_t* b0 = border_maps ? border_maps + (long)r * V : ws_border;
    uint8_t* b1 = border_maps ? border_maps + ((long)R + r) * V : ws_border + V;
    int32_t* m0 = d2_maps ? d2_maps + (long)r * V : ws_d2;
    int32_t* m1 = d2_maps ? d2_maps + ((long)R + r) * V : ws_d2 + V;
    hipLaunchKernelGGL(surface_border_kernel, dim3(nb, 2), dim3(256), 0, st, pred, target, (int64_t)classes[r], b0, b1,
                       m0, m1, D, H, W, ndim == 3 ? 1 : 0);
    launch_minplus<1>(st, m0, m1, W, 1, 1L, (long)W, (long)D * H);                  // along W: rows
    launch_minplus<CY_SURFACE_LINES>(st, m0, m1, H, W, (long)W, HW, (long)D);       // along H: columns of a slice
    launch_minplus<CY_SURFACE_LINES>(st, m0, m1, D, (int)HW, HW, 0L, 1L);           // along D
    hipLaunchKernelGGL(surface_gather_kernel, dim3(nb, 2), dim3(256), 0, st, b0, b1, m0, m1, partials, (int)V);
    hipLaunchKernelGGL(surface_final_kernel, dim3(2), dim3(256), 0, st, partials, nb, count, sum, maxd2, R, r);
  }
  CY_CHECK_LAUNCH();
  return CY_OK;
}

}  // extern "C"
