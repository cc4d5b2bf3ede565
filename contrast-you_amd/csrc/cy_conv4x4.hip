// The 4 x 4 convolutions of the adversarial baseline's discriminator (contrastyou/arch/discriminator.py:17-43 of the
// reference: nn.Conv2d(Cin, Cout, 4, 2, 1, bias=False) four times, nn.Conv2d(Cin, 1, 4, 1, 0, bias=False) once) as
// implicit GEMMs: f32 storage, NHWC activations, f32 accumulation on v_mfma_f32_32x32x2_f32.  No patch matrix is ever
// written: every kernel gathers the patches from the activation map while it stages its LDS tiles.
//   forward          rows (n, ho, wo) x columns cout, K = (kh, kw, ci); weights packed [Cout][kh][kw][Cin]
//   data gradient    rows = input pixels x columns ci, K = (tap, co); stride 2: the 2 x 2 taps that reach a pixel are
//                    selected by the parities of (h, w), one parity class per blockIdx.z, no scatter and no atomics;
//                    stride 1: all 16 taps.  Weights packed [Cin][kh][kw][Cout]
//   weight gradient  rows cout x columns (kh, kw, ci), summed over the output positions; the positions are split over
//                    blockIdx.z into f32 partials that a second launch adds in ascending order (no floating-point
//                    atomics: two runs give the same bits) and writes as [Cout][Cin][4][4]
// MFMA form (Cout >= 32): 256 threads = 4 waves, every wave owns a 64 x 64 tile = four independent 32 x 32
// accumulators; the block tile is 256 x 64 (narrow column side) or 128 x 128, one LDS stage holds 16 reduction steps,
// stored reduction-major ([k][row], rows padded by 4) so that an operand read is one 4-byte LDS read per lane at
// consecutive addresses; the next stage's global loads are in flight while the current one is multiplied.
// Loads are 16 bytes where the contiguous channel count is a multiple of 4 and the base is 16-byte aligned, 4 bytes
// otherwise; the launcher picks by that rule.  Cout < 32 takes VALU forms (a wave per output position forward, a
// thread per element for the gradients): an MFMA tile would be mostly padding there; so would the data gradient's
// tile for Cin < 32 (its columns are the input channels), which takes the VALU form too -- at stride 2 with Cin <= 8 and
// Cout <= 64 one whose 16 lanes share a pixel's dy row (the first layer).
// Element offsets are 64-bit; pixel counts must fit 31 bits.  Arguments are checked before any launch.
#include <limits.h>

#include "cy_common.h"
#include "cy_reduce.h"

namespace {

constexpr int BK = 16;         // reduction steps per LDS stage
constexpr int PADL = 4;        // row padding of an LDS stage, in floats
constexpr int SMALL_COUT = 32; // below: the VALU forms
constexpr int NARROW_CIN = 8;  // up to here (stride 2, Cout <= 64, Cout % 4 == 0): the 16-lanes-per-pixel data gradient
constexpr int NARROW_BLOCKS = 512;  // per parity class: its weight prologue is paid per block
constexpr int MAX_CH = 1 << 20;
constexpr int WG_ROWS_MFMA = 512, WG_ROWS_SMALL = 64, WG_BLOCKS = 256, WG_SPLITS_MAX = 256;
constexpr int OUTSIDE = INT_MIN / 2;  // a window start that no tap brings into the map

struct Geo {
  int N, H, W, Cin, Ho, Wo, Cout, stride, pad;
  int K;  // 16 * Cin
  int M;  // N * Ho * Wo
};

// ---------------------------------------------------------------- loads of four adjacent reduction columns
// p[base + k .. base + k + 3], zero past `len` or when !ok.  V: one 16-byte load (len % 4 == 0, base % 4 == 0)
template <bool V>
__device__ __forceinline__ f32x4 row4(const float* __restrict__ p, long base, int k, int len, bool ok) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (V) {
    if (ok && k < len) v = *reinterpret_cast<const f32x4*>(p + base + k);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (ok && k + e < len) v[e] = p[base + k + e];
  }
  return v;
}

// patch columns k .. k + 3 (k = (kh * 4 + kw) * Cin + ci) of the output position whose window starts at (hi0, wi0)
// of the image that starts at pixel pix0; zero in the padding
template <bool V>
__device__ __forceinline__ f32x4 patch4(const float* __restrict__ x, const Geo& g, long pix0, int hi0, int wi0,
                                        int k) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (V) {
    if (k < g.K) {
      const int tap = k / g.Cin, ci = k - tap * g.Cin;
      const int hi = hi0 + (tap >> 2), wi = wi0 + (tap & 3);
      if ((unsigned)hi < (unsigned)g.H && (unsigned)wi < (unsigned)g.W)
        v = *reinterpret_cast<const f32x4*>(x + ((pix0 + (long)hi * g.W + wi) * g.Cin + ci));
    }
  } else {
    int tap = k / g.Cin, ci = k - tap * g.Cin;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (tap < 16) {  // k + e < K
        const int hi = hi0 + (tap >> 2), wi = wi0 + (tap & 3);
        if ((unsigned)hi < (unsigned)g.H && (unsigned)wi < (unsigned)g.W)
          v[e] = x[(pix0 + (long)hi * g.W + wi) * g.Cin + ci];
      }
      if (++ci == g.Cin) ci = 0, ++tap;
    }
  }
  return v;
}

// data gradient, A side: columns k .. k + 3 (k = (th * TH + tw) * Cout + co) of an input pixel: dy at output position
// (hb - th, wb - tw) of the image whose outputs start at position out0
template <bool V>
__device__ __forceinline__ f32x4 grad4(const float* __restrict__ dy, const Geo& g, int TH, int Kd, long out0, int hb,
                                       int wb, int k) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  const int sh = TH == 2 ? 1 : 2;
#pragma unroll
  for (int e = 0; e < (V ? 1 : 4); ++e) {
    const int ke = k + e;
    if (ke < Kd) {
      const int t = ke / g.Cout, co = ke - t * g.Cout;
      const int ho = hb - (t >> sh), wo = wb - (t & (TH - 1));
      if ((unsigned)ho < (unsigned)g.Ho && (unsigned)wo < (unsigned)g.Wo) {
        const float* p = dy + ((out0 + (long)ho * g.Wo + wo) * g.Cout + co);
        if (V)
          v = *reinterpret_cast<const f32x4*>(p);
        else
          v[e] = *p;
      }
    }
  }
  return v;
}

// data gradient, B side: the same columns of input channel ci from the weights packed [Cin][kh][kw][Cout]
template <bool V>
__device__ __forceinline__ f32x4 wt4(const float* __restrict__ wt, const Geo& g, int TH, int Kd, int kh0, int kw0,
                                     int ci, int k) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  const int sh = TH == 2 ? 1 : 2;
#pragma unroll
  for (int e = 0; e < (V ? 1 : 4); ++e) {
    const int ke = k + e;
    if (ci < g.Cin && ke < Kd) {
      const int t = ke / g.Cout, co = ke - t * g.Cout;
      const int kh = kh0 + g.stride * (t >> sh), kw = kw0 + g.stride * (t & (TH - 1));
      const float* p = wt + (((long)ci * 16 + kh * 4 + kw) * g.Cout + co);
      if (V)
        v = *reinterpret_cast<const f32x4*>(p);
      else
        v[e] = *p;
    }
  }
  return v;
}

// ---------------------------------------------------------------- the wave's 64 x 64 product of one LDS stage
// As [BK][LDA], Bs [BK][LDB]; lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]
template <int LDA, int LDB>
__device__ __forceinline__ void mma_stage(const float* As, const float* Bs, int wm, int wn, int lane,
                                          f32x16 (&acc)[2][2]) {
  const float* a = As + (lane >> 5) * LDA + wm * 64 + (lane & 31);
  const float* b = Bs + (lane >> 5) * LDB + wn * 64 + (lane & 31);
#pragma unroll
  for (int kk = 0; kk < BK; kk += 2) {
    const float a0 = a[kk * LDA], a1 = a[kk * LDA + 32];
    const float b0 = b[kk * LDB], b1 = b[kk * LDB + 32];
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
  }
}

__device__ __forceinline__ void zero_acc(f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
}

// f(i, j, value) for every element of the wave's tile; C/D map: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2)
// + 4 * (lane >> 5)
template <typename F>
__device__ __forceinline__ void each_acc(const f32x16 (&acc)[2][2], int wm, int wn, int lane, F f) {
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        f(wm * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), wn * 64 + tn * 32 + (lane & 31),
          acc[tm][tn][r]);
}

// four reduction-adjacent values of tile row r into a reduction-major stage
__device__ __forceinline__ void put_t(float* S, int ld, int q, int r, const f32x4& v) {
#pragma unroll
  for (int e = 0; e < 4; ++e) S[(4 * q + e) * ld + r] = v[e];
}

// ---------------------------------------------------------------- forward, MFMA form
template <int WM, int WN, bool VA, bool VB>
__global__ void __launch_bounds__(256)
    fwd_mfma_kernel(const float* __restrict__ x, const float* __restrict__ wp, float* __restrict__ y, Geo g) {
  constexpr int BM = 64 * WM, BN = 64 * WN, LDA = BM + PADL, LDB = BN + PADL;
  __shared__ float As[BK * LDA];
  __shared__ float Bs[BK * LDB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int q = tid & 3, r0 = tid >> 2;
  long pix0[WM];
  int hi0[WM], wi0[WM];
#pragma unroll
  for (int i = 0; i < WM; ++i) {
    const int row = m0 + r0 + 64 * i;
    pix0[i] = 0, hi0[i] = OUTSIDE, wi0[i] = 0;
    if (row < g.M) {
      const int n = row / (g.Ho * g.Wo), rem = row - n * (g.Ho * g.Wo);
      const int ho = rem / g.Wo, wo = rem - ho * g.Wo;
      pix0[i] = (long)n * g.H * g.W, hi0[i] = ho * g.stride - g.pad, wi0[i] = wo * g.stride - g.pad;
    }
  }
  f32x4 ra[WM], rb[WN];
  f32x16 acc[2][2];
  zero_acc(acc);
#define CY_FWD_LOAD(K0)                                                                    \
  do {                                                                                     \
    _Pragma("unroll") for (int i = 0; i < WM; ++i)                                         \
        ra[i] = patch4<VA>(x, g, pix0[i], hi0[i], wi0[i], (K0) + 4 * q);                   \
    _Pragma("unroll") for (int i = 0; i < WN; ++i) {                                       \
      const int c = n0 + r0 + 64 * i;                                                      \
      rb[i] = row4<VB>(wp, (long)c * g.K, (K0) + 4 * q, g.K, c < g.Cout);                  \
    }                                                                                      \
  } while (0)
  CY_FWD_LOAD(0);
  for (int k0 = 0; k0 < g.K; k0 += BK) {
#pragma unroll
    for (int i = 0; i < WM; ++i) put_t(As, LDA, q, r0 + 64 * i, ra[i]);
#pragma unroll
    for (int i = 0; i < WN; ++i) put_t(Bs, LDB, q, r0 + 64 * i, rb[i]);
    __syncthreads();
    if (k0 + BK < g.K) CY_FWD_LOAD(k0 + BK);
    mma_stage<LDA, LDB>(As, Bs, wm, wn, lane, acc);
    __syncthreads();
  }
#undef CY_FWD_LOAD
  each_acc(acc, wm, wn, lane, [&](int i, int j, float v) {
    const int row = m0 + i, c = n0 + j;
    if (row < g.M && c < g.Cout) y[(long)row * g.Cout + c] = v;
  });
}

// ---------------------------------------------------------------- data gradient, MFMA form
template <int WM, int WN, bool V>
__global__ void __launch_bounds__(256)
    dgrad_mfma_kernel(const float* __restrict__ dy, const float* __restrict__ wt, float* __restrict__ dx, Geo g) {
  constexpr int BM = 64 * WM, BN = 64 * WN, LDA = BM + PADL, LDB = BN + PADL;
  __shared__ float As[BK * LDA];
  __shared__ float Bs[BK * LDB];
  __shared__ long rowpix[BM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int q = tid & 3, r0 = tid >> 2;
  const bool s2 = g.stride == 2;
  const int ph = s2 ? (int)(blockIdx.z >> 1) : 0, pw = s2 ? (int)(blockIdx.z & 1) : 0;
  const int Hc = s2 ? (g.H - ph + 1) >> 1 : g.H, Wc = s2 ? (g.W - pw + 1) >> 1 : g.W;
  const int Mc = g.N * Hc * Wc;
  if (m0 >= Mc) return;
  const int TH = s2 ? 2 : 4, Kd = TH * TH * g.Cout;
  const int kh0 = s2 ? 1 - ph : 0, kw0 = s2 ? 1 - pw : 0;
  // pixel (n, h, w) of class row `row`, h = h2 * stride + ph; its taps read dy at (hb - th, wb - tw)
  auto decode = [&](int row, int& n, int& h2, int& w2) {
    n = row / (Hc * Wc);
    const int rem = row - n * (Hc * Wc);
    h2 = rem / Wc, w2 = rem - h2 * Wc;
  };
  if (tid < BM) {
    long p = -1;
    if (m0 + tid < Mc) {
      int n, h2, w2;
      decode(m0 + tid, n, h2, w2);
      p = ((long)n * g.H + (h2 * g.stride + ph)) * g.W + (w2 * g.stride + pw);
    }
    rowpix[tid] = p;
  }
  long out0[WM];
  int hb[WM], wb[WM];
#pragma unroll
  for (int i = 0; i < WM; ++i) {
    const int row = m0 + r0 + 64 * i;
    out0[i] = 0, hb[i] = OUTSIDE, wb[i] = 0;
    if (row < Mc) {
      int n, h2, w2;
      decode(row, n, h2, w2);
      out0[i] = (long)n * g.Ho * g.Wo, hb[i] = s2 ? h2 + ph : h2, wb[i] = s2 ? w2 + pw : w2;
    }
  }
  f32x4 ra[WM], rb[WN];
  f32x16 acc[2][2];
  zero_acc(acc);
#define CY_DG_LOAD(K0)                                                                             \
  do {                                                                                             \
    _Pragma("unroll") for (int i = 0; i < WM; ++i)                                                 \
        ra[i] = grad4<V>(dy, g, TH, Kd, out0[i], hb[i], wb[i], (K0) + 4 * q);                      \
    _Pragma("unroll") for (int i = 0; i < WN; ++i)                                                 \
        rb[i] = wt4<V>(wt, g, TH, Kd, kh0, kw0, n0 + r0 + 64 * i, (K0) + 4 * q);                   \
  } while (0)
  CY_DG_LOAD(0);
  for (int k0 = 0; k0 < Kd; k0 += BK) {
#pragma unroll
    for (int i = 0; i < WM; ++i) put_t(As, LDA, q, r0 + 64 * i, ra[i]);
#pragma unroll
    for (int i = 0; i < WN; ++i) put_t(Bs, LDB, q, r0 + 64 * i, rb[i]);
    __syncthreads();
    if (k0 + BK < Kd) CY_DG_LOAD(k0 + BK);
    mma_stage<LDA, LDB>(As, Bs, wm, wn, lane, acc);
    __syncthreads();
  }
#undef CY_DG_LOAD
  each_acc(acc, wm, wn, lane, [&](int i, int j, float v) {
    const long p = rowpix[i];
    const int c = n0 + j;
    if (p >= 0 && c < g.Cin) dx[p * g.Cin + c] = v;
  });
}

// ---------------------------------------------------------------- weight gradient, MFMA form
// tile 128 (cout) x 128 (patch columns); the reduction runs over the output positions [row_lo, row_hi) of split
// blockIdx.z; both operands are contiguous along their tile index, so a stage is written with 16-byte LDS stores
template <bool VA, bool VB>
__global__ void __launch_bounds__(256)
    wgrad_mfma_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ part, Geo g,
                      int rows_per_split) {
  constexpr int BM = 128, BN = 128, LDA = BM + PADL, LDB = BN + PADL;
  __shared__ __attribute__((aligned(16))) float As[BK * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[BK * LDB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
  const int c4 = tid & 31, rk0 = tid >> 5;  // this thread's stage rows: rk0 and rk0 + 8
  const long lo = (long)blockIdx.z * rows_per_split;
  const int row_lo = (int)(lo < g.M ? lo : g.M);
  const int row_hi = (int)(lo + rows_per_split < g.M ? lo + rows_per_split : g.M);
  const int co = m0 + 4 * c4, k = n0 + 4 * c4;
  f32x4 ra[2], rb[2];
  f32x16 acc[2][2];
  zero_acc(acc);
#define CY_WG_LOAD(R0)                                                                     \
  do {                                                                                     \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                        \
      const int row = (R0) + rk0 + 8 * i;                                                  \
      const bool ok = row < row_hi;                                                        \
      ra[i] = row4<VA>(dy, (long)row * g.Cout, co, g.Cout, ok);                            \
      int n = 0, ho = 0, wo = 0;                                                           \
      if (ok) {                                                                            \
        n = row / (g.Ho * g.Wo);                                                           \
        const int rem = row - n * (g.Ho * g.Wo);                                           \
        ho = rem / g.Wo, wo = rem - ho * g.Wo;                                             \
      }                                                                                    \
      rb[i] = patch4<VB>(x, g, (long)n * g.H * g.W, ok ? ho * g.stride - g.pad : OUTSIDE,  \
                         wo * g.stride - g.pad, k);                                        \
    }                                                                                      \
  } while (0)
  CY_WG_LOAD(row_lo);
  for (int r = row_lo; r < row_hi; r += BK) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<f32x4*>(&As[(rk0 + 8 * i) * LDA + 4 * c4]) = ra[i];
      *reinterpret_cast<f32x4*>(&Bs[(rk0 + 8 * i) * LDB + 4 * c4]) = rb[i];
    }
    __syncthreads();
    if (r + BK < row_hi) CY_WG_LOAD(r + BK);
    mma_stage<LDA, LDB>(As, Bs, wm, wn, lane, acc);
    __syncthreads();
  }
#undef CY_WG_LOAD
  float* out = part + (long)blockIdx.z * g.Cout * g.K;
  each_acc(acc, wm, wn, lane, [&](int i, int j, float v) {
    const int c = m0 + i, kk = n0 + j;
    if (c < g.Cout && kk < g.K) out[(long)c * g.K + kk] = v;
  });
}

// dw[co][ci][kh][kw] = the partials of (co, (kh, kw, ci)) added in ascending split order
__global__ void __launch_bounds__(256)
    wgrad_sum_kernel(const float* __restrict__ part, float* __restrict__ dw, int Cin, int Cout, int splits) {
  const long total = (long)Cout * 16 * Cin;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += part[z * total + e];
    const long c = e / (16 * Cin);
    const int k = (int)(e - c * (16 * Cin)), tap = k / Cin, ci = k - tap * Cin;
    dw[(c * Cin + ci) * 16 + tap] = s;
  }
}

// ---------------------------------------------------------------- Cout < 32: VALU forms
// forward: a wave per output position, the lanes stride over the patch columns (contiguous in NHWC within a kernel row)
template <bool V>
__global__ void __launch_bounds__(256)
    fwd_small_kernel(const float* __restrict__ x, const float* __restrict__ wp, float* __restrict__ y, Geo g) {
  const int lane = threadIdx.x & 63;
  const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (row >= g.M) return;
  const int n = (int)(row / (g.Ho * g.Wo)), rem = (int)(row - (long)n * (g.Ho * g.Wo));
  const int ho = rem / g.Wo, wo = rem - ho * g.Wo;
  const long pix0 = (long)n * g.H * g.W;
  const int hi0 = ho * g.stride - g.pad, wi0 = wo * g.stride - g.pad;
  for (int c = 0; c < g.Cout; ++c) {
    float acc = 0.f;
    for (int k = 4 * lane; k < g.K; k += 256) {
      const f32x4 a = patch4<V>(x, g, pix0, hi0, wi0, k);
      const f32x4 b = row4<V>(wp, (long)c * g.K, k, g.K, true);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = fmaf(a[e], b[e], acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) y[row * g.Cout + c] = acc;
  }
}

// data gradient: a thread per (input pixel, ci); weights packed [Cin][kh][kw][Cout].  Also the form of a narrow input
// (Cin < 32, the first layer): there the MFMA tile's columns, the input channels, would be mostly padding
template <bool V>
__global__ void __launch_bounds__(256)
    dgrad_small_kernel(const float* __restrict__ dy, const float* __restrict__ wt, float* __restrict__ dx, Geo g) {
  const long total = (long)g.N * g.H * g.W * g.Cin;
  const bool s2 = g.stride == 2;
  const int TH = s2 ? 2 : 4;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const long pix = e / g.Cin;
    const int ci = (int)(e - pix * g.Cin);
    const int n = (int)(pix / (g.H * g.W)), rem = (int)(pix - (long)n * (g.H * g.W));
    const int h = rem / g.W, w = rem - h * g.W;
    const int kh0 = s2 ? (h + 1) & 1 : 0, kw0 = s2 ? (w + 1) & 1 : 0;
    const int hb = s2 ? (h + 1 - kh0) >> 1 : h, wb = s2 ? (w + 1 - kw0) >> 1 : w;
    float acc = 0.f;
    for (int th = 0; th < TH; ++th) {
      const int ho = hb - th, kh = kh0 + g.stride * th;
      if ((unsigned)ho >= (unsigned)g.Ho) continue;
      for (int tw = 0; tw < TH; ++tw) {
        const int wo = wb - tw, kw = kw0 + g.stride * tw;
        if ((unsigned)wo >= (unsigned)g.Wo) continue;
        const float* d = dy + (((long)n * g.Ho + ho) * g.Wo + wo) * g.Cout;
        const float* wv = wt + ((long)ci * 16 + kh * 4 + kw) * g.Cout;
        if (V) {
          for (int c = 0; c < g.Cout; c += 4) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(d + c), b = *reinterpret_cast<const f32x4*>(wv + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = fmaf(a[e], b[e], acc);
          }
        } else {
          for (int c = 0; c < g.Cout; ++c) acc = fmaf(d[c], wv[c], acc);
        }
      }
    }
    dx[e] = acc;
  }
}

// data gradient of a narrow input at stride 2 (Cin = CT <= 8, Cout <= 64, Cout % 4 == 0: the first layer).  16 lanes --
// one DPP row -- share an input pixel of parity class blockIdx.y; lane l owns channels 4l .. 4l + 3 of dy, so a pixel's
// dy row is one contiguous read of up to 256 bytes; the class's 2 x 2 taps of the weights stay in registers over the
// grid-stride loop (few blocks: the weight prologue is paid per block); the Cin sums are added across the 16 lanes
// by four DPP steps in a fixed order and lane ci stores channel ci
template <int CTRL>
__device__ __forceinline__ float dpp_read(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_read<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v += dpp_read<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v += dpp_read<0x141>(v);  // row_half_mirror
  v += dpp_read<0x140>(v);  // row_mirror
  return v;
}

template <int CT>
__global__ void __launch_bounds__(256)
    dgrad_narrow_kernel(const float* __restrict__ dy, const float* __restrict__ wt, float* __restrict__ dx, Geo g) {
  const int ph = (int)(blockIdx.y >> 1), pw = (int)(blockIdx.y & 1);
  const int Hc = (g.H - ph + 1) >> 1, Wc = (g.W - pw + 1) >> 1;
  const long Mc = (long)g.N * Hc * Wc;
  const int kh0 = 1 - ph, kw0 = 1 - pw;
  const int l16 = threadIdx.x & 15, c = 4 * l16;
  const bool lane_on = c < g.Cout;
  f32x4 wreg[4][CT];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int ci = 0; ci < CT; ++ci) {
      wreg[t][ci] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (lane_on)
        wreg[t][ci] = *reinterpret_cast<const f32x4*>(
            wt + ((long)ci * 16 + (kh0 + 2 * (t >> 1)) * 4 + kw0 + 2 * (t & 1)) * g.Cout + c);
    }
  for (long row = blockIdx.x * 16L + (threadIdx.x >> 4); row < Mc; row += (long)gridDim.x * 16L) {
    const int r = (int)row, n = r / (Hc * Wc), rem = r - n * (Hc * Wc);
    const int h2 = rem / Wc, w2 = rem - h2 * Wc;
    float acc[CT];
#pragma unroll
    for (int ci = 0; ci < CT; ++ci) acc[ci] = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int ho = h2 + ph - (t >> 1), wo = w2 + pw - (t & 1);
      if (lane_on && (unsigned)ho < (unsigned)g.Ho && (unsigned)wo < (unsigned)g.Wo) {
        const f32x4 a =
            *reinterpret_cast<const f32x4*>(dy + (((long)n * g.Ho + ho) * g.Wo + wo) * g.Cout + c);
#pragma unroll
        for (int ci = 0; ci < CT; ++ci)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[ci] = fmaf(a[e], wreg[t][ci][e], acc[ci]);
      }
    }
    float mine = 0.f;
#pragma unroll
    for (int ci = 0; ci < CT; ++ci) {
      const float v = row16_sum(acc[ci]);
      if (l16 == ci) mine = v;
    }
    if (l16 < CT) dx[(((long)n * g.H + (2 * h2 + ph)) * g.W + (2 * w2 + pw)) * CT + l16] = mine;
  }
}

// weight gradient: a thread per (co, patch column), the output positions of split blockIdx.y in ascending order
__global__ void __launch_bounds__(256)
    wgrad_small_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ part, Geo g,
                       int rows_per_split) {
  const int total = g.Cout * g.K;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int c = e / g.K, k = e - c * g.K, tap = k / g.Cin, ci = k - tap * g.Cin, kh = tap >> 2, kw = tap & 3;
  const long lo = (long)blockIdx.y * rows_per_split;
  const int row_lo = (int)(lo < g.M ? lo : g.M);
  const int row_hi = (int)(lo + rows_per_split < g.M ? lo + rows_per_split : g.M);
  float acc = 0.f;
  if (row_lo < row_hi) {
    int n = row_lo / (g.Ho * g.Wo), rem = row_lo - n * (g.Ho * g.Wo);
    int ho = rem / g.Wo, wo = rem - ho * g.Wo;
    for (int row = row_lo; row < row_hi; ++row) {
      const int hi = ho * g.stride - g.pad + kh, wi = wo * g.stride - g.pad + kw;
      if ((unsigned)hi < (unsigned)g.H && (unsigned)wi < (unsigned)g.W)
        acc = fmaf(dy[(long)row * g.Cout + c], x[(((long)n * g.H + hi) * g.W + wi) * g.Cin + ci], acc);
      if (++wo == g.Wo) {
        wo = 0;
        if (++ho == g.Ho) ho = 0, ++n;
      }
    }
  }
  part[(long)blockIdx.y * total + e] = acc;
}

// [Cout][Cin][4][4] -> [Cout][kh][kw][Cin] (transposed == 0) or [Cin][kh][kw][Cout] (transposed != 0)
__global__ void __launch_bounds__(256)
    pack_kernel(const float* __restrict__ w, float* __restrict__ out, int Cin, int Cout, int transposed) {
  const long total = (long)Cout * Cin * 16;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    int co, ci, tap;
    if (transposed) {
      co = (int)(e % Cout);
      const long t = e / Cout;
      tap = (int)(t & 15), ci = (int)(t >> 4);
    } else {
      ci = (int)(e % Cin);
      const long t = e / Cin;
      tap = (int)(t & 15), co = (int)(t >> 4);
    }
    out[e] = w[((long)co * Cin + ci) * 16 + tap];
  }
}

// ---------------------------------------------------------------- host side
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

constexpr long FLAT_GRID_CAP = 1L << 20;  // blocks of 256 of the pack / sum kernels; the rest is grid-stride

int make_geo(int N, int H, int W, int Cin, int Cout, int ksize, int stride, int pad, Geo* g) {
  if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || ksize < 1 || stride < 1 || pad < 0) return CY_ERR_ARG;
  if (Cin > MAX_CH || Cout > MAX_CH) return CY_ERR_ARG;
  if (!(ksize == 4 && ((stride == 2 && pad == 1) || (stride == 1 && pad == 0)))) return CY_ERR_SHAPE;
  if (H + 2 * pad < 4 || W + 2 * pad < 4) return CY_ERR_SHAPE;
  if ((long)N * H * W > INT_MAX) return CY_ERR_ARG;  // pixel indices are 32-bit (element offsets are 64-bit)
  g->N = N, g->H = H, g->W = W, g->Cin = Cin, g->Cout = Cout, g->stride = stride, g->pad = pad;
  g->Ho = (H + 2 * pad - 4) / stride + 1, g->Wo = (W + 2 * pad - 4) / stride + 1;
  g->K = 16 * Cin;
  g->M = N * g->Ho * g->Wo;
  return CY_OK;
}

int wgrad_splits(const Geo& g) {
  const bool small = g.Cout < SMALL_COUT;
  const long tiles = small ? cy_cdiv((long)g.Cout * g.K, 256) : (long)cy_cdiv(g.Cout, 128) * cy_cdiv(g.K, 128);
  long s = cy_cdiv(WG_BLOCKS, tiles);
  const long by_rows = cy_cdiv(g.M, small ? WG_ROWS_SMALL : WG_ROWS_MFMA);
  if (s > by_rows) s = by_rows;
  if (s > WG_SPLITS_MAX) s = WG_SPLITS_MAX;
  return (int)(s < 1 ? 1 : s);
}

template <int WM, int WN>
void launch_fwd(bool va, bool vb, dim3 grid, hipStream_t st, const float* x, const float* wp, float* y, const Geo& g) {
  if (va && vb)
    hipLaunchKernelGGL((fwd_mfma_kernel<WM, WN, true, true>), grid, dim3(256), 0, st, x, wp, y, g);
  else if (vb)
    hipLaunchKernelGGL((fwd_mfma_kernel<WM, WN, false, true>), grid, dim3(256), 0, st, x, wp, y, g);
  else if (va)
    hipLaunchKernelGGL((fwd_mfma_kernel<WM, WN, true, false>), grid, dim3(256), 0, st, x, wp, y, g);
  else
    hipLaunchKernelGGL((fwd_mfma_kernel<WM, WN, false, false>), grid, dim3(256), 0, st, x, wp, y, g);
}

template <int WM, int WN>
void launch_dgrad(bool v, dim3 grid, hipStream_t st, const float* dy, const float* wt, float* dx, const Geo& g) {
  if (v)
    hipLaunchKernelGGL((dgrad_mfma_kernel<WM, WN, true>), grid, dim3(256), 0, st, dy, wt, dx, g);
  else
    hipLaunchKernelGGL((dgrad_mfma_kernel<WM, WN, false>), grid, dim3(256), 0, st, dy, wt, dx, g);
}

}  // namespace

extern "C" {

int cy_conv4x4_pack_weights(const float* w, float* packed, int Cin, int Cout, int transposed, void* stream) {
  if (!w || !packed || Cin < 1 || Cout < 1 || Cin > MAX_CH || Cout > MAX_CH) return CY_ERR_ARG;
  hipLaunchKernelGGL(pack_kernel, dim3(cy_blocks((long)Cout * Cin * 16, 256, FLAT_GRID_CAP)), dim3(256), 0,
                     (hipStream_t)stream, w, packed, Cin, Cout, transposed);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_conv4x4_fwd(const float* x, const float* wp, float* y, int N, int H, int W, int Cin, int Cout, int ksize,
                   int stride, int pad, void* stream) {
  if (!x || !wp || !y) return CY_ERR_ARG;
  Geo g;
  const int rc = make_geo(N, H, W, Cin, Cout, ksize, stride, pad, &g);
  if (rc != CY_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool va = Cin % 4 == 0 && aligned16(x), vb = aligned16(wp);
  if (Cout < SMALL_COUT) {
    if (va && vb)
      hipLaunchKernelGGL(fwd_small_kernel<true>, dim3(cy_cdiv(g.M, 4)), dim3(256), 0, st, x, wp, y, g);
    else
      hipLaunchKernelGGL(fwd_small_kernel<false>, dim3(cy_cdiv(g.M, 4)), dim3(256), 0, st, x, wp, y, g);
  } else if (Cout <= 64) {
    launch_fwd<4, 1>(va, vb, dim3(cy_cdiv(g.M, 256), 1), st, x, wp, y, g);
  } else {
    launch_fwd<2, 2>(va, vb, dim3(cy_cdiv(g.M, 128), cy_cdiv(Cout, 128)), st, x, wp, y, g);
  }
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_conv4x4_dgrad(const float* dy, const float* wpt, float* dx, int N, int H, int W, int Cin, int Cout, int ksize,
                     int stride, int pad, void* stream) {
  if (!dy || !wpt || !dx) return CY_ERR_ARG;
  Geo g;
  const int rc = make_geo(N, H, W, Cin, Cout, ksize, stride, pad, &g);
  if (rc != CY_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool v = Cout % 4 == 0 && aligned16(dy) && aligned16(wpt);
  if (v && stride == 2 && Cin <= NARROW_CIN && Cout <= 64) {
    const long rows = (long)N * ((H + 1) / 2) * ((W + 1) / 2);  // of the largest parity class, 16 per block pass
    const long want = (rows + 15) / 16;
    const dim3 grid((unsigned)(want < NARROW_BLOCKS ? want : NARROW_BLOCKS), 4);
#define CY_NARROW(CT)                                                                                   \
  case CT:                                                                                              \
    hipLaunchKernelGGL(dgrad_narrow_kernel<CT>, grid, dim3(256), 0, st, dy, wpt, dx, g);                \
    break;
    switch (Cin) {
      CY_NARROW(1) CY_NARROW(2) CY_NARROW(3) CY_NARROW(4) CY_NARROW(5) CY_NARROW(6) CY_NARROW(7) CY_NARROW(8)
    }
#undef CY_NARROW
  } else if (Cout < SMALL_COUT || Cin < SMALL_COUT) {
    const dim3 grid(cy_blocks((long)N * H * W * Cin, 256, FLAT_GRID_CAP));
    if (v)
      hipLaunchKernelGGL(dgrad_small_kernel<true>, grid, dim3(256), 0, st, dy, wpt, dx, g);
    else
      hipLaunchKernelGGL(dgrad_small_kernel<false>, grid, dim3(256), 0, st, dy, wpt, dx, g);
  } else {
    const long rows = stride == 2 ? (long)N * ((H + 1) / 2) * ((W + 1) / 2) : (long)N * H * W;
    const unsigned classes = stride == 2 ? 4 : 1;
    if (Cin <= 64)
      launch_dgrad<4, 1>(v, dim3(cy_cdiv(rows, 256), 1, classes), st, dy, wpt, dx, g);
    else
      launch_dgrad<2, 2>(v, dim3(cy_cdiv(rows, 128), cy_cdiv(Cin, 128), classes), st, dy, wpt, dx, g);
  }
  CY_CHECK_LAUNCH();
  return CY_OK;
}

size_t cy_conv4x4_wgrad_ws_bytes(int N, int H, int W, int Cin, int Cout, int ksize, int stride, int pad) {
  Geo g;
  if (make_geo(N, H, W, Cin, Cout, ksize, stride, pad, &g) != CY_OK) return 0;
  return sizeof(float) * (size_t)wgrad_splits(g) * (size_t)Cout * (size_t)g.K;
}

int cy_conv4x4_wgrad(const float* x, const float* dy, float* dw, int N, int H, int W, int Cin, int Cout, int ksize,
                     int stride, int pad, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !dy || !dw || !ws) return CY_ERR_ARG;
  Geo g;
  const int rc = make_geo(N, H, W, Cin, Cout, ksize, stride, pad, &g);
  if (rc != CY_OK) return rc;
  const int splits = wgrad_splits(g);
  if (ws_bytes < sizeof(float) * (size_t)splits * (size_t)Cout * (size_t)g.K) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  if (Cout < SMALL_COUT) {
    const int rps = cy_cdiv(g.M, splits);
    hipLaunchKernelGGL(wgrad_small_kernel, dim3(cy_cdiv((long)Cout * g.K, 256), splits), dim3(256), 0, st, x, dy, part,
                       g, rps);
  } else {
    const int rps = cy_roundup(cy_cdiv(g.M, splits), BK);
    const bool va = Cout % 4 == 0 && aligned16(dy), vb = Cin % 4 == 0 && aligned16(x);
    const dim3 grid(cy_cdiv(g.K, 128), cy_cdiv(Cout, 128), splits);
    if (va && vb)
      hipLaunchKernelGGL((wgrad_mfma_kernel<true, true>), grid, dim3(256), 0, st, x, dy, part, g, rps);
    else if (va)
      hipLaunchKernelGGL((wgrad_mfma_kernel<true, false>), grid, dim3(256), 0, st, x, dy, part, g, rps);
    else if (vb)
      hipLaunchKernelGGL((wgrad_mfma_kernel<false, true>), grid, dim3(256), 0, st, x, dy, part, g, rps);
    else
      hipLaunchKernelGGL((wgrad_mfma_kernel<false, false>), grid, dim3(256), 0, st, x, dy, part, g, rps);
  }
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(wgrad_sum_kernel, dim3(cy_blocks((long)Cout * g.K, 256, FLAT_GRID_CAP)), dim3(256), 0, st, part,
                     dw, Cin, Cout, splits);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

}  // extern "C"
