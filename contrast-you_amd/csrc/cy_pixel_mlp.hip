// Per-row projector over NHWC rows (DenseProjectionHead without pooling, contrastyou/projectors/heads.py:99-123,
// projectors/nn.py:16-23): y[m] = W2 lrelu(W1 x[r(m)] + b1) + b2 (or W1 x + b1), optionally L2-normalised, with an
// optional row list r(m) = idx[m] so that point evaluation computes the sampled pixels only.
//
// One workgroup (four waves) owns a tile of TM rows (64 for 16-bit storage, 32 for f32) and loops over tiles past the
// workgroup cap.  All products run on the matrix cores through Mma<T> (bf16 / f16 MFMA with f32 accumulation; exact f32
// MFMA for f32 rows).  C, hid and out are zero-padded to multiples of 32 inside the kernel: padded x columns, weight
// rows / columns and biases read as zero, padded rows of the last tile read x = 0 and are never stored.
//
// A product D[row][col] = sum_k A[row][k] B[k][col] takes its A fragments from an LDS tile whose k runs contiguously
// (8 elements = one fragment per lane) and its B fragments either from such a tile or straight from the f32 weights in
// global memory (L2-resident: at most 2 x 256 KB), rounded to the storage type on the way as cy_dense_mfma.h rounds W1.
// Wave w owns the 32-column blocks w and w + 4 of a product for all rows of the tile: 2 x (TM/32) accumulator blocks,
// 64 registers at most, and the hidden and the output accumulators are never live together.
//
// Forward: x tile -> LDS; hidden = lrelu(x W1^T + b1) in f32, rounded ONCE to the storage type into a second LDS tile
// (it never reaches memory); y = hidden W2^T + b2 in registers; the row norm is reduced over the 32 lanes of a
// column block by shuffles and over the waves through LDS in wave order.
//
// Backward: recomputes the hidden tile (kept transposed, [unit][row], as the B operand of dW2; the sign of the
// pre-activation stays in registers as one bit per element), forms dY from (dy, y, inv), then
//   dW2 += dY^T H, db2 += sum dY, dH = (dY W2) * lrelu', dW1 += dH^T x, db1 += sum dH, dx[r(m)] += dH W1.
// dY and dH are rounded to the storage type for their products (f32 rows: nothing is rounded).  The parameter
// gradients of a workgroup accumulate in ITS slab of the workspace -- every slab element is read and written by one
// and the same lane for the whole launch -- and one reduce launch adds the slabs in slab order: no atomics, the same
// bits every run.
#include "cy_conv_tile.h"
#include "cy_reduce.h"

namespace {

constexpr int PM_MAXD = 256;     // fused range of C, hid, out
constexpr int PM_FWD_CAP = 1024; // workgroups of the forward launch; more tiles: the kernel loops
constexpr int PM_BWD_CAP = 256;  // workgroups of the backward launch == partial slabs
constexpr int PM_PAD = 8;        // elements added to every LDS row (16 / 32 bytes: rows 1 apart start in other banks)
constexpr int PM_LDS_MAX = 160 * 1024;

struct PmPlan {
  int form, tm, fwd_wgs, fwd_trips, bwd_wgs, bwd_trips, slabs, lds_fwd, lds_bwd;
  int Cp, Hp, Op, KA;  // padded sizes; pitch of the row-major LDS tiles
  long ntiles;
  size_t slab_floats;
};

inline int pm_plan(long M, int C, int hid, int out, int dtype, PmPlan& P) {
  if (dtype != CY_F32 && dtype != CY_BF16 && dtype != CY_F16) return CY_ERR_DTYPE;
  if (M < 1 || C < 1 || C > PM_MAXD || hid < 0 || hid > PM_MAXD || out < 1 || out > PM_MAXD) return CY_ERR_SHAPE;
  const int esz = dtype == CY_F32 ? 4 : 2;
  P.form = dtype == CY_F32 ? CY_PIXEL_MLP_MFMA32 : CY_PIXEL_MLP_MFMA16;
  P.tm = dtype == CY_F32 ? 32 : 64;
  P.Cp = cy_roundup(C, 32), P.Hp = cy_roundup(hid, 32), P.Op = cy_roundup(out, 32);
  const int mx = P.Cp > P.Hp ? (P.Cp > P.Op ? P.Cp : P.Op) : (P.Hp > P.Op ? P.Hp : P.Op);
  P.KA = mx + PM_PAD;
  P.ntiles = (M + P.tm - 1) / P.tm;
  P.fwd_wgs = (int)(P.ntiles < PM_FWD_CAP ? P.ntiles : PM_FWD_CAP);
  P.fwd_trips = (int)((P.ntiles + P.fwd_wgs - 1) / P.fwd_wgs);
  P.bwd_wgs = (int)(P.ntiles < PM_BWD_CAP ? P.ntiles : PM_BWD_CAP);
  P.bwd_trips = (int)((P.ntiles + P.bwd_wgs - 1) / P.bwd_wgs);
  P.slabs = P.bwd_wgs;
  const int J1p = hid ? P.Hp : P.Op;  // rows of W1
  P.slab_floats = (size_t)J1p * P.Cp + J1p + (hid ? (size_t)P.Op * P.Hp + P.Op : 0);
  const int PT = P.tm + PM_PAD, Dp = P.Hp > P.Op ? P.Hp : P.Op;
  P.lds_fwd = (hid ? 2 : 1) * P.tm * P.KA * esz + 4 * P.tm * 4;
  P.lds_bwd = (P.tm * P.KA + (P.Cp + P.Hp + Dp) * PT) * esz + P.tm * 4;
  return CY_OK;
}

template <typename T> using PmFrag = typename Mma<T>::Frag;

template <typename T> __device__ __forceinline__ PmFrag<T> pm_pack(const float (&f)[8]) {
  PmFrag<T> r;
  if constexpr (sizeof(T) == 2) {
    r.v = __builtin_bit_cast(decltype(r.v), Chunk<T>::pack(f));
  } else {
    r.lo = f32x4{f[0], f[1], f[2], f[3]};
    r.hi = f32x4{f[4], f[5], f[6], f[7]};
  }
  return r;
}

// 8 consecutive elements of an LDS tile (16-byte aligned)
template <typename T> __device__ __forceinline__ PmFrag<T> pm_lds_frag(const T* p) {
  PmFrag<T> r;
  if constexpr (sizeof(T) == 2) {
    r.v = *reinterpret_cast<const decltype(r.v)*>(p);
  } else {
    r.lo = *reinterpret_cast<const f32x4*>(p);
    r.hi = *reinterpret_cast<const f32x4*>(p + 4);
  }
  return r;
}

// B fragment of W [N][K] f32 with k contiguous: column n, k .. k + 7 (k a multiple of 8); outside the matrix: zero
struct PmWk {
  const float* W;
  int N, K, vec;  // vec: K % 8 == 0 and W 16-byte aligned
  template <typename T> __device__ __forceinline__ PmFrag<T> frag(int n, int k) const {
    float f[8];
    if (vec) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
      if (n < N && k < K) {
        a = *reinterpret_cast<const f32x4*>(W + (size_t)n * K + k);
        b = *reinterpret_cast<const f32x4*>(W + (size_t)n * K + k + 4);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) f[i] = a[i], f[4 + i] = b[i];
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) f[i] = (n < N && k + i < K) ? W[(size_t)n * K + k + i] : 0.f;
    }
    return pm_pack<T>(f);
  }
};

// B fragment of W^T: B[k][n] = W[k][n] of W [K][N] f32 (k strided; the 32 lanes of a half read 128 contiguous bytes)
struct PmWt {
  const float* W;
  int N, K;
  template <typename T> __device__ __forceinline__ PmFrag<T> frag(int n, int k) const {
    float f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (n < N && k + i < K) ? W[(size_t)(k + i) * N + n] : 0.f;
    return pm_pack<T>(f);
  }
};

// acc[rb][j] = rows 32 rb .. of the tile x columns 32 (wave + 4 j) ..: sum over k < Kp of sA[row][k] B[k][col]
template <typename T, int NRB, typename BF>
__device__ __forceinline__ void pm_mm(const T* sA, int pitch, int Kp, const BF& B, int ncb, int wave, int lane,
                                      f32x16 (&acc)[NRB][2]) {
  using M = Mma<T>;
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[rb][j][i] = 0.f;
  for (int k0 = 0; k0 < Kp; k0 += 16) {
    PmFrag<T> a[NRB];
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) a[rb] = pm_lds_frag<T>(sA + (rb * 32 + r) * pitch + k0 + 8 * h);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int cb = wave + 4 * j;
      if (cb < ncb) {  // (wave-uniform)
        const PmFrag<T> b = B.template frag<T>(cb * 32 + r, k0 + 8 * h);
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) M::mma(a[rb], b, acc[rb][j]);
      }
    }
  }
}

// row of the tile that accumulator register i of lane half h holds (32x32 MFMA output layout)
__device__ __forceinline__ int pm_acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// slab[row][col] (+)= sum over the tile's rows k of sAt[row][k] sBt[col][k]; 32x32 blocks dealt to the waves in a
// fixed order, so every slab element belongs to one lane for the whole launch
template <typename T, int TM>
__device__ __forceinline__ void pm_dw(const T* sAt, const T* sBt, int nrb, int ncb, float* slab, int ld, bool first,
                                      int wave, int lane) {
  using M = Mma<T>;
  constexpr int PT = TM + PM_PAD;
  const int r = lane & 31, h = lane >> 5;
  for (int b = wave; b < nrb * ncb; b += 4) {
    const int rbk = b / ncb, cbk = b - rbk * ncb;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int k0 = 0; k0 < TM; k0 += 16)
      M::mma(pm_lds_frag<T>(sAt + (rbk * 32 + r) * PT + k0 + 8 * h), pm_lds_frag<T>(sBt + (cbk * 32 + r) * PT + k0 + 8 * h),
             acc);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float* p = slab + (size_t)(rbk * 32 + pm_acc_row(i, h)) * ld + cbk * 32 + r;
      *p = first ? acc[i] : *p + acc[i];
    }
  }
}

// slab[j] (+)= sum over the tile's rows of sAt[j][row]
template <typename T, int TM>
__device__ __forceinline__ void pm_db(const T* sAt, int n, float* slab, bool first) {
  constexpr int PT = TM + PM_PAD;
  for (int j = threadIdx.x; j < n; j += 256) {
    float s = 0.f;
    for (int k = 0; k < TM; ++k) s += to_f32<T>(sAt[j * PT + k]);
    slab[j] = first ? s : slab[j] + s;
  }
}

// x rows m0 .. m0 + TM of the problem -> sX [TM][pitch] (and, TR: sXt [Cp][TM + PAD]); zero outside (M, C)
template <typename T, int TM, bool TR>
__device__ __forceinline__ void pm_stage_x(const T* __restrict__ x, const int32_t* __restrict__ idx, long m0, long M,
                                           int C, int Cp, int ldx, int vec, T* sX, int pitch, T* sXt) {
  constexpr int PT = TM + PM_PAD;
  constexpr int EPC = ElemTr<T>::EPC;
  if (vec) {  // C and ldx multiples of a 16-byte chunk, x 16-byte aligned
    const int cpr = Cp / EPC;
    for (int e = threadIdx.x; e < TM * cpr; e += 256) {
      const int row = e / cpr, c0 = (e - row * cpr) * EPC;
      const long m = m0 + row;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (m < M && c0 < C) v = ld16(x + (size_t)(idx ? (long)idx[m] : m) * ldx + c0);
      st16(sX + row * pitch + c0, v);
      if constexpr (TR) {
        alignas(16) T el[EPC];
        *reinterpret_cast<u32x4*>(el) = v;
#pragma unroll
        for (int i = 0; i < EPC; ++i) sXt[(c0 + i) * PT + row] = el[i];
      }
    }
  } else {
    for (int e = threadIdx.x; e < TM * Cp; e += 256) {
      const int row = e / Cp, c = e - row * Cp;
      const long m = m0 + row;
      T v = from_f32<T>(0.f);
      if (m < M && c < C) v = x[(size_t)(idx ? (long)idx[m] : m) * ldx + c];
      sX[row * pitch + c] = v;
      if constexpr (TR) sXt[c * PT + row] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------ forward
template <typename T>
__global__ void __launch_bounds__(256)
    pixel_mlp_fwd_kernel(const T* __restrict__ x, const int32_t* __restrict__ idx, const float* __restrict__ w1,
                         const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                         float* __restrict__ y, float* __restrict__ inv, long M, long ntiles, int C, int ldx, int hid,
                         int out, int Cp, int Hp, int Op, int KA, float slope, int normalize, int xvec, int w1vec,
                         int w2vec) {
  constexpr int TM = sizeof(T) == 2 ? 64 : 32, NRB = TM / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char pm_smem[];
  T* sX = reinterpret_cast<T*>(pm_smem);
  T* sH = sX + TM * KA;
  float* sRed = reinterpret_cast<float*>(sX + (hid ? 2 : 1) * TM * KA);  // [4][TM]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;

  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long m0 = tile * TM;
    pm_stage_x<T, TM, false>(x, idx, m0, M, C, Cp, ldx, xvec, sX, KA, nullptr);
    __syncthreads();
    f32x16 acc[NRB][2];
    if (hid) {
      pm_mm<T, NRB>(sX, KA, Cp, PmWk{w1, hid, C, w1vec}, Hp >> 5, wave, lane, acc);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = (wave + 4 * j) * 32 + r;
        if (wave + 4 * j < (Hp >> 5)) {
          const float bias = col < hid ? b1[col] : 0.f;
#pragma unroll
          for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const float pre = acc[rb][j][i] + bias;
              sH[(rb * 32 + pm_acc_row(i, h)) * KA + col] = from_f32<T>(pre > 0.f ? pre : slope * pre);
            }
        }
      }
      __syncthreads();
    }
    const float* bo = hid ? b2 : b1;
    if (hid) pm_mm<T, NRB>(sH, KA, Hp, PmWk{w2, out, hid, w2vec}, Op >> 5, wave, lane, acc);
    else pm_mm<T, NRB>(sX, KA, Cp, PmWk{w1, out, C, w1vec}, Op >> 5, wave, lane, acc);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = (wave + 4 * j) * 32 + r;
      const float bias = (wave + 4 * j < (Op >> 5) && col < out) ? bo[col] : 0.f;
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[rb][j][i] += bias;  // (columns past `out`: 0 + 0)
    }
    if (normalize) {
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          float ss = acc[rb][0][i] * acc[rb][0][i] + acc[rb][1][i] * acc[rb][1][i];
#pragma unroll
          for (int o = 16; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);  // the 32 lanes of this half
          if (r == 0) sRed[wave * TM + rb * 32 + pm_acc_row(i, h)] = ss;
        }
      __syncthreads();
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int row = rb * 32 + pm_acc_row(i, h);
          const float ss = ((sRed[row] + sRed[TM + row]) + sRed[2 * TM + row]) + sRed[3 * TM + row];
          const float s = 1.f / fmaxf(sqrtf(ss), 1e-12f);
          acc[rb][0][i] *= s, acc[rb][1][i] *= s;
          if (wave == 0 && r == 0 && m0 + row < M) inv[m0 + row] = s;
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = (wave + 4 * j) * 32 + r;
      if (wave + 4 * j < (Op >> 5) && col < out) {
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const long m = m0 + rb * 32 + pm_acc_row(i, h);
            if (m < M) y[(size_t)m * out + col] = acc[rb][j][i];
          }
      }
    }
    __syncthreads();  // (the tiles and sRed are rewritten by the next trip)
  }
}

// ------------------------------------------------------------------------------------------------ backward
template <typename T>
__global__ void __launch_bounds__(256)
    pixel_mlp_bwd_kernel(const T* __restrict__ x, const int32_t* __restrict__ idx, const float* __restrict__ w1,
                         const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ y,
                         const float* __restrict__ inv, const float* __restrict__ dy, T* __restrict__ dx,
                         float* __restrict__ slabs, size_t slab_floats, int need_dw, long M, long ntiles, int C, int ldx,
                         int hid, int out, int Cp, int Hp, int Op, int KA, float slope, int normalize, int xvec,
                         int w1vec) {
  constexpr int TM = sizeof(T) == 2 ? 64 : 32, NRB = TM / 32, PT = TM + PM_PAD;
  extern __shared__ __attribute__((aligned(16))) unsigned char pm_smem[];
  const int Dp = Hp > Op ? Hp : Op;
  T* sA = reinterpret_cast<T*>(pm_smem);  // [TM][KA]: x, then dY, then dH
  T* sXt = sA + TM * KA;                  // [Cp][PT]
  T* sHt = sXt + Cp * PT;                 // [Hp][PT]
  T* sDt = sHt + Hp * PT;                 // [Dp][PT]: dY^T, then dH^T
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int J1p = hid ? Hp : Op;  // rows of W1 (padded)
  float* slab = slabs + (size_t)blockIdx.x * slab_floats;
  float* s_dw1 = slab;
  float* s_db1 = s_dw1 + (size_t)J1p * Cp;
  float* s_dw2 = s_db1 + J1p;
  float* s_db2 = s_dw2 + (size_t)Op * Hp;

  bool first = true;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long m0 = tile * TM;
    pm_stage_x<T, TM, true>(x, idx, m0, M, C, Cp, ldx, xvec, sA, KA, sXt);
    __syncthreads();
    f32x16 acc[NRB][2];
    uint32_t pos[NRB][2];  // bit i: the pre-activation of accumulator register i is > 0
    if (hid) {
      pm_mm<T, NRB>(sA, KA, Cp, PmWk{w1, hid, C, w1vec}, Hp >> 5, wave, lane, acc);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = (wave + 4 * j) * 32 + r;
        const bool on = wave + 4 * j < (Hp >> 5);
        const float bias = (on && col < hid) ? b1[col] : 0.f;
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) {
          uint32_t bits = 0u;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const float pre = acc[rb][j][i] + bias;
            bits |= (pre > 0.f ? 1u : 0u) << i;
            if (on) sHt[col * PT + rb * 32 + pm_acc_row(i, h)] = from_f32<T>(pre > 0.f ? pre : slope * pre);
          }
          pos[rb][j] = bits;
        }
      }
    }
    __syncthreads();  // x tile read by every wave; hidden tile complete

    // dY -> sA [row][o] and sDt [o][row]; rows past M and columns past `out` are zero
    for (int row = wave; row < TM; row += 4) {
      const long m = m0 + row;
      const bool ok = m < M;
      float dot = 0.f, s = 1.f;
      if (normalize) {
        if (ok)
          for (int o = lane; o < out; o += 64) dot += dy[(size_t)m * out + o] * y[(size_t)m * out + o];
        dot = wave_sum(dot);
        s = ok ? inv[m] : 0.f;
      }
      for (int o = lane; o < Op; o += 64) {
        float v = 0.f;
        if (ok && o < out) {
          v = dy[(size_t)m * out + o];
          if (normalize) v = s * (v - y[(size_t)m * out + o] * dot);
        }
        const T t = from_f32<T>(v);
        sA[row * KA + o] = t;
        sDt[o * PT + row] = t;
      }
    }
    __syncthreads();

    if (hid) {
      if (need_dw) {
        pm_dw<T, TM>(sDt, sHt, Op >> 5, Hp >> 5, s_dw2, Hp, first, wave, lane);
        pm_db<T, TM>(sDt, Op, s_db2, first);
      }
      pm_mm<T, NRB>(sA, KA, Op, PmWt{w2, hid, out}, Hp >> 5, wave, lane, acc);  // dH[row][j] = sum_o dY[row][o] W2[o][j]
      __syncthreads();  // every wave is done with dY and dY^T
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = (wave + 4 * j) * 32 + r;
        if (wave + 4 * j < (Hp >> 5)) {
#pragma unroll
          for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const int row = rb * 32 + pm_acc_row(i, h);
              const T t = from_f32<T>(((pos[rb][j] >> i) & 1u) ? acc[rb][j][i] : slope * acc[rb][j][i]);
              sA[row * KA + col] = t;
              sDt[col * PT + row] = t;
            }
        }
      }
      __syncthreads();
    }
    // sA / sDt hold the gradient at the output of W1 (dH, or dY of the linear head): J1p columns
    if (need_dw) {
      pm_dw<T, TM>(sDt, sXt, J1p >> 5, Cp >> 5, s_dw1, Cp, first, wave, lane);
      pm_db<T, TM>(sDt, J1p, s_db1, first);
    }
    if (dx) {
      pm_mm<T, NRB>(sA, KA, J1p, PmWt{w1, C, hid ? hid : out}, Cp >> 5, wave, lane, acc);  // dx[row][c] = sum_j g[row][j] W1[j][c]
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = (wave + 4 * j) * 32 + r;
        if (wave + 4 * j < (Cp >> 5) && col < C) {
#pragma unroll
          for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const long m = m0 + rb * 32 + pm_acc_row(i, h);
              if (m < M) {
                T* p = dx + (size_t)(idx ? (long)idx[m] : m) * ldx + col;
                *p = from_f32<T>(to_f32<T>(*p) + acc[rb][j][i]);
              }
            }
        }
      }
    }
    first = false;
    __syncthreads();  // (the tiles are rewritten by the next trip)
  }
}

// parameter gradients <- sum over the slabs in slab order (f64 accumulator); one thread per element
__global__ void __launch_bounds__(256)
    pixel_mlp_reduce_kernel(const float* __restrict__ slabs, size_t slab_floats, int nslab, float* __restrict__ dw1,
                            float* __restrict__ db1, float* __restrict__ dw2, float* __restrict__ db2, int accumulate,
                            int C, int Cp, int J1, int J1p, int hid, int Hp, int out, int Op) {
  const long n1 = (long)J1 * C, n2 = n1 + J1, n3 = n2 + (hid ? (long)out * hid : 0), n4 = n3 + (hid ? out : 0);
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n4) return;
  float* dst;
  size_t off;
  if (e < n1) {
    const long j = e / C, c = e - j * C;
    dst = dw1 ? dw1 + e : nullptr, off = (size_t)j * Cp + c;
  } else if (e < n2) {
    dst = db1 ? db1 + (e - n1) : nullptr, off = (size_t)J1p * Cp + (e - n1);
  } else if (e < n3) {
    const long o = (e - n2) / hid, j = (e - n2) - o * hid;
    dst = dw2 ? dw2 + (e - n2) : nullptr, off = (size_t)J1p * Cp + J1p + (size_t)o * Hp + j;
  } else {
    dst = db2 ? db2 + (e - n3) : nullptr, off = (size_t)J1p * Cp + J1p + (size_t)Op * Hp + (e - n3);
  }
  if (!dst) return;
  double s = 0.0;
  for (int k = 0; k < nslab; ++k) s += (double)slabs[(size_t)k * slab_floats + off];
  *dst = accumulate ? *dst + (float)s : (float)s;
}

inline bool pm_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T> inline int pm_xvec(const void* x, int C, int ldx) {
  constexpr int EPC = ElemTr<T>::EPC;
  return C % EPC == 0 && ldx % EPC == 0 && pm_aligned16(x);
}
inline int pm_wvec(const float* w, int K) { return w && K % 8 == 0 && pm_aligned16(w); }

inline bool pm_lds_ok() {
  return cy_lds_limit_once<pixel_mlp_fwd_kernel<float>, pixel_mlp_fwd_kernel<bf16>, pixel_mlp_fwd_kernel<f16>,
                           pixel_mlp_bwd_kernel<float>, pixel_mlp_bwd_kernel<bf16>, pixel_mlp_bwd_kernel<f16>>(PM_LDS_MAX);
}

template <typename T>
int pm_launch_fwd(const PmPlan& P, const void* x, const int32_t* idx, const float* w1, const float* b1, const float* w2,
                  const float* b2, float* y, float* inv, long M, int C, int ldx, int hid, int out, float slope,
                  int normalize, hipStream_t st) {
  hipLaunchKernelGGL(pixel_mlp_fwd_kernel<T>, dim3(P.fwd_wgs), dim3(256), (size_t)P.lds_fwd, st, (const T*)x, idx, w1, b1,
                     w2, b2, y, inv, M, P.ntiles, C, ldx, hid, out, P.Cp, P.Hp, P.Op, P.KA, slope, normalize,
                     pm_xvec<T>(x, C, ldx), pm_wvec(w1, C), pm_wvec(w2, hid));
  CY_CHECK_LAUNCH();
  return CY_OK;
}

template <typename T>
int pm_launch_bwd(const PmPlan& P, const void* x, const int32_t* idx, const float* w1, const float* b1, const float* w2,
                  const float* y, const float* inv, const float* dy, void* dx, float* dw1, float* db1, float* dw2,
                  float* db2, int accumulate, long M, int C, int ldx, int hid, int out, float slope, int normalize,
                  float* ws, hipStream_t st) {
  const int need_dw = (dw1 || db1 || dw2 || db2) ? 1 : 0;
  if (!need_dw && !dx) return CY_OK;
  hipLaunchKernelGGL(pixel_mlp_bwd_kernel<T>, dim3(P.bwd_wgs), dim3(256), (size_t)P.lds_bwd, st, (const T*)x, idx, w1, b1,
                     w2, y, inv, dy, (T*)dx, ws, P.slab_floats, need_dw, M, P.ntiles, C, ldx, hid, out, P.Cp, P.Hp, P.Op,
                     P.KA, slope, normalize, pm_xvec<T>(x, C, ldx) && (!dx || pm_aligned16(dx)), pm_wvec(w1, C));
  CY_CHECK_LAUNCH();
  if (need_dw) {
    const int J1 = hid ? hid : out;
    const long n = (long)J1 * C + J1 + (hid ? (long)out * hid + out : 0);
    hipLaunchKernelGGL(pixel_mlp_reduce_kernel, dim3(cy_cdiv(n, 256)), dim3(256), 0, st, (const float*)ws, P.slab_floats,
                       P.slabs, dw1, db1, dw2, db2, accumulate, C, P.Cp, J1, hid ? P.Hp : P.Op, hid, P.Hp, out, P.Op);
    CY_CHECK_LAUNCH();
  }
  return CY_OK;
}

}  // namespace

extern "C" {

int cy_pixel_mlp_plan(long M, int C, int hid, int out, int dtype, cy_pixel_mlp_plan_t* plan) {
  if (!plan) return CY_ERR_ARG;
  PmPlan P;
  const int rc = pm_plan(M, C, hid, out, dtype, P);
  if (rc != CY_OK) return rc;
  plan->form = P.form, plan->rows_per_tile = P.tm, plan->slabs = P.slabs;
  plan->fwd_grid = P.fwd_wgs, plan->fwd_trips = P.fwd_trips, plan->bwd_grid = P.bwd_wgs, plan->bwd_trips = P.bwd_trips;
  plan->lds_bytes = P.lds_fwd > P.lds_bwd ? P.lds_fwd : P.lds_bwd;
  return CY_OK;
}

int cy_pixel_mlp_fwd(const void* x, const int32_t* idx, const float* w1, const float* b1, const float* w2,
                     const float* b2, float* y, float* inv, long M, int C, int ldx, int hid, int out, float slope,
                     int normalize, int dtype, void* stream) {
  if (!x || !w1 || !b1 || !y || (hid > 0 && (!w2 || !b2)) || (normalize && !inv)) return CY_ERR_ARG;
  PmPlan P;
  const int rc = pm_plan(M, C, hid, out, dtype, P);
  if (rc != CY_OK) return rc;
  if (ldx < C) return CY_ERR_SHAPE;
  if (!pm_lds_ok()) return CY_ERR_LAUNCH;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == CY_F32)
    return pm_launch_fwd<float>(P, x, idx, w1, b1, w2, b2, y, inv, M, C, ldx, hid, out, slope, normalize, st);
  if (dtype == CY_BF16)
    return pm_launch_fwd<bf16>(P, x, idx, w1, b1, w2, b2, y, inv, M, C, ldx, hid, out, slope, normalize, st);
  return pm_launch_fwd<f16>(P, x, idx, w1, b1, w2, b2, y, inv, M, C, ldx, hid, out, slope, normalize, st);
}

size_t cy_pixel_mlp_bwd_ws_bytes(long M, int C, int hid, int out, int dtype) {
  PmPlan P;
  if (pm_plan(M, C, hid, out, dtype, P) != CY_OK) return 0;
  return (size_t)P.slabs * P.slab_floats * sizeof(float);
}

int cy_pixel_mlp_bwd(const void* x, const int32_t* idx, const float* w1, const float* b1, const float* w2,
                     const float* y, const float* inv, const float* dy, void* dx, float* dw1, float* db1, float* dw2,
                     float* db2, int accumulate, long M, int C, int ldx, int hid, int out, float slope, int normalize,
                     int dtype, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !w1 || !b1 || !dy || (hid > 0 && !w2) || (normalize && (!y || !inv))) return CY_ERR_ARG;
  PmPlan P;
  const int rc = pm_plan(M, C, hid, out, dtype, P);
  if (rc != CY_OK) return rc;
  if (ldx < C) return CY_ERR_SHAPE;
  const bool need_dw = dw1 || db1 || dw2 || db2;
  if (need_dw && (!ws || ws_bytes < (size_t)P.slabs * P.slab_floats * sizeof(float))) return CY_ERR_WORKSPACE;
  if (!pm_lds_ok()) return CY_ERR_LAUNCH;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == CY_F32)
    return pm_launch_bwd<float>(P, x, idx, w1, b1, w2, y, inv, dy, dx, dw1, db1, dw2, db2, accumulate, M, C, ldx, hid, out,
                                slope, normalize, (float*)ws, st);
  if (dtype == CY_BF16)
    return pm_launch_bwd<bf16>(P, x, idx, w1, b1, w2, y, inv, dy, dx, dw1, db1, dw2, db2, accumulate, M, C, ldx, hid, out,
                               slope, normalize, (float*)ws, st);
  return pm_launch_bwd<f16>(P, x, idx, w1, b1, w2, y, inv, dy, dx, dw1, db1, dw2, db2, accumulate, M, C, ldx, hid, out,
                            slope, normalize, (float*)ws, st);
}

}  // extern "C"
