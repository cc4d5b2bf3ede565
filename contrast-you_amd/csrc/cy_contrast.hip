// The InfoNCE / SupCon loss and the f32 GEMM under its materialised path.
//   contrastyou/losses/contrastive.py:14-20,31-212  (exp_sim_temperature, SupConLoss1, SelfPacedSupConLoss)
// Everything here is f32: the embedding x embedding similarity and the
// G*P products run on the exact f32 MFMA (v_mfma_f32_32x32x2_f32).
// (The projection head that produces the embeddings is cy_proj_head.hip.)
#include "cy_common.h"
#include "cy_reduce.h"

namespace {

// ---------------------------------------------------------------- sgemm (f32 MFMA)
// C[M][N] = alpha * A[M][K] * op(B).  64x64 block tile, 4 waves each a 32x32
// MFMA accumulator, K staged 16 at a time through LDS.
template <bool BT>
__global__ void __launch_bounds__(256)
    sgemm_kernel(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ C,
                 int M, int N, int K, float alpha) {
  __shared__ float sA[64][17];
  __shared__ float sB[16][65];  // [k][n]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const int i = lane & 31, kk = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  for (int k0 = 0; k0 < K; k0 += 16) {
    __syncthreads();
    // A tile: 64 rows x 16 k
    for (int e = tid; e < 64 * 16; e += 256) {
      const int rr = e >> 4, kc = e & 15;
      const int gm = m0 + rr, gk = k0 + kc;
      sA[rr][kc] = (gm < M && gk < K) ? A[(size_t)gm * K + gk] : 0.f;
    }
    if (BT) {
      for (int e = tid; e < 64 * 16; e += 256) {
        const int nn = e >> 4, kc = e & 15;
        const int gn = n0 + nn, gk = k0 + kc;
        sB[kc][nn] = (gn < N && gk < K) ? B[(size_t)gn * K + gk] : 0.f;
      }
    } else {
      for (int e = tid; e < 64 * 16; e += 256) {
        const int kc = e >> 6, nn = e & 63;
        const int gn = n0 + nn, gk = k0 + kc;
        sB[kc][nn] = (gn < N && gk < K) ? B[(size_t)gk * N + gn] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 16; ks += 2) {
      const float av = sA[wm * 32 + i][ks + kk];
      const float bv = sB[ks + kk][wn * 32 + i];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int row = (reg & 3) + 8 * (reg >> 2) + 4 * kk;
    const int gm = m0 + wm * 32 + row, gn = n0 + wn * 32 + i;
    if (gm < M && gn < N) C[(size_t)gm * N + gn] = alpha * acc[reg];
  }
}

int launch_sgemm(const float* A, const float* B, float* C, int M, int N, int K, float alpha,
                 int b_trans, hipStream_t st) {
  dim3 grid(cy_cdiv(N, 64), cy_cdiv(M, 64));
  if (b_trans)
    hipLaunchKernelGGL(sgemm_kernel<true>, grid, dim3(256), 0, st, A, B, C, M, N, K, alpha);
  else
    hipLaunchKernelGGL(sgemm_kernel<false>, grid, dim3(256), 0, st, A, B, C, M, N, K, alpha);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

// ---------------------------------------------------------------- SupCon
// An explicit mask holds one code per ordered pair (contrastive.py:35-36): 1 positive, 0 negative, anything else
// neither -- such a pair enters no sum at all.  It is read as given, pm[i mod n][j mod n] for the pair (i, j), and
// need not be symmetric: the transposed term of G + G^T reads pm[j mod n][i mod n].
__device__ __forceinline__ bool is_pos(const int32_t* labels, const uint8_t* pm, int n, int i,
                                       int j) {
  const int a = i % n, b = j % n;
  if (labels) return labels[a] == labels[b];
  return pm[(size_t)a * n + b] == 1;
}
// code of the ordered pair (i, j): 1, 0, or > 1 for neither (labels know only 1 and 0)
__device__ __forceinline__ int pair_code(const int32_t* labels, const uint8_t* pm, int n, int i, int j) {
  const int a = i % n, b = j % n;
  if (labels) return labels[a] == labels[b] ? 1 : 0;
  return pm[(size_t)a * n + b];
}

// one wave per row: row max (incl. diagonal), sum_{k!=i, not neither} exp(s-m), sum over positives, count
__global__ void __launch_bounds__(256)
    supcon_rowstats_kernel(const float* __restrict__ S, const int32_t* __restrict__ labels,
                           const uint8_t* __restrict__ pm, float* __restrict__ tmp, int n) {
  const int R = 2 * n;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* sr = S + (size_t)row * R;
  float m = -INFINITY;
  for (int j = lane; j < R; j += 64) m = fmaxf(m, sr[j]);
  m = wave_max(m);
  float l = 0.f, ps = 0.f, cnt = 0.f;
  for (int j = lane; j < R; j += 64) {
    if (j == row) continue;
    const int code = pair_code(labels, pm, n, row, j);
    if (code > 1) continue;
    const float s = sr[j];
    l += expf(s - m);
    if (code == 1) {
      ps += s;
      cnt += 1.f;
    }
  }
  l = wave_sum(l);
  ps = wave_sum(ps);
  cnt = wave_sum(cnt);
  if (lane == 0) {
    tmp[row * 4 + 0] = m;
    tmp[row * 4 + 1] = l;
    tmp[row * 4 + 2] = ps;
    tmp[row * 4 + 3] = cnt;
  }
}

// single block: global max, per-row denominators, mean loss
__global__ void __launch_bounds__(256)
    supcon_finalize_kernel(float* __restrict__ row_stats, float* __restrict__ loss, int R) {
  __shared__ float smax[256];
  __shared__ double ssum[256];
  const int tid = threadIdx.x;
  float m = -INFINITY;
  for (int i = tid; i < R; i += 256) m = fmaxf(m, row_stats[i * 4 + 0]);
  smax[tid] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) smax[tid] = fmaxf(smax[tid], smax[tid + o]);
    __syncthreads();
  }
  const float M = smax[0];
  double acc = 0.0;
  for (int i = tid; i < R; i += 256) {
    const float mi = row_stats[i * 4 + 0], li = row_stats[i * 4 + 1];
    const float ps = row_stats[i * 4 + 2], cnt = row_stats[i * 4 + 3];
    const float Di = li * expf(mi - M) + 1e-16f;
    const float li_loss = ps / cnt - M - logf(Di);  // cnt==0 -> NaN like the reference
    acc += (double)li_loss;
    row_stats[i * 4 + 0] = Di;
    row_stats[i * 4 + 1] = cnt;
    row_stats[i * 4 + 2] = ps;
    row_stats[i * 4 + 3] = M;
  }
  ssum[tid] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) ssum[tid] += ssum[tid + o];
    __syncthreads();
  }
  if (tid == 0) loss[0] = (float)(-ssum[0] / (double)R);
}

// G + G^T with G_ij = -(g/R) [pos_ij/cnt_i - in_ij e_ij/D_i], zero diagonal; in_ij: the pair is in row i's denominator
__global__ void __launch_bounds__(256)
    supcon_gsym_kernel(const float* __restrict__ S, const float* __restrict__ rs,
                       const int32_t* __restrict__ labels, const uint8_t* __restrict__ pm,
                       const float* __restrict__ gscale, float* __restrict__ G, int n) {
  const int R = 2 * n;
  const long total = (long)R * R;
  const float gs = gscale[0] / (float)R;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const int i = (int)(e / R), j = (int)(e % R);
    float v = 0.f;
    if (i != j) {
      const float M = rs[3];
      const float eij = expf(S[e] - M);
      const float Di = rs[i * 4 + 0], Dj = rs[j * 4 + 0];
      const float ci = rs[i * 4 + 1], cj = rs[j * 4 + 1];
      if (labels) {
        const float pos = is_pos(labels, pm, n, i, j) ? 1.f : 0.f;
        v = -gs * (pos * (1.f / ci + 1.f / cj) - eij * (1.f / Di + 1.f / Dj));
      } else {  // explicit mask: the transposed term goes by the code of (j, i)
        const int cij = pair_code(labels, pm, n, i, j), cji = pair_code(labels, pm, n, j, i);
        const float p = (cij == 1 ? 1.f / ci : 0.f) + (cji == 1 ? 1.f / cj : 0.f);
        const float q = (cij <= 1 ? 1.f / Di : 0.f) + (cji <= 1 ? 1.f / Dj : 0.f);
        v = -gs * (p - eij * q);
      }
    }
    G[e] = v;
  }
}

// ---- SupConLoss1(exclude_other_pos=True), contrastyou/losses/contrastive.py:87-91 --------------------------------------
// Per positive pair (i, j) the denominator holds that pair and the negatives only, the negatives' sum rescaled by
// kappa_i = 1 / (neg_i / (pos_i + neg_i) + 1e-4):
//   loss_i = (1 / c_i) sum_{j in pos_i} [ s_ij - log(e_ij + a_i) ],   a_i = kappa_i sum_{k in neg_i} e_ik + 1e-16,  e = exp(s - M)
// with M the global maximum (detached, as in the reference).  On the materialised similarity matrix: row maxima from
// supcon_rowstats_kernel, then one wave per row.  rs[row] = (a_i, c_i, kappa_i T_i / c_i, loss_i), T_i = sum_pos 1 / (e_ij + a_i).
__global__ void __launch_bounds__(256)
    supcon_excl_rows_kernel(const float* __restrict__ S, const int32_t* __restrict__ labels,
                            const uint8_t* __restrict__ pm, const float* __restrict__ tmp, float* __restrict__ rs,
                            float* __restrict__ Mout, int n) {
  const int R = 2 * n;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  float M = -INFINITY;
  for (int i = lane; i < R; i += 64) M = fmaxf(M, tmp[i * 4]);  // (every wave: the row maxima are 4 R bytes)
  M = wave_max(M);
  const float* sr = S + (size_t)row * R;
  float ln = 0.f, cnt = 0.f, nc = 0.f;
  for (int j = lane; j < R; j += 64) {
    if (j == row) continue;
    const int code = pair_code(labels, pm, n, row, j);
    if (code == 1) cnt += 1.f;
    else if (code == 0) ln += expf(sr[j] - M), nc += 1.f;
  }
  ln = wave_sum(ln);
  cnt = wave_sum(cnt);
  nc = wave_sum(nc);
  const float negc = labels ? (float)(R - 1) - cnt : nc;  // (a mask's "neither" pairs are in neither count)
  const float kappa = 1.f / (negc / (cnt + negc) + 1e-4f);
  const float ai = ln * kappa + 1e-16f;
  float T = 0.f, ls = 0.f;
  for (int j = lane; j < R; j += 64) {
    if (j == row || !is_pos(labels, pm, n, row, j)) continue;
    const float sm = sr[j] - M;
    const float d = expf(sm) + ai;
    T += 1.f / d;
    ls += sm - logf(d);
  }
  T = wave_sum(T);
  ls = wave_sum(ls);
  if (lane == 0) {
    rs[row * 4 + 0] = ai;
    rs[row * 4 + 1] = cnt;
    rs[row * 4 + 2] = kappa * T / cnt;
    rs[row * 4 + 3] = ls / cnt;  // cnt == 0 -> NaN like the reference
    if (row == 0) Mout[0] = M;
  }
}

__global__ void __launch_bounds__(256)
    supcon_excl_loss_kernel(float* __restrict__ rs, float* __restrict__ loss, const float* __restrict__ Mptr, int R) {
  __shared__ double ssum[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < R; i += 256) acc += (double)rs[i * 4 + 3];
  ssum[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) ssum[threadIdx.x] += ssum[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    loss[0] = (float)(-ssum[0] / (double)R);
    rs[3] = Mptr[0];  // (where cy_supcon_matrices looks for the shift; row 0's loss term has been summed)
  }
}

// G + G^T with G_ij = -(g/R) d loss_i / d s_ij:  pos: (1/c_i) a_i / (e_ij + a_i);  neg: -e_ij kappa_i T_i / c_i;  neither: 0
__global__ void __launch_bounds__(256)
    supcon_excl_gsym_kernel(const float* __restrict__ S, const float* __restrict__ rs, const float* __restrict__ Mptr,
                            const int32_t* __restrict__ labels, const uint8_t* __restrict__ pm,
                            const float* __restrict__ gscale, float* __restrict__ G, int n) {
  const int R = 2 * n;
  const long total = (long)R * R;
  const float gs = gscale[0] / (float)R;
  const float M = Mptr[0];
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const int i = (int)(e / R), j = (int)(e % R);
    float v = 0.f;
    if (i != j) {
      const float eij = expf(S[e] - M);
      const int cij = pair_code(labels, pm, n, i, j);
      const int cji = labels ? cij : pair_code(labels, pm, n, j, i);  // (mask: the transposed term has its own code)
      const float ai = rs[i * 4 + 0], aj = rs[j * 4 + 0];
      if (cij == 1 && cji == 1) {
        v = -gs * (ai / ((eij + ai) * rs[i * 4 + 1]) + aj / ((eij + aj) * rs[j * 4 + 1]));
      } else if (cij == 0 && cji == 0) {
        v = gs * eij * (rs[i * 4 + 2] + rs[j * 4 + 2]);
      } else {  // the two directions differ, or one is neither (no term)
        const float vi = cij == 1 ? -ai / ((eij + ai) * rs[i * 4 + 1]) : (cij == 0 ? eij * rs[i * 4 + 2] : 0.f);
        const float vj = cji == 1 ? -aj / ((eij + aj) * rs[j * 4 + 1]) : (cji == 0 ? eij * rs[j * 4 + 2] : 0.f);
        v = gs * (vi + vj);
      }
    }
    G[e] = v;
  }
}

__global__ void __launch_bounds__(256)
    supcon_matrices_kernel(const float* __restrict__ S, const float* __restrict__ rs,
                           const int32_t* __restrict__ labels, const uint8_t* __restrict__ pm,
                           float* sl, float* se, float* po, float* ne, int n) {
  const int R = 2 * n;
  const long total = (long)R * R;
  const float M = rs[3];
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const int i = (int)(e / R), j = (int)(e % R);
    const float s = S[e] - M;
    if (sl) sl[e] = s;
    if (se) se[e] = expf(s);
    const int code = pair_code(labels, pm, n, i, j);
    if (po) po[e] = (i != j && code == 1) ? 1.f : 0.f;
    if (ne) ne[e] = (i != j && code == 0) ? 1.f : 0.f;
  }
}

// ---------------------------------------------------------------- SupCon, fused: S never leaves the CU
// The 2n x 2n similarity matrix S = P P^T / t (64 MB at the C5 size of 4096 embeddings) and the gradient
// matrix G of the same size are formed tile by tile in the MFMA accumulators and consumed there:
//   forward   row sums  l_i = sum_{k != i} exp(S_ik - M),  ps_i = sum_{pos} S_ik,  cnt_i   per 64-row block and
//             column split, with the reference's global shift M = max S known beforehand: S_ij <= max(S_ii, S_jj)
//             (Cauchy-Schwarz), so M = max_i |P_i|^2 / t from a row-norm pre-pass -- no online rescaling;
//   backward  dP_i = (1/t) sum_j G_ij P_j with G_ij = -(g/R)[pos_ij (1/c_i + 1/c_j) - e_ij (1/D_i + 1/D_j)]:
//             the S tile is recomputed, turned into the G tile in registers, passed through LDS into operand
//             layout and multiplied with the P_j block that is already resident for the first product.
// Exact f32 MFMA (v_mfma_f32_32x32x2_f32) as before; fixed summation orders (column splits are summed in order
// by the finalize / reduce kernels) => bitwise reproducible.  D <= 256.
constexpr int SC_TM = 64;  // rows / columns of a tile
// LDS image of a 64-row block of P: the k index split by parity, [k & 1][row][k >> 1] with row pitch D/2 + 4 floats
// and the two parity planes 16 floats out of step -- the f32 MFMA takes one k per half-wave (lane >> 5), so a lane's
// operands for four successive k-steps are one ds_read_b128, and a column-wise read (second product of the
// backward pass) alternates planes lane by lane without bank conflicts
__device__ __host__ constexpr int sc_ld2(int D) { return D / 2 + 4; }
__device__ __host__ constexpr int sc_plane(int D) { return SC_TM * sc_ld2(D) + 16; }
__device__ __host__ constexpr int sc_block_floats(int D) { return 2 * sc_plane(D); }
// dynamic LDS of the sweeps below, in bytes.  Forward: the row and the column block, then `extra` floats of the kernel's
// own.  Backward: the two blocks, the G tile [64][65] and `nrow` staged floats per row of the block.
constexpr int SC_MAXD = 256;
constexpr int sc_fwd_lds(int D, int extra) { return (2 * sc_block_floats(D) + extra) * (int)sizeof(float); }
constexpr int sc_bwd_lds(int D, int nrow) {
  return (2 * sc_block_floats(D) + SC_TM * (SC_TM + 1) + SC_TM * nrow) * (int)sizeof(float);
}

__global__ void __launch_bounds__(256)
    supcon_diag_kernel(const float* __restrict__ P, float* __restrict__ diag, int R, int D, float inv_t) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* pr = P + (size_t)row * D;
  float s = 0.f;
  for (int i = lane; i < D; i += 64) s = fmaf(pr[i], pr[i], s);
  s = wave_sum(s);
  if (lane == 0) diag[row] = s * inv_t;
}

__device__ __forceinline__ void sc_stage(const float* __restrict__ P, float* sdst, int r0, int R, int D, int tid) {
  // rows r0 .. r0+63 of P -> the parity-split image (zeros beyond R)
  const int dq = D / 4, ld2 = sc_ld2(D), pl = sc_plane(D);
  for (int e = tid; e < SC_TM * dq; e += 256) {
    const int rr = e / dq, c4 = (e % dq) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r0 + rr < R) v = *reinterpret_cast<const f32x4*>(P + (size_t)(r0 + rr) * D + c4);
    float* d = sdst + rr * ld2 + (c4 >> 1);
    d[0] = v[0], d[1] = v[2];
    d[pl] = v[1], d[pl + 1] = v[3];
  }
}

// S tile (64 x 64) of row block sPi x column block sPj into the four waves' 32x32 accumulators
__device__ __forceinline__ f32x16 sc_tile(const float* sPi, const float* sPj, int D, int wm, int wn, int i, int kk) {
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  const int ld2 = sc_ld2(D), pl = sc_plane(D);
  const float* pa = sPi + kk * pl + (wm * 32 + i) * ld2;
  const float* pb = sPj + kk * pl + (wn * 32 + i) * ld2;
  for (int k4 = 0; k4 < D / 2; k4 += 4) {  // four k-steps per pair of 16-byte reads
    const f32x4 a4 = *reinterpret_cast<const f32x4*>(pa + k4);
    const f32x4 b4 = *reinterpret_cast<const f32x4*>(pb + k4);
#pragma unroll
    for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[q], b4[q], acc, 0, 0, 0);
  }
  return acc;
}

// positives with the row side hoisted out of the column loop: folded index (i mod n) and label per row
struct ScRow {
  int a;    // row mod n (R = 2n: one conditional subtraction, no division)
  int lab;  // label of the row (labels mode)
};
__device__ __forceinline__ ScRow sc_row(const int32_t* labels, int n, int row) {
  ScRow q;
  q.a = row >= n ? row - n : row;
  q.lab = (labels && row < 2 * n) ? labels[q.a] : 0;
  return q;
}
__device__ __forceinline__ bool sc_pos(const ScRow& r, const ScRow& c, const int32_t* labels, const uint8_t* pm, int n) {
  return labels ? r.lab == c.lab : pm[(size_t)r.a * n + c.a] == 1;
}
// explicit mask: the code of the ordered pair (r, c) -- 1 positive, 0 negative, anything else neither.  Callers keep
// `row < R && col < R` in front: beyond R the folded index leaves the n x n mask.
__device__ __forceinline__ int sc_code(const ScRow& r, const ScRow& c, const uint8_t* pm, int n) {
  return pm[(size_t)r.a * n + c.a];
}

// ---- the sweep over the S tiles, one per direction, shared by the fused and the self-paced kernels ----
// Grid (row blocks, column splits), 256 threads: four waves (wm, wn), each the 32x32 accumulator of a quarter tile.
// What a thread is in its block:
struct ScBlock {
  int R, m0;               // rows of S (2n); first row of this block
  int cb0, cb1;            // this split's column blocks [cb0, cb1)
  int tid, wm, wn, i, kk;  // wave row / column in the tile; the lane's column in the wave and its k half
};
__device__ __forceinline__ ScBlock sc_block(int n, int nsplit) {
  ScBlock b;
  b.R = 2 * n;
  b.tid = threadIdx.x;
  const int lane = b.tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(b.tid >> 6);
  b.wm = wave >> 1, b.wn = wave & 1;
  b.i = lane & 31, b.kk = lane >> 5;
  b.m0 = blockIdx.x * SC_TM;
  const int ncb = (b.R + SC_TM - 1) / SC_TM;
  b.cb0 = (ncb * (int)blockIdx.y) / nsplit, b.cb1 = (ncb * ((int)blockIdx.y + 1)) / nsplit;
  return b;
}
// row within the block that accumulator register `reg` of this lane holds (f32 32x32 MFMA layout)
__device__ __forceinline__ int sc_rr(const ScBlock& b, int reg) {
  return b.wm * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * b.kk;
}

// Forward: part[split][R][NV] = per-row sums over the split's columns.  term(reg, a, row, col, v0, v1, v2) adds the
// element with raw accumulator value a (S_ij t) to the first NV sums of its register; it sees live off-diagonal
// elements only.
// LDS: the row block, the column block (reused for the totals at the end), then whatever the caller keeps behind.
template <int NV, class Term>
__device__ __forceinline__ void sc_fwd_sweep(const ScBlock& b, const float* __restrict__ P,
                                             const int32_t* __restrict__ labels, float* sm, float* __restrict__ part,
                                             int n, int D, Term term) {
  float* sPi = sm;
  float* sPj = sm + sc_block_floats(D);
  float* sred = sPj;  // reused at the end: [2 wn][64 rows][NV]
  sc_stage(P, sPi, b.m0, b.R, D, b.tid);
  // the per-register sums, NV <= 3 of them in use.  Three arrays, all three zeroed, and not one [16][NV]: the compiler
  // drops what is unused, and the register allocation depends on the form -- with one array the labels instantiations
  // come out about ten VGPRs lower and on another occupancy step than the measured kernels
  // (profiles/supcon_shared_sweep_ab.txt)
  static_assert(NV >= 1 && NV <= 3);
  float s0[16], s1[16], s2[16];
  auto sum = [&](int reg, int v) -> float& { return v == 0 ? s0[reg] : (v == 1 ? s1[reg] : s2[reg]); };
  ScRow rws[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
#pragma unroll
    for (int v = 0; v < 3; ++v) sum(q, v) = 0.f;
    rws[q] = sc_row(labels, n, b.m0 + sc_rr(b, q));
  }
  for (int cb = b.cb0; cb < b.cb1; ++cb) {
    const int n0 = cb * SC_TM;
    __syncthreads();  // previous tile's reads of sPj are done
    sc_stage(P, sPj, n0, b.R, D, b.tid);
    __syncthreads();
    const f32x16 acc = sc_tile(sPi, sPj, D, b.wm, b.wn, b.i, b.kk);
    const int col = n0 + b.wn * 32 + b.i;
    const ScRow cq = sc_row(labels, n, col);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = b.m0 + sc_rr(b, reg);
      if (row < b.R && col < b.R && row != col) term(reg, acc[reg], rws[reg], cq, s0[reg], s1[reg], s2[reg]);
    }
  }
  // row totals: over the 32 lanes that share kk (fixed xor tree), then over the two column halves (wn)
#pragma unroll
  for (int reg = 0; reg < 16; ++reg)
#pragma unroll
    for (int o = 16; o > 0; o >>= 1)
#pragma unroll
      for (int v = 0; v < NV; ++v) sum(reg, v) += __shfl_xor(sum(reg, v), o, 64);
  __syncthreads();
  if (b.i == 0) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      float* d = sred + (b.wn * SC_TM + sc_rr(b, reg)) * NV;
#pragma unroll
      for (int v = 0; v < NV; ++v) d[v] = sum(reg, v);
    }
  }
  __syncthreads();
  for (int e = b.tid; e < SC_TM * NV; e += 256) {
    const int rr = e / NV;
    if (b.m0 + rr < b.R)
      part[((size_t)blockIdx.y * b.R + b.m0 + rr) * NV + e % NV] = sred[e] + sred[SC_TM * NV + e];
  }
}

// Backward: dpart[split][R][D] = sum over the split's columns of (G_ij + G_ji) P_j.  The S tile is recomputed, turned
// into the G tile element by element, passed through LDS into operand layout and multiplied with the resident P_j.
// Elem supplies  NROW floats staged per row of the block (stage_row),  a Col of per-column values (load_col)  and
// g(a, row, col, staged row, Col) = G_ij + G_ji of a live off-diagonal element with raw accumulator value a.
template <class Elem>
__device__ __forceinline__ void sc_bwd_sweep(const ScBlock& b, const float* __restrict__ P,
                                             const int32_t* __restrict__ labels, float* sm, float* __restrict__ dpart,
                                             int n, int D, Elem elem) {
  constexpr int ldg = SC_TM + 1, NROW = Elem::NROW;
  const int ld2 = sc_ld2(D), pl = sc_plane(D);
  float* sPi = sm;
  float* sPj = sm + sc_block_floats(D);
  float* sG = sPj + sc_block_floats(D);
  float* sRow = sG + SC_TM * ldg;  // [64][NROW]
  sc_stage(P, sPi, b.m0, b.R, D, b.tid);
  if (b.tid < SC_TM) elem.stage_row(sRow + b.tid * NROW, b.m0 + b.tid, b.R);
  const int nct = (D + 31) / 32;          // 32-wide column tiles of dP
  f32x16 acc2[4];                          // this wave's column tiles: wn, wn + 2, wn + 4, wn + 6
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc2[c][q] = 0.f;
  for (int cb = b.cb0; cb < b.cb1; ++cb) {
    const int n0 = cb * SC_TM;
    __syncthreads();  // previous tile: the second product has read sG and sPj
    sc_stage(P, sPj, n0, b.R, D, b.tid);
    __syncthreads();
    const f32x16 acc = sc_tile(sPi, sPj, D, b.wm, b.wn, b.i, b.kk);
    const int col = n0 + b.wn * 32 + b.i;
    const ScRow cq = sc_row(labels, n, col);
    const typename Elem::Col cj = elem.load_col(col, b.R);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int rr = sc_rr(b, reg);
      const int row = b.m0 + rr;
      float v = 0.f;
      if (row < b.R && col < b.R && row != col)
        v = elem.g(acc[reg], sc_row(labels, n, row), cq, sRow + rr * NROW, cj);
      sG[rr * ldg + b.wn * 32 + b.i] = v;
    }
    __syncthreads();
    // dP rows (wm block) += G[64 rows][64 j] * P_j[64 j][D]
    const float* ga = sG + (b.wm * 32 + b.i) * ldg + b.kk;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int ct = b.wn + 2 * c;
      if (ct < nct) {
        const int dcol = ct * 32 + b.i;  // P_j[j][dcol] sits at [dcol & 1][j][dcol >> 1]
        const float* pb = sPj + (dcol & 1) * pl + b.kk * ld2 + (dcol >> 1);
#pragma unroll 8
        for (int js = 0; js < SC_TM; js += 2)
          acc2[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[js], pb[js * ld2], acc2[c], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int ct = b.wn + 2 * c;
    const int dcol = ct * 32 + b.i;
    if (ct < nct && dcol < D) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = b.m0 + sc_rr(b, reg);
        if (row < b.R) dpart[((size_t)blockIdx.y * b.R + row) * D + dcol] = acc2[c][reg];
      }
    }
  }
}

// (l, ps, cnt) of an element.  MASK: positives from the explicit mask's codes (labels == NULL); the labels
// instantiation is the one the training hooks run.
template <bool MASK>
struct FusedFwdTerm {
  const int32_t* labels;
  const uint8_t* pm;
  int n;
  float inv_t, M;
  __device__ __forceinline__ void operator()(int, float a, const ScRow& r, const ScRow& c, float& l, float& ps,
                                             float& cnt) const {
    const float s = a * inv_t;
    if (MASK) {
      const int code = sc_code(r, c, pm, n);
      if (code <= 1) l += expf(s - M);  // (neither: in no sum)
      if (code == 1) {
        ps += s;
        cnt += 1.f;
      }
    } else {
      l += expf(s - M);
      if (sc_pos(r, c, labels, pm, n)) {
        ps += s;
        cnt += 1.f;
      }
    }
  }
};

// part[split][R][3] = (l, ps, cnt) of the split's columns
template <bool MASK>
__global__ void __launch_bounds__(256)
    supcon_fused_fwd_kernel(const float* __restrict__ P, const int32_t* __restrict__ labels,
                            const uint8_t* __restrict__ pm, const float* __restrict__ Mptr,
                            float* __restrict__ part, int n, int D, float inv_t, int nsplit) {
  extern __shared__ float sm[];
  const FusedFwdTerm<MASK> term{labels, pm, n, inv_t, Mptr[0]};
  sc_fwd_sweep<3>(sc_block(n, nsplit), P, labels, sm, part, n, D, term);
}

// single block: M = max diag (grid-wide value for the other kernels), then (after the fused pass) the loss
__global__ void __launch_bounds__(256)
    supcon_max_kernel(const float* __restrict__ diag, float* __restrict__ Mout, int R) {
  __shared__ float smax[256];
  const int tid = threadIdx.x;
  float m = -INFINITY;
  for (int i = tid; i < R; i += 256) m = fmaxf(m, diag[i]);
  smax[tid] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) smax[tid] = fmaxf(smax[tid], smax[tid + o]);
    __syncthreads();
  }
  if (tid == 0) Mout[0] = smax[0];
}

__global__ void __launch_bounds__(256)
    supcon_fused_finalize_kernel(const float* __restrict__ part, const float* __restrict__ Mptr,
                                 float* __restrict__ row_stats, float* __restrict__ loss, int R, int nsplit) {
  __shared__ double ssum[256];
  const int tid = threadIdx.x;
  const float M = Mptr[0];
  double acc = 0.0;
  for (int i = tid; i < R; i += 256) {
    float li = 0.f, ps = 0.f, cnt = 0.f;
    for (int s = 0; s < nsplit; ++s) {
      const float* p = part + ((size_t)s * R + i) * 3;
      li += p[0], ps += p[1], cnt += p[2];
    }
    const float Di = li + 1e-16f;
    acc += (double)(ps / cnt - M - logf(Di));  // cnt == 0 -> NaN like the reference
    row_stats[i * 4 + 0] = Di;
    row_stats[i * 4 + 1] = cnt;
    row_stats[i * 4 + 2] = ps;
    row_stats[i * 4 + 3] = M;
  }
  ssum[tid] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) ssum[tid] += ssum[tid + o];
    __syncthreads();
  }
  if (tid == 0) loss[0] = (float)(-ssum[0] / (double)R);
}

// G_ij + G_ji = -(g/R) [pos_ij/c_i + pos_ji/c_j - e_ij (in_ij/D_i + in_ji/D_j)], the transposed terms by pm[j][i].
// Staged per row: 1/D_i, 1/c_i.  MASK as above.
template <bool MASK>
struct FusedBwdElem {
  static constexpr int NROW = 2;
  struct Col {
    float iD, ic;  // 1/D_j, 1/c_j
  };
  const int32_t* labels;
  const uint8_t* pm;
  const float* rs;
  int n;
  float inv_t, M, gs;
  __device__ __forceinline__ void stage_row(float* d, int row, int R) const {
    d[0] = row < R ? 1.f / rs[row * 4 + 0] : 0.f;
    d[1] = row < R ? 1.f / rs[row * 4 + 1] : 0.f;
  }
  __device__ __forceinline__ Col load_col(int col, int R) const {
    Col c;
    c.iD = col < R ? 1.f / rs[col * 4 + 0] : 0.f;
    c.ic = col < R ? 1.f / rs[col * 4 + 1] : 0.f;
    return c;
  }
  __device__ __forceinline__ float g(float a, const ScRow& rq, const ScRow& cq, const float* ri, const Col& cj) const {
    const float e = expf(a * inv_t - M);
    if (MASK) {
      const int cij = sc_code(rq, cq, pm, n), cji = sc_code(cq, rq, pm, n);
      const float p = (cij == 1 ? ri[1] : 0.f) + (cji == 1 ? cj.ic : 0.f);
      const float q = (cij <= 1 ? ri[0] : 0.f) + (cji <= 1 ? cj.iD : 0.f);
      return -gs * (p - e * q);
    }
    const float pos = sc_pos(rq, cq, labels, pm, n) ? 1.f : 0.f;
    return -gs * (pos * (ri[1] + cj.ic) - e * (ri[0] + cj.iD));
  }
};

template <bool MASK>
__global__ void __launch_bounds__(256)
    supcon_fused_bwd_kernel(const float* __restrict__ P, const int32_t* __restrict__ labels,
                            const uint8_t* __restrict__ pm, const float* __restrict__ rs,
                            const float* __restrict__ gscale, float* __restrict__ dpart, int n, int D,
                            float inv_t, int nsplit) {
  extern __shared__ float sm[];
  const FusedBwdElem<MASK> elem{labels, pm, rs, n, inv_t, rs[3], gscale[0] / (float)(2 * n)};
  sc_bwd_sweep(sc_block(n, nsplit), P, labels, sm, dpart, n, D, elem);
}

__global__ void __launch_bounds__(256)
    supcon_dpart_reduce_kernel(const float* __restrict__ dpart, float* __restrict__ dP, long total, int nsplit,
                               float inv_t) {
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    float s = 0.f;
    for (int k = 0; k < nsplit; ++k) s += dpart[(size_t)k * total + e];
    dP[e] = s * inv_t;
  }
}

inline int sc_nsplit(int R) {
  const int rb = (R + SC_TM - 1) / SC_TM;
  int ns = 256 / rb;
  if (ns > rb) ns = rb;
  if (ns < 1) ns = 1;
  return ns;
}

// ---------------------------------------------------------------- SupCon, self-paced: the fused kernels with weights
// SelfPacedSupConLoss (contrastive.py:103-212): every positive pair carries a constant weight w_ij of its own negative
// log-likelihood l_ij = -llh_ij, llh_ij = (S_ij - M) - log D_i -- hard [l_ij <= gamma], soft max(1 - l_ij / gamma, 0):
//   loss = -(1/R) sum_i (1/c_i) sum_pos w_ij llh_ij,   ratio = sum_pos w_ij / sum_i c_i
// w_ij needs the finished D_i, so the forward runs over the tiles twice: supcon_fused_fwd_kernel for (l, ps, cnt), then
// supcon_sp_fwd_kernel for (sum_pos w llh, sum_pos w); the backward recomputes w from row_stats on both sides of
//   G_ij + G_ji = -(g scale / R) [pos_ij w_ij / c_i + pos_ji w_ji / c_j - e_ij (in_ij W_i / (c_i D_i) + in_ji W_j / (c_j D_j))]
// Same tiles, same exact f32 MFMA, same fixed orders as above.  S_ij is rounded before M is subtracted (no fused
// multiply-add) and llh is formed as (S_ij - M) - log D_i in every kernel: the hard weight is a threshold, forward and
// backward must come down on the same side of it.

// D_i and c_i of a row: the column splits of the first pass summed in order -- the one place this sum is written
__device__ __forceinline__ void sp_row_sums(const float* __restrict__ partA, int R, int nsplit, int row, float& Di,
                                            float& ci) {
  float li = 0.f, cnt = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float* p = partA + ((size_t)s * R + row) * 3;
    li += p[0], cnt += p[2];
  }
  Di = li + 1e-16f;
  ci = cnt;
}

template <bool SOFT>
__device__ __forceinline__ float sp_weight(float llh, float gamma) {
  const float l = -llh;
  return SOFT ? fmaxf(1.f - l / gamma, 0.f) : (l <= gamma ? 1.f : 0.f);
}

// (w llh, w) of a positive element; logD[reg] = log D_i of the row in accumulator register reg
template <bool MASK, bool SOFT>
struct SpFwdTerm {
  const int32_t* labels;
  const uint8_t* pm;
  int n;
  float inv_t, M, gamma;
  float logD[16];
  __device__ __forceinline__ void operator()(int reg, float a, const ScRow& r, const ScRow& c, float& wl, float& wsum,
                                             float&) const {
    const bool pos = MASK ? sc_code(r, c, pm, n) == 1 : sc_pos(r, c, labels, pm, n);
    if (pos) {
      const float llh = (__fmul_rn(a, inv_t) - M) - logD[reg];
      const float w = sp_weight<SOFT>(llh, gamma);
      wl += w * llh;
      wsum += w;
    }
  }
};
constexpr int SP_FWD_LDS_FLOATS = SC_TM;  // behind the two blocks: log D_i of the row block

// partB[split][R][2] = (sum w llh, sum w) over the positives among the split's columns
template <bool MASK, bool SOFT>
__global__ void __launch_bounds__(256)
    supcon_sp_fwd_kernel(const float* __restrict__ P, const int32_t* __restrict__ labels,
                         const uint8_t* __restrict__ pm, const float* __restrict__ Mptr,
                         const float* __restrict__ partA, float* __restrict__ partB, int n, int D, float inv_t,
                         float gamma, int nsplit) {
  extern __shared__ float sm[];
  const ScBlock b = sc_block(n, nsplit);
  float* sLog = sm + 2 * sc_block_floats(D);  // [64]
  if (b.tid < SC_TM) {
    float Di = 1.f, ci = 0.f;
    if (b.m0 + b.tid < b.R) sp_row_sums(partA, b.R, nsplit, b.m0 + b.tid, Di, ci);
    sLog[b.tid] = logf(Di);
  }
  __syncthreads();
  SpFwdTerm<MASK, SOFT> term{labels, pm, n, inv_t, Mptr[0], gamma, {}};
#pragma unroll
  for (int q = 0; q < 16; ++q) term.logD[q] = sLog[sc_rr(b, q)];
  sc_fwd_sweep<2>(b, P, labels, sm, partB, n, D, term);
}

// single block: row_stats[R][4] = (D_i, c_i, W_i, M), aux[4] = (loss, ratio, scale, sum c); rows summed in f64
__global__ void __launch_bounds__(256)
    supcon_sp_finalize_kernel(const float* __restrict__ partA, const float* __restrict__ partB,
                              const float* __restrict__ Mptr, float* __restrict__ row_stats, float* __restrict__ aux,
                              int R, int nsplit, int correct_grad) {
  __shared__ double ssum[3][256];
  const int tid = threadIdx.x;
  const float M = Mptr[0];
  double al = 0.0, aw = 0.0, ac = 0.0;
  for (int i = tid; i < R; i += 256) {
    float Di, ci, wl = 0.f, W = 0.f;
    sp_row_sums(partA, R, nsplit, i, Di, ci);
    for (int s = 0; s < nsplit; ++s) {
      const float* q = partB + ((size_t)s * R + i) * 2;
      wl += q[0], W += q[1];
    }
    al += (double)(wl / ci);  // c_i == 0 -> NaN like the reference
    aw += (double)W;
    ac += (double)ci;
    row_stats[i * 4 + 0] = Di;
    row_stats[i * 4 + 1] = ci;
    row_stats[i * 4 + 2] = W;
    row_stats[i * 4 + 3] = M;
  }
  ssum[0][tid] = al, ssum[1][tid] = aw, ssum[2][tid] = ac;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o)
      for (int k = 0; k < 3; ++k) ssum[k][tid] += ssum[k][tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const double ratio = ssum[1][0] / ssum[2][0];
    const double scale = (correct_grad && ratio > 0.0) ? 1.0 / ratio : 1.0;
    aux[0] = (float)(-ssum[0][0] / (double)R * scale);
    aux[1] = (float)ratio;
    aux[2] = (float)scale;
    aux[3] = (float)ssum[2][0];
  }
}

// G_ij + G_ji as above, the weights recomputed from row_stats on both sides.  Staged per row, and loaded per column:
// W / (c D), 1 / c, log D.
template <bool MASK, bool SOFT>
struct SpBwdElem {
  static constexpr int NROW = 3;
  struct Col {
    float a, ic, lg;
  };
  const int32_t* labels;
  const uint8_t* pm;
  const float* rs;
  int n;
  float inv_t, M, gs, gamma;
  __device__ __forceinline__ Col load_col(int col, int R) const {
    Col c{0.f, 0.f, 0.f};
    if (col < R) {
      const float Dj = rs[col * 4 + 0], cj = rs[col * 4 + 1];
      c.a = rs[col * 4 + 2] / (cj * Dj), c.ic = 1.f / cj, c.lg = logf(Dj);
    }
    return c;
  }
  __device__ __forceinline__ void stage_row(float* d, int row, int R) const {
    const Col c = load_col(row, R);
    d[0] = c.a, d[1] = c.ic, d[2] = c.lg;
  }
  __device__ __forceinline__ float g(float acc, const ScRow& rq, const ScRow& cq, const float* ri, const Col& cj) const {
    const float sl = __fmul_rn(acc, inv_t) - M;
    bool pij, pji, iij = true, iji = true;
    if (MASK) {
      const int cij = sc_code(rq, cq, pm, n), cji = sc_code(cq, rq, pm, n);
      pij = cij == 1, pji = cji == 1, iij = cij <= 1, iji = cji <= 1;
    } else {
      pij = pji = sc_pos(rq, cq, labels, pm, n);
    }
    float p = 0.f;
    if (pij) p += sp_weight<SOFT>(sl - ri[2], gamma) * ri[1];
    if (pji) p += sp_weight<SOFT>(sl - cj.lg, gamma) * cj.ic;
    const float q = (iij ? ri[0] : 0.f) + (iji ? cj.a : 0.f);
    return -gs * (p - expf(sl) * q);
  }
};

// rs = row_stats of the forward, aux[2] = scale
template <bool MASK, bool SOFT>
__global__ void __launch_bounds__(256)
    supcon_sp_bwd_kernel(const float* __restrict__ P, const int32_t* __restrict__ labels,
                         const uint8_t* __restrict__ pm, const float* __restrict__ rs, const float* __restrict__ aux,
                         const float* __restrict__ gscale, float* __restrict__ dpart, int n, int D, float inv_t,
                         float gamma, int nsplit) {
  extern __shared__ float sm[];
  const SpBwdElem<MASK, SOFT> elem{labels, pm, rs, n, inv_t, rs[3], gscale[0] * aux[2] / (float)(2 * n), gamma};
  sc_bwd_sweep(sc_block(n, nsplit), P, labels, sm, dpart, n, D, elem);
}

constexpr int GRID_CAP = 8192;  // blocks of 256 of the elementwise kernels; the rest is their grid-stride loop

// ---- host side of the fused and the self-paced entries ----
// what the tiles take (the self-paced entries check gamma in addition)
inline bool sc_shape_ok(int n, int D, float t) { return n > 0 && D > 0 && D <= SC_MAXD && D % 8 == 0 && t > 0.f; }

// diag[R] + M[4] + forward partials [ns][R][fwd_row_floats] | backward partials [ns][R][D]
inline size_t sc_ws_bytes(int n, int D, int fwd_row_floats) {
  if (n <= 0 || D <= 0) return 0;
  const size_t R = 2 * (size_t)n;
  const size_t ns = (size_t)sc_nsplit((int)R);
  const size_t fwd = ns * R * (size_t)fwd_row_floats, bwd = ns * R * (size_t)D;
  return (R + 4 + (fwd > bwd ? fwd : bwd)) * sizeof(float);
}

// the workspace of that layout, and the launch geometry that goes with it
struct ScWs {
  int R, ns, rb;
  float* diag;  // diag_out if given (written in place: no device-to-device copy afterwards)
  float* Mv;
  float* part;  // (l, ps, cnt) partials of the forward's first pass; dpart of a backward
  ScWs(void* ws, int n, float* diag_out = nullptr) : R(2 * n), ns(sc_nsplit(R)), rb(cy_cdiv(R, SC_TM)) {
    diag = diag_out ? diag_out : (float*)ws;
    Mv = (float*)ws + R;
    part = Mv + 4;
  }
  dim3 grid() const { return dim3(rb, ns); }
};

// first pass of every forward: diag(S), M = max diag, then (l, ps, cnt) per row and column split into w.part
int sc_first_pass(const float* P, const int32_t* labels, const uint8_t* pm, const ScWs& w, int n, int D, float t,
                  hipStream_t st) {
  hipLaunchKernelGGL(supcon_diag_kernel, dim3(cy_cdiv(w.R, 4)), dim3(256), 0, st, P, w.diag, w.R, D, 1.f / t);
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(supcon_max_kernel, dim3(1), dim3(256), 0, st, (const float*)w.diag, w.Mv, w.R);
  CY_CHECK_LAUNCH();
  if (!cy_lds_limit_once<supcon_fused_fwd_kernel<false>, supcon_fused_fwd_kernel<true>>(sc_fwd_lds(SC_MAXD, 0)))
    return CY_ERR_LAUNCH;
  const auto kernel = labels ? supcon_fused_fwd_kernel<false> : supcon_fused_fwd_kernel<true>;
  hipLaunchKernelGGL(kernel, w.grid(), dim3(256), sc_fwd_lds(D, 0), st, P, labels, pm, (const float*)w.Mv, w.part, n, D,
                     1.f / t, w.ns);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

// dP = (1/t) * the column splits of w.part summed in order
int sc_reduce_dpart(const ScWs& w, float* dP, int D, float t, hipStream_t st) {
  const long total = (long)w.R * D;
  hipLaunchKernelGGL(supcon_dpart_reduce_kernel, dim3(cy_blocks(total, 256, GRID_CAP)), dim3(256), 0, st,
                     (const float*)w.part, dP, total, w.ns, 1.f / t);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

}  // namespace

extern "C" {

int cy_sgemm(const float* A, const float* B, float* C, int M, int N, int K, float alpha,
             int b_trans, void* stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0) return CY_ERR_ARG;
  return launch_sgemm(A, B, C, M, N, K, alpha, b_trans, (hipStream_t)stream);
}

int cy_supcon_fwd(const float* P, const int32_t* labels, const uint8_t* pos_mask, float* S,
                  float* loss, float* row_stats, int n, int D, float t, void* stream) {
  if (!P || (!labels && !pos_mask) || !S || !loss || !row_stats) return CY_ERR_ARG;
  if (n <= 0 || D <= 0 || !(t > 0.f)) return CY_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int R = 2 * n;
  int rc = launch_sgemm(P, P, S, R, R, D, 1.f / t, 1, st);
  if (rc != CY_OK) return rc;
  hipLaunchKernelGGL(supcon_rowstats_kernel, dim3(cy_cdiv(R, 4)), dim3(256), 0, st, S, labels,
                     pos_mask, row_stats, n);
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(supcon_finalize_kernel, dim3(1), dim3(256), 0, st, row_stats, loss, R);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_supcon_bwd(const float* P, const int32_t* labels, const uint8_t* pos_mask, const float* S,
                  const float* row_stats, const float* gscale, float* G, float* dP, int n, int D,
                  float t, void* stream) {
  if (!P || (!labels && !pos_mask) || !S || !row_stats || !gscale || !G || !dP) return CY_ERR_ARG;
  if (n <= 0 || D <= 0 || !(t > 0.f)) return CY_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int R = 2 * n;
  hipLaunchKernelGGL(supcon_gsym_kernel, dim3(cy_blocks((long)R * R, 256, GRID_CAP)), dim3(256), 0, st, S,
                     row_stats, labels, pos_mask, gscale, G, n);
  CY_CHECK_LAUNCH();
  return launch_sgemm(G, P, dP, R, D, R, 1.f / t, 0, st);
}

int cy_supcon_excl_fwd(const float* P, const int32_t* labels, const uint8_t* pos_mask, float* S, float* loss,
                       float* row_stats, float* tmp, int n, int D, float t, void* stream) {
  if (!P || (!labels && !pos_mask) || !S || !loss || !row_stats || !tmp) return CY_ERR_ARG;
  if (n <= 0 || D <= 0 || !(t > 0.f)) return CY_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int R = 2 * n;
  int rc = launch_sgemm(P, P, S, R, R, D, 1.f / t, 1, st);
  if (rc != CY_OK) return rc;
  hipLaunchKernelGGL(supcon_rowstats_kernel, dim3(cy_cdiv(R, 4)), dim3(256), 0, st, S, labels, pos_mask, tmp, n);
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(supcon_excl_rows_kernel, dim3(cy_cdiv(R, 4)), dim3(256), 0, st, S, labels, pos_mask, (const float*)tmp,
                     row_stats, tmp + (size_t)4 * R, n);
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(supcon_excl_loss_kernel, dim3(1), dim3(256), 0, st, row_stats, loss, (const float*)(tmp + (size_t)4 * R), R);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_supcon_excl_bwd(const float* P, const int32_t* labels, const uint8_t* pos_mask, const float* S,
                       const float* row_stats, const float* tmp, const float* gscale, float* G, float* dP, int n, int D,
                       float t, void* stream) {
  if (!P || (!labels && !pos_mask) || !S || !row_stats || !tmp || !gscale || !G || !dP) return CY_ERR_ARG;
  if (n <= 0 || D <= 0 || !(t > 0.f)) return CY_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int R = 2 * n;
  hipLaunchKernelGGL(supcon_excl_gsym_kernel, dim3(cy_blocks((long)R * R, 256, GRID_CAP)), dim3(256), 0, st, S,
                     row_stats, tmp + (size_t)4 * R, labels, pos_mask, gscale, G, n);
  CY_CHECK_LAUNCH();
  return launch_sgemm(G, P, dP, R, D, R, 1.f / t, 0, st);
}

size_t cy_supcon_fused_ws_bytes(int n, int D) { return sc_ws_bytes(n, D, 3); }

int cy_supcon_fused_fwd(const float* P, const int32_t* labels, const uint8_t* pos_mask, float* loss,
                        float* row_stats, float* diag_out, void* ws, size_t ws_bytes, int n, int D, float t,
                        void* stream) {
  if (!P || (!labels && !pos_mask) || !loss || !row_stats || !ws) return CY_ERR_ARG;
  if (!sc_shape_ok(n, D, t)) return CY_ERR_SHAPE;
  if (ws_bytes < cy_supcon_fused_ws_bytes(n, D)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const ScWs w(ws, n, diag_out);
  const int rc = sc_first_pass(P, labels, pos_mask, w, n, D, t, st);
  if (rc != CY_OK) return rc;
  hipLaunchKernelGGL(supcon_fused_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)w.part,
                     (const float*)w.Mv, row_stats, loss, w.R, w.ns);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_supcon_fused_bwd(const float* P, const int32_t* labels, const uint8_t* pos_mask, const float* row_stats,
                        const float* gscale, float* dP, void* ws, size_t ws_bytes, int n, int D, float t,
                        void* stream) {
  if (!P || (!labels && !pos_mask) || !row_stats || !gscale || !dP || !ws) return CY_ERR_ARG;
  if (!sc_shape_ok(n, D, t)) return CY_ERR_SHAPE;
  if (ws_bytes < cy_supcon_fused_ws_bytes(n, D)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const ScWs w(ws, n);
  constexpr int NROW = FusedBwdElem<false>::NROW;
  if (!cy_lds_limit_once<supcon_fused_bwd_kernel<false>, supcon_fused_bwd_kernel<true>>(sc_bwd_lds(SC_MAXD, NROW)))
    return CY_ERR_LAUNCH;
  const auto kernel = labels ? supcon_fused_bwd_kernel<false> : supcon_fused_bwd_kernel<true>;
  hipLaunchKernelGGL(kernel, w.grid(), dim3(256), sc_bwd_lds(D, NROW), st, P, labels, pos_mask, row_stats, gscale,
                     w.part, n, D, 1.f / t, w.ns);
  CY_CHECK_LAUNCH();
  return sc_reduce_dpart(w, dP, D, t, st);
}

size_t cy_supcon_sp_ws_bytes(int n, int D) { return sc_ws_bytes(n, D, 3 + 2); }  // the first pass's and (w llh, w)

int cy_supcon_sp_fwd(const float* P, const int32_t* labels, const uint8_t* pos_mask, float* aux, float* row_stats,
                     float* diag_out, void* ws, size_t ws_bytes, int n, int D, float t, float gamma, int soft,
                     int correct_grad, void* stream) {
  if (!P || (!labels && !pos_mask) || !aux || !row_stats || !ws) return CY_ERR_ARG;
  if (!sc_shape_ok(n, D, t) || !(gamma > 0.f)) return CY_ERR_SHAPE;
  if (ws_bytes < cy_supcon_sp_ws_bytes(n, D)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const ScWs w(ws, n, diag_out);
  float* partB = w.part + (size_t)w.ns * w.R * 3;
  if (!cy_lds_limit_once<supcon_sp_fwd_kernel<false, false>, supcon_sp_fwd_kernel<false, true>,
                         supcon_sp_fwd_kernel<true, false>, supcon_sp_fwd_kernel<true, true>>(
          sc_fwd_lds(SC_MAXD, SP_FWD_LDS_FLOATS)))
    return CY_ERR_LAUNCH;
  const int rc = sc_first_pass(P, labels, pos_mask, w, n, D, t, st);
  if (rc != CY_OK) return rc;
  const auto kernel = labels ? (soft ? supcon_sp_fwd_kernel<false, true> : supcon_sp_fwd_kernel<false, false>)
                             : (soft ? supcon_sp_fwd_kernel<true, true> : supcon_sp_fwd_kernel<true, false>);
  hipLaunchKernelGGL(kernel, w.grid(), dim3(256), sc_fwd_lds(D, SP_FWD_LDS_FLOATS), st, P, labels, pos_mask,
                     (const float*)w.Mv, (const float*)w.part, partB, n, D, 1.f / t, gamma, w.ns);
  CY_CHECK_LAUNCH();
  hipLaunchKernelGGL(supcon_sp_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)w.part, (const float*)partB,
                     (const float*)w.Mv, row_stats, aux, w.R, w.ns, correct_grad);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

int cy_supcon_sp_bwd(const float* P, const int32_t* labels, const uint8_t* pos_mask, const float* row_stats,
                     const float* aux, const float* gscale, float* dP, void* ws, size_t ws_bytes, int n, int D, float t,
                     float gamma, int soft, void* stream) {
  if (!P || (!labels && !pos_mask) || !row_stats || !aux || !gscale || !dP || !ws) return CY_ERR_ARG;
  if (!sc_shape_ok(n, D, t) || !(gamma > 0.f)) return CY_ERR_SHAPE;
  if (ws_bytes < cy_supcon_sp_ws_bytes(n, D)) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const ScWs w(ws, n);
  constexpr int NROW = SpBwdElem<false, false>::NROW;
  if (!cy_lds_limit_once<supcon_sp_bwd_kernel<false, false>, supcon_sp_bwd_kernel<false, true>,
                         supcon_sp_bwd_kernel<true, false>, supcon_sp_bwd_kernel<true, true>>(
          sc_bwd_lds(SC_MAXD, NROW)))
    return CY_ERR_LAUNCH;
  const auto kernel = labels ? (soft ? supcon_sp_bwd_kernel<false, true> : supcon_sp_bwd_kernel<false, false>)
                             : (soft ? supcon_sp_bwd_kernel<true, true> : supcon_sp_bwd_kernel<true, false>);
  hipLaunchKernelGGL(kernel, w.grid(), dim3(256), sc_bwd_lds(D, NROW), st, P, labels, pos_mask, row_stats, aux, gscale,
                     w.part, n, D, 1.f / t, gamma, w.ns);
  CY_CHECK_LAUNCH();
  return sc_reduce_dpart(w, dP, D, t, st);
}

int cy_supcon_matrices(const float* S, const float* row_stats, const int32_t* labels,
                       const uint8_t* pos_mask, float* sim_logits, float* sim_exp,
                       float* pos_out, float* neg_out, int n, void* stream) {
  if (!S || !row_stats || (!labels && !pos_mask) || n <= 0) return CY_ERR_ARG;
  const int R = 2 * n;
  hipLaunchKernelGGL(supcon_matrices_kernel, dim3(cy_blocks((long)R * R, 256, GRID_CAP)), dim3(256), 0,
                     (hipStream_t)stream, S, row_stats, labels, pos_mask, sim_logits, sim_exp,
                     pos_out, neg_out, n);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

}  // extern "C"
