// Streamed matrix-core form of the dense projector for 16-bit feature maps with C = 256 or 512 channels and 128 or 256
// hidden units: `Up_conv5` at max_channel 512, `Up_conv5` / `Up_conv4` at max_channel 1024 (14 x 14 and 28 x 28 maps).
// The forward and the dx product: same jobs, same job -> wave assignment and same rounding points as the
// register-resident kernels of cy_dense_mfma.h, whose job records and g tiles they reuse.  (dW1 / db1 of these maps stay
// on the VALU kernel of cy_dense.hip: a streamed dW1 kernel was built and is held back, DESIGN.md says why.)  Two things
// differ, because CB = C / 32 = 8 or 16 channel blocks fit neither in registers nor in a static LDS image:
//
//   rows   The pre-activation accumulator of a block of 32 pixels -- 128 hidden units, 64 registers -- stays in
//          registers while the pixel rows STREAM through a window of DPW_WIN channel blocks (16 registers), two windows
//          in flight: the loads of window w + 1 are issued before the MFMAs of window w, the last window of a block
//          requests the first window of the next block (or of the wave's next job).  Rows past the job's end are turned
//          into zeros when they are used, not when they are loaded, so no wait sits between a load and the MFMAs it
//          overlaps.
//   W1     rounded to the storage type, as a DYNAMIC LDS image [channel block][hidden unit][32 channels] of the hidden
//          units of ONE pass, behind the per-wave tiles (no static __shared__ in front of it):
//            forward: 128 units per pass -> CB x 8 KB = 64 KB (C = 256) or 128 KB (C = 512); a workgroup works on
//              pass blockIdx.x % (hid / 128), so 256 hidden units are two passes over the pixels.
//            dx: the contraction runs over ALL hidden units, 128 at a time through the g tile with the channel stream
//              repeated per 128 units, so the image holds every unit: hid x C x 2 bytes behind 32 KB of g tiles --
//              96 KB (256, 128), 160 KB (256, 256) and (512, 128).  (512, 256) would be 288 KB: there the fragments are
//              read from a 16-bit image of W1 in the workspace (one more small launch writes it), through L2.
//          The limit of dynamic LDS is raised with hipFuncSetAttribute in front of EVERY launch that needs it: the call
//          is host-side and cheap, and a per-process flag would be wrong on a second device.
//
// As in the register-resident form the second product of the dx kernel is done for one block of 32 channels per
// launch (`cbs`), each launch recomputing the pre-activations: CB dx launches (x 4 colour classes with a bin list).  Jobs are bins
// (forward, bin list) or cells of the bin partition (all bins); a job's pixels are walked 32 at a time, so a 2 x 2 bin
// of a 28 x 28 map fills an eighth of its MFMA block -- accepted, see DESIGN.md.
#pragma once
#include "cy_dense_mfma.h"

namespace {

constexpr int DPW_WIN = 2;                // channel blocks per window of rows
constexpr int DPW_HB = 4;                 // 32-unit blocks of hidden units per pass (forward) / per g tile (dx)
constexpr int DPW_GT = 4 * 128 * 64;      // dx kernel: four g tiles
constexpr int DPW_LDS_MAX = 160 * 1024;

template <typename T> struct DpwRows {
  const T* p;  // this lane's pixel row (channel 8h of block 0)
  bool ok;     // false: past the job's last pixel, reads as zero
};

struct DpwWin {
  u32x4 f[DPW_WIN][2];
  bool ok;
};

template <typename T>
__device__ __forceinline__ DpwRows<T> dpw_rows(const T* __restrict__ x, long pix0, int npx, int bw, float inv_bw, int W,
                                               int ldx, int blk, int r, int h) {
  const int q = blk * 32 + r;
  DpwRows<T> P;
  P.ok = q < npx;
  const int qc = P.ok ? q : 0;
  const int qr = (int)(((float)qc + 0.5f) * inv_bw), qcol = qc - qr * bw;
  P.p = x + (pix0 + (long)qr * W + qcol) * ldx + 8 * h;
  return P;
}
template <typename T>
__device__ __forceinline__ DpwRows<T> dpw_rows(const T* __restrict__ x, const DpRec& R, int W, int ldx, int blk, int r,
                                               int h) {
  return dpw_rows<T>(x, R.pix0, R.npx, R.bw, R.inv_bw, W, ldx, blk, r, h);
}

template <typename T> __device__ __forceinline__ void dpw_load(const DpwRows<T>& P, int cb0, DpwWin& w) {
#pragma unroll
  for (int k = 0; k < DPW_WIN; ++k) {
    w.f[k][0] = ld16(P.p + 32 * (cb0 + k));
    w.f[k][1] = ld16(P.p + 32 * (cb0 + k) + 16);
  }
  w.ok = P.ok;
}

// W1 rows [o0, o0 + rows) rounded to T as the image [cb][rows][64 bytes] (dpm_xoff swizzle); thread `tid` of `nthr`
template <typename T>
__device__ __forceinline__ void dpw_stage_w(const float* __restrict__ w1, int CB, int o0, int rows, unsigned char* img,
                                            int tid, int nthr) {
  const int per = CB * 4, C = CB * 32;
  for (int idx = tid; idx < rows * per; idx += nthr) {
    const int row = idx / per, rem = idx - row * per;
    const int cb = rem >> 2, slot = rem & 3;
    const float* src = w1 + (size_t)(o0 + row) * C + cb * 32 + slot * 8;
    float f[8];
    const f32x4 a = *reinterpret_cast<const f32x4*>(src);
    const f32x4 b = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = a[i], f[4 + i] = b[i];
    st16(img + (size_t)cb * (rows * 64) + dpm_xoff(row, slot), Chunk<T>::pack(f));
  }
}

// (the dx kernel of 512 channels x 256 hidden units reads this image from the workspace)
template <typename T>
__global__ void __launch_bounds__(256)
    dpw_round_w_kernel(const float* __restrict__ w1, int CB, int hid, unsigned char* __restrict__ img) {
  dpw_stage_w<T>(w1, CB, 0, hid, img, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// acc[hb] += (32 pixel rows) x (hidden units of block hb)^T over all CB channel blocks.  On entry A holds window 0 of
// `cur`, on exit window 0 of `nxt`.  wimg: the image of dpw_stage_w at hidden block 0 of this pass, `img` bytes per
// channel block.
template <typename T, int CB>
__device__ __forceinline__ void dpw_preact(const DpwRows<T>& cur, const DpwRows<T>& nxt, DpwWin& A, DpwWin& B,
                                           const unsigned char* wimg, int img, const int (&woff)[2],
                                           f32x16 (&acc)[DPW_HB]) {
  using M = Mma<T>;
  constexpr int NS = CB / DPW_WIN;
  static_assert(NS % 2 == 0, "two windows per trip");
  auto mm = [&](const DpwWin& w, int cb0) {
#pragma unroll
    for (int k = 0; k < DPW_WIN; ++k) {
      const u32x4 zero = {0u, 0u, 0u, 0u};
      const u32x4 v0 = w.ok ? w.f[k][0] : zero, v1 = w.ok ? w.f[k][1] : zero;
      const unsigned char* wb = wimg + (size_t)(cb0 + k) * img;
#pragma unroll
      for (int hb = 0; hb < DPW_HB; ++hb) {
        M::mma(dpm_frag<T>(v0), dpm_frag<T>(ld16(wb + woff[0] + hb * 2048)), acc[hb]);
        M::mma(dpm_frag<T>(v1), dpm_frag<T>(ld16(wb + woff[1] + hb * 2048)), acc[hb]);
      }
    }
  };
#pragma unroll
  for (int s = 0; s < NS; s += 2) {
    dpw_load<T>(cur, (s + 1) * DPW_WIN, B);
    mm(A, s * DPW_WIN);
    __builtin_amdgcn_sched_barrier(0);  // (bounds the rows in flight to the two windows)
    if (s + 2 < NS) dpw_load<T>(cur, (s + 2) * DPW_WIN, A);
    else dpw_load<T>(nxt, 0, A);
    mm(B, (s + 1) * DPW_WIN);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ------------------------------------------------------------------------------------------------ forward
template <typename T, int CB>
__global__ void __launch_bounds__(256, 2)
    dense_proj_wide_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w1, const float* __restrict__ b1,
                               const int32_t* __restrict__ bins, int nb, float* __restrict__ hpool, int H, int W,
                               int ldx, int hid, int sh, int sw, float slope) {
  constexpr int HB = DPW_HB;
  extern __shared__ __attribute__((aligned(16))) unsigned char dpw_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int npass = hid / (32 * HB);
  const int pass = blockIdx.x % npass, o0 = pass * HB * 32;
  const int slot = (blockIdx.x / npass) * 4 + wave, nslot = (gridDim.x / npass) * 4;

  dpw_stage_w<T>(w1, CB, o0, 32 * HB, dpw_lds, threadIdx.x, 256);
  __syncthreads();
  int woff[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) woff[ks] = dpm_xoff(r, 2 * ks + h);
  float bias[HB], sbias[HB], lbias[HB];
#pragma unroll
  for (int hb = 0; hb < HB; ++hb) {
    bias[hb] = b1[o0 + hb * 32 + r];
    sbias[hb] = slope * bias[hb];
    lbias[hb] = fmaxf(bias[hb], sbias[hb]);
  }

  DpRun cur = dpm_run<false>(bins, slot, nb, sh, sw, H, W, -1);
  DpwRows<T> rows = dpw_rows<T>(x, cur.pix0, cur.J.npx, cur.J.bw, cur.inv_bw, W, ldx, 0, r, h);
  DpwWin A, B;
  dpw_load<T>(rows, 0, A);
  for (int b = slot; b < nb; b += nslot) {
    const DpRun nxt = dpm_run<false>(bins, b + nslot, nb, sh, sw, H, W, -1);
    const int nblk = cur.nblk;  // (>= 1: a bin is never empty)
    float sum[HB];
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) sum[hb] = 0.f;
    for (int blk = 0; blk < nblk; ++blk) {
      const DpwRows<T> nrows =
          blk + 1 < nblk ? dpw_rows<T>(x, cur.pix0, cur.J.npx, cur.J.bw, cur.inv_bw, W, ldx, blk + 1, r, h)
                         : dpw_rows<T>(x, nxt.pix0, nxt.J.npx, nxt.J.bw, nxt.inv_bw, W, ldx, 0, r, h);
      f32x16 acc[HB];
#pragma unroll
      for (int hb = 0; hb < HB; ++hb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[hb][i] = 0.f;
      dpw_preact<T, CB>(rows, nrows, A, B, dpw_lds, 32 * HB * 64, woff, acc);
#pragma unroll
      for (int hb = 0; hb < HB; ++hb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float v = acc[hb][i];  // lrelu(t) = max(t, slope * t) for slope <= 1
          sum[hb] += fmaxf(v + bias[hb], fmaf(slope, v, sbias[hb]));
        }
      rows = nrows;
    }
    const float npad = (float)(nblk * 32 - cur.J.npx);
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) {
      float s = sum[hb] + __shfl_xor(sum[hb], 32, 64);
      s -= npad * lbias[hb];
      if (h == 0) hpool[(size_t)b * hid + o0 + hb * 32 + r] = s * cur.J.inv[0];
    }
    cur = nxt;
  }
}

// ------------------------------------------------------------------------------------------------ backward
// dx of channel block `cbs`: the dx kernel of cy_dense_mfma.h with streamed rows; the channel stream is repeated for
// every 128 hidden units.  GW: the pre-activations' W1 fragments come from the 16-bit image `wglob` in memory.
// LDS: [4 g tiles][W1 image of all hidden units (not GW)].
template <typename T, int NHB, bool CELLS, int CB, bool GW>
__global__ void __launch_bounds__(256, GW ? 1 : 2)
    dense_proj_wide_dx_kernel(const T* __restrict__ x, const float* __restrict__ w1, const float* __restrict__ b1,
                              const DpRec* __restrict__ recs, int njobs, const float* __restrict__ dhpool,
                              T* __restrict__ dx, const unsigned char* __restrict__ wglob, int W, int ldx, int hid,
                              float slope, int colour, int cbs) {
  using M = Mma<T>;
  constexpr int HB = DPW_HB;
  extern __shared__ __attribute__((aligned(16))) unsigned char dpw_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int gsel = (lane >> 4) & 1, q4 = (lane & 15) >> 2, p4 = lane & 3;
  const int gw = blockIdx.x * 4 + wave, nw = gridDim.x * 4;
  unsigned char* sg = dpw_lds + wave * (128 * 64);
  const unsigned char* wimg;
  if constexpr (GW) {
    wimg = wglob;
  } else {
    dpw_stage_w<T>(w1, CB, 0, 32 * NHB, dpw_lds + DPW_GT, threadIdx.x, 256);
    __syncthreads();
    wimg = dpw_lds + DPW_GT;
  }
  int woff[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) woff[ks] = dpm_xoff(r, 2 * ks + h);
  DpFrag<T> wt[NHB * 2];  // dx: A operand, row = channel r of block cbs, k = hidden unit 16t + 8h + i
  float nbias[NHB];
#pragma unroll
  for (int hb = 0; hb < NHB; ++hb) nbias[hb] = -b1[hb * 32 + r];
#pragma unroll
  for (int t = 0; t < NHB * 2; ++t) {
    float f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = w1[(size_t)(16 * t + 8 * h + i) * (32 * CB) + cbs * 32 + r];
    wt[t] = dpm_frag<T>(Chunk<T>::pack(f));
  }
  // transposed reads of the g tile (cy_dense_mfma.h): two variants (t even / odd) + t * 1024 bytes
  int glo[2], ghi[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int rl = 16 * t + 8 * h + q4, rh = rl + 4;
    glo[t] = dpm_goff(rl, 4 * gsel + p4) - t * 1024;
    ghi[t] = dpm_goff(rh, 4 * gsel + p4) - t * 1024;
  }

  DpRec cur = dpm_rec(recs, gw, njobs, colour);
  DpwRows<T> rows = dpw_rows<T>(x, cur, W, ldx, 0, r, h);
  DpwWin A, B;
  dpw_load<T>(rows, 0, A);
  for (int job = gw; job < njobs; job += nw) {
    float dpos[NHB];
#pragma unroll
    for (int hb = 0; hb < NHB; ++hb) dpos[hb] = dpm_rec_coef(dhpool, cur, hid, hb * 32 + r);
    const DpRec nxt = dpm_rec(recs, job + nw, njobs, colour);
    const int nblk = cur.nblk;
    for (int blk = 0; blk < nblk; ++blk) {
      const DpwRows<T> nrows = blk + 1 < nblk ? dpw_rows<T>(x, cur, W, ldx, blk + 1, r, h) : dpw_rows<T>(x, nxt, W, ldx, 0, r, h);
      f32x16 dxa;
#pragma unroll
      for (int i = 0; i < 16; ++i) dxa[i] = 0.f;
      const unsigned char* wblk = wimg;
      if constexpr (GW) {
        // (the image in memory never changes, so its 256 fragment loads are loop-invariant: left visible, they are all
        //  hoisted out of the block loop and spilled.  An offset the optimiser cannot see through keeps them per block.)
        int opaque = 0;
        asm volatile("" : "+s"(opaque));
        wblk += opaque;
      }
#pragma unroll
      for (int hq = 0; hq < NHB / HB; ++hq) {  // 128 hidden units through the g tile at a time
        f32x16 acc[HB];
#pragma unroll
        for (int hb = 0; hb < HB; ++hb)
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[hb][i] = 0.f;
        dpw_preact<T, CB>(rows, hq + 1 < NHB / HB ? rows : nrows, A, B, wblk + hq * (HB * 2048), 32 * NHB * 64, woff, acc);
#pragma unroll
        for (int k = 0; k < HB; ++k) {
          const float dp = dpos[hq * HB + k], dn = slope * dp, bs = nbias[hq * HB + k];
          float g[16];
#pragma unroll
          for (int i = 0; i < 16; ++i) g[i] = acc[k][i] > bs ? dp : dn;  // pre = acc + b1 > 0
          const u32x4 lo = Chunk<T>::pack(g), hi = Chunk<T>::pack(g + 8);
          // registers 4j .. 4j+3 = pixels 8j + 4h + 0..3 of hidden unit row: 8-byte slot 2j + h
          const int row = k * 32 + r;
          *reinterpret_cast<u32x2*>(sg + dpm_goff(row, 0 + h)) = u32x2{lo[0], lo[1]};
          *reinterpret_cast<u32x2*>(sg + dpm_goff(row, 2 + h)) = u32x2{lo[2], lo[3]};
          *reinterpret_cast<u32x2*>(sg + dpm_goff(row, 4 + h)) = u32x2{hi[0], hi[1]};
          *reinterpret_cast<u32x2*>(sg + dpm_goff(row, 6 + h)) = u32x2{hi[2], hi[3]};
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const DpFrag<T> gt = dpm_tr_frag<T>(sg + glo[t & 1] + t * 1024, sg + ghi[t & 1] + t * 1024);
          M::mma(wt[hq * 8 + t], gt, dxa);
        }
        __builtin_amdgcn_wave_barrier();
      }
      // lane (pixel r of the block, half h): channels 8j + 4h + 0..3 in registers 4j .. 4j+3
      const int q = blk * 32 + r;
      if (q < cur.npx) {
        const int qr = (int)(((float)q + 0.5f) * cur.inv_bw), qcol = q - qr * cur.bw;
        T* p = dx + (cur.pix0 + (long)qr * W + qcol) * ldx + cbs * 32 + 4 * h;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          T pk[4];
          if constexpr (CELLS) {
#pragma unroll
            for (int e = 0; e < 4; ++e) pk[e] = from_f32<T>(dxa[4 * j + e]);
          } else {
            const u32x2 old = *reinterpret_cast<const u32x2*>(p + 8 * j);
            float fo[8];
            Chunk<T>::unpack(u32x4{old[0], old[1], 0u, 0u}, fo);
#pragma unroll
            for (int e = 0; e < 4; ++e) pk[e] = from_f32<T>(fo[e] + dxa[4 * j + e]);
          }
          *reinterpret_cast<u32x2*>(p + 8 * j) = __builtin_bit_cast(u32x2, *reinterpret_cast<const s16x4*>(pk));
        }
      }
      rows = nrows;
    }
    if (nblk == 0) {  // an empty cell, or a bin of another colour class: A still holds its (unused) window
      rows = dpw_rows<T>(x, nxt, W, ldx, 0, r, h);
      dpw_load<T>(rows, 0, A);
    }
    cur = nxt;
  }
}

// ------------------------------------------------------------------------------------------------ launch plan
inline bool dpm_enabled() {
  static const bool on = [] {
    const char* e = getenv("CY_DENSE_MFMA");
    return !(e && e[0] == '0');
  }();
  return on;
}

// what cy_dense_proj_plan reports and the three entry points follow
struct DpPlan {
  int form;                     // CY_DENSE_PROJ_*
  int cb;                       // channel blocks of 32 (VALU: staged chunks)
  int fwd_pass, dw_pass;        // passes over the hidden units: forward, dW1 kernel (the dx kernel always makes one)
  int lds_fwd, lds_dx;          // dynamic LDS bytes
  int w_global;                 // 1: the dx kernel reads W1 from a 16-bit image in the workspace
};

inline int dp_plan(int C, int hid, int dtype, float slope, DpPlan& P) {
  if (C <= 0 || C % 8 || hid <= 0) return CY_ERR_SHAPE;
  if (dtype != CY_F32 && dtype != CY_BF16 && dtype != CY_F16) return CY_ERR_DTYPE;
  P = DpPlan{CY_DENSE_PROJ_VALU, cy_cdiv(C, DP_CB), 1, 1, 0, 0, 0};
  // (slope <= 1: the forward kernels form lrelu as max(t, slope * t))
  if (!dpm_enabled() || dtype == CY_F32 || !(hid == 128 || hid == 256) || !(slope <= 1.f)) return CY_OK;
  if (C == 32 || C == 64 || C == 128) {
    P.form = CY_DENSE_PROJ_MFMA_REG;
    P.cb = C / 32;
    P.fwd_pass = C == 128 ? hid / 64 : C == 64 ? hid / 128 : 1;  // (dpm_launch_fwd_cb)
    P.dw_pass = hid / 128;
  } else if (C == 256 || C == 512) {
    P.form = CY_DENSE_PROJ_MFMA_STREAM;
    P.cb = C / 32;
    P.fwd_pass = hid / (32 * DPW_HB);  // (dW1 / db1: the VALU kernel, one pass)
    P.lds_fwd = P.cb * 32 * DPW_HB * 64;
    P.lds_dx = DPW_GT + hid * C * 2;
    if (P.lds_dx > DPW_LDS_MAX) P.lds_dx = DPW_GT, P.w_global = 1;
  }
  return CY_OK;
}

// launches of one backward that asks for dx and the parameter gradients
inline int dp_plan_launches(const DpPlan& P, bool list) {
  if (P.form == CY_DENSE_PROJ_VALU) return 6;  // dW1, four colour classes of dx, the slab sum
  if (P.form == CY_DENSE_PROJ_MFMA_STREAM)  // VALU dW1 + slab sum, job table, W1 image, dx per channel block (and colour)
    return 3 + P.w_global + P.cb * (list ? 4 : 1);
  return 1 + P.cb * (2 + (list ? 4 : 1));
}

inline size_t dp_wide_image_bytes(int C, int hid) { return (size_t)hid * C * 2; }

template <typename K> inline bool dpw_lds_limit(K kern, int bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
}

// persistent workgroups: two per CU while two fit in LDS
inline int dpw_wgs(int lds) { return 2 * lds <= DPW_LDS_MAX ? DPM_WGS : DPM_WGS / 2; }

template <typename T, int CB>
int dpw_launch_fwd(const DpPlan& P, const T* x, const float* w1, const float* b1, const int32_t* bins, int nb, float* hpool,
                   int H, int W, int ldx, int hid, int sh, int sw, float slope, hipStream_t st) {
  const auto kern = dense_proj_wide_fwd_kernel<T, CB>;
  if (!dpw_lds_limit(kern, P.lds_fwd)) return CY_ERR_LAUNCH;
  const int per = cy_cdiv(nb, 4), cap = dpw_wgs(P.lds_fwd) / P.fwd_pass;
  const int grid = (per < cap ? per : cap) * P.fwd_pass;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), (size_t)P.lds_fwd, st, x, w1, b1, bins, nb, hpool, H, W, ldx, hid, sh, sw,
                     slope);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

template <typename T, int NHB, bool CELLS, int CB>
int dpw_launch_dx(const DpPlan& P, const T* x, const float* w1, const float* b1, const DpRec* recs, int njobs,
                  const float* dhpool, T* dx, const unsigned char* wglob, int W, int ldx, int hid, float slope, int colour,
                  int cbs, hipStream_t st) {
  constexpr bool GW = DPW_GT + NHB * 32 * CB * 32 * 2 > DPW_LDS_MAX;
  if (GW != (P.w_global != 0)) return CY_ERR_LAUNCH;
  const auto kern = dense_proj_wide_dx_kernel<T, NHB, CELLS, CB, GW>;
  if (!dpw_lds_limit(kern, P.lds_dx)) return CY_ERR_LAUNCH;
  const int cap = GW ? DPM_WGS / 2 : dpw_wgs(P.lds_dx);  // (GW: 272-280 registers, one workgroup per CU)
  const int grid = njobs < cap * 4 ? cy_cdiv(njobs, 4) : cap;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), (size_t)P.lds_dx, st, x, w1, b1, recs, njobs, dhpool, dx, wglob, W, ldx,
                     hid, slope, colour, cbs);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

// dx of the streamed form (dW1 / db1 are the caller's: the VALU kernel).  Workspace as the register-resident form lays
// it out: [DPM_WGS partials (unused here)][job records (< 4 nb)][16-bit image of W1 (w_global)]
template <typename T, int CB>
int dpw_launch_dx_all(const DpPlan& P, const T* x, const float* w1, const float* b1, const int32_t* bins, int nb,
                      const float* dhpool, T* dx, int N, int H, int W, int ldx, int hid, int sh, int sw, float slope,
                      float* ws, hipStream_t st) {
  const bool cells = bins == nullptr;
  const int njobs = cells ? N * (2 * sh - 1) * (2 * sw - 1) : nb;
  DpRec* recs = reinterpret_cast<DpRec*>(ws + (size_t)DPM_WGS * DPM_PART);
  unsigned char* wglob = reinterpret_cast<unsigned char*>(recs + (size_t)4 * nb);
  hipLaunchKernelGGL(dpm_jobs_kernel, dim3(cy_cdiv(njobs, 256)), dim3(256), 0, st, bins, njobs, recs, cells ? 1 : 0, sh,
                     sw, H, W);
  CY_CHECK_LAUNCH();
  if (P.w_global) {
    hipLaunchKernelGGL(dpw_round_w_kernel<T>, dim3(cy_cdiv((long)hid * CB * 4, 256)), dim3(256), 0, st, w1, CB, hid, wglob);
    CY_CHECK_LAUNCH();
  }
  for (int cbs = 0; cbs < CB; ++cbs) {  // one block of 32 channels per launch
    int rc = CY_OK;
    if (cells) {
      rc = hid == 256 ? dpw_launch_dx<T, 8, true, CB>(P, x, w1, b1, recs, njobs, dhpool, dx, wglob, W, ldx, hid, slope, -1, cbs, st)
                      : dpw_launch_dx<T, 4, true, CB>(P, x, w1, b1, recs, njobs, dhpool, dx, wglob, W, ldx, hid, slope, -1, cbs, st);
    } else {
      for (int colour = 0; colour < 4 && rc == CY_OK; ++colour)
        rc = hid == 256
                 ? dpw_launch_dx<T, 8, false, CB>(P, x, w1, b1, recs, njobs, dhpool, dx, wglob, W, ldx, hid, slope, colour, cbs, st)
                 : dpw_launch_dx<T, 4, false, CB>(P, x, w1, b1, recs, njobs, dhpool, dx, wglob, W, ldx, hid, slope, colour, cbs, st);
    }
    if (rc != CY_OK) return rc;
  }
  return CY_OK;
}

}  // namespace
