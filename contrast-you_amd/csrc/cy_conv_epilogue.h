// Pieces of the epilogue that the 3x3 matrix-core kernels share: the register epilogue of the kernels that run their
// MFMAs with the WEIGHTS as the row operand (plane, flow, stream, first-layer), and the split destination and the
// workgroup finish of the BatchNorm sums, which the igemm kernel shares with them.
//
// After such an MFMA a lane (r = lane & 31, h = lane >> 5) holds ONE output position and 16 couts of a 32-cout
// block in four runs of four consecutive channels: register `reg` is channel frag_channel(reg, h) of the block.
// From there
//   * frag_pair_swap pairs two runs across the half-waves, so that a lane stores 16 bytes instead of 8 twice;
//   * frag_stats_reduce reduce-scatters the 16 per-register sums of the statistics over the 32 lanes of a half-wave,
//     after which the lane holds the totals of register frag_stats_reg(lane);
//   * conv_stats_finish adds the wave rows a workgroup left in LDS and hands the totals to the BatchNorm, as one
//     partial row per tile or into the accumulator of cy_bn_acc.h;
//   * conv_out_ptr is the destination of a channel run when the output is split over two tensors.
//
// Every helper is forced inline and takes arrays as plain pointers.  Both matter: these kernels sit at their register
// limits, and the same statements behind an array reference, a by-value payload or one more level of calls reach the
// register allocator in another order -- which has cost between one spilled register and an occupancy step.  The
// resource table of cy_conv3x3.hip (-Rpass-analysis=kernel-resource-usage through tools/resusage.py) is the check for
// any change here.  For the same reason some copies are still written out where they were, because behind a call each
// of them changed that table: the half-wave swap in conv3x3_flow_kernel, the channel formula in conv3x3_plane_kernel,
// and the round-and-pack loops and split-K slab stores of all of them (the rows each trial changed: DESIGN.md, "The
// conv kernels' shared epilogue pieces").
#pragma once
#include "cy_conv_tile.h"

namespace {

// channel, inside the fragment's 32-cout block, of accumulator register `reg` in half-wave h
__device__ __forceinline__ int frag_channel(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// Lane i holds channels 8g+0..3 (lo) and 8g+8+0..3 (hi) of its position, lane i+32 channels 8g+4..7 and 8g+8+4..7 of
// the same position (g even): one half-wave swap per dword leaves the lower half with channels 8g .. 8g+7 and the upper
// half with 8g+8 .. 8g+15 in (lo, hi) -- {lo[0], lo[1], hi[0], hi[1]} is ONE 16-byte store at channel 8g + 8h, two per
// fragment instead of four 8-byte ones
__device__ __forceinline__ void frag_pair_swap(u32x2& lo, u32x2& hi) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const auto sw = __builtin_amdgcn_permlane32_swap(lo[j], hi[j], false, false);
    lo[j] = sw[0];
    hi[j] = sw[1];
  }
}

// one stage of the reduce-scatter: lanes paired by xor 2W exchange halves of the 2W live registers and keep W.
// (W is a template parameter: a run-time loop over the stage width is not unrolled, and costs registers)
template <int W> __device__ __forceinline__ void frag_stats_stage(float* s1, float* s2, int lane) {
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const bool up = (lane & (2 * W)) != 0;
    const float snd1 = up ? s1[i] : s1[i + W], snd2 = up ? s2[i] : s2[i + W];
    const float kp1 = up ? s1[i + W] : s1[i], kp2 = up ? s2[i + W] : s2[i];
    s1[i] = kp1 + __shfl_xor(snd1, 2 * W, 64);
    s2[i] = kp2 + __shfl_xor(snd2, 2 * W, 64);
  }
}

// Reduce-scatter of a lane's 16 per-register sums s1[16], s2[16] over the 32 lanes of its half (same h): xor 16 / 8 /
// 4 / 2 halve the register count while they pair the lanes, xor 1 joins the last pair.  Every lane ends up with the
// half-wave totals of ONE register, frag_stats_reg(lane), in s1[0] / s2[0]; the two lanes of an even / odd pair hold
// the same one, and the even lane is the one that stores it
__device__ __forceinline__ void frag_stats_reduce(float* s1, float* s2, int lane) {
  frag_stats_stage<8>(s1, s2, lane);
  frag_stats_stage<4>(s1, s2, lane);
  frag_stats_stage<2>(s1, s2, lane);
  frag_stats_stage<1>(s1, s2, lane);
  s1[0] += __shfl_xor(s1[0], 1, 64);
  s2[0] += __shfl_xor(s2[0], 1, 64);
}
__device__ __forceinline__ int frag_stats_reg(int lane) {
  return ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
}

// destination of channel `co` of output position gp: the second tensor takes the channels from a.split_c on
template <typename T>
__device__ __forceinline__ T* conv_out_ptr(const ConvArgs& a, T* o1, T* o2, size_t gp, int co) {
  return (a.split_c > 0 && co >= a.split_c) ? o2 + gp * a.ldo2 + (co - a.split_c) : o1 + gp * a.ldo + co;
}

// the workgroup's totals of channel `tid` of its cout block: the WGM wave rows [sum | sum of squares][BN] in sstat
template <int BN, int WGM>
__device__ __forceinline__ void conv_stats_total(const float* sstat, int tid, float& t1, float& t2) {
  t1 = 0.f, t2 = 0.f;
#pragma unroll
  for (int q = 0; q < WGM; ++q) {
    t1 += sstat[(q * 2 + 0) * BN + tid];
    t2 += sstat[(q * 2 + 1) * BN + tid];
  }
}

// Workgroup finish of the BatchNorm sums (behind the __syncthreads() that follows the waves' writes to sstat): thread
// tid owns cout n0 + tid and either adds its totals into the accumulator a.sacc (cy_bn_acc.h) or writes them into the
// tile's partial row of a.stats
template <int BN, int WGM>
__device__ __forceinline__ void conv_stats_finish(const ConvArgs& a, const float* sstat, int tile, int n0, int tid) {
  if (tid < BN && n0 + tid < a.Cout) {
    float t1, t2;
    conv_stats_total<BN, WGM>(sstat, tid, t1, t2);
    if (a.sacc) {
      bn_acc_add(a.sacc, a.sR, a.Cout, tile & (a.sR - 1), 0, n0 + tid, t1);
      bn_acc_add(a.sacc, a.sR, a.Cout, tile & (a.sR - 1), 1, n0 + tid, t2);
    } else {
      a.stats[((size_t)tile * 2 + 0) * a.Cout + n0 + tid] = t1;
      a.stats[((size_t)tile * 2 + 1) * a.Cout + n0 + tid] = t2;
    }
  }
}

}  // namespace
