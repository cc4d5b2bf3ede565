/*
 * contrastyou_hip.h -- C ABI of libcontrastyou_hip.so, the MI355X (gfx950)
 * implementation of the Contrast-You SemiSupervisedEpocher hot path.
 *
 * The reference (jizongFox/Contrast-You) is 100 % Python on torch: it has no
 * FFI of its own.  Every entry point below therefore replaces a torch library
 * call made by a reference leaf; the file:line of that call site is cited per
 * function.  Conventions:
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *     the parameter name starts with h_ (host);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it,
 *     nothing synchronises, nothing allocates (callers pass workspaces);
 *   - activations are NHWC ("channels_last"): element (n,h,w,c) lives at
 *     ((n*H + h)*W + w)*ld + c, ld >= C the pixel pitch in elements;
 *   - dtype codes: CY_F32 (verification mode, f32 MFMA, exact fmaf chains)
 *     CY_BF16 (production mode, bf16 MFMA with f32 accumulation) and CY_F16
 *     (the reference's fp16 autocast mode, f16 MFMA with f32 accumulation);
 *   - return value 0 = enqueued, <0 = argument/shape error (nothing was
 *     launched), see CY_ERR_*.
 */
#ifndef CONTRASTYOU_HIP_H
#define CONTRASTYOU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CY_OK 0
#define CY_ERR_ARG (-1)
#define CY_ERR_SHAPE (-2)
#define CY_ERR_DTYPE (-3)
#define CY_ERR_LAUNCH (-4)
#define CY_ERR_WORKSPACE (-5)

#define CY_F32 0
#define CY_BF16 1
#define CY_F16 2 /* IEEE half: the reference's own autocast dtype (contrastyou/amp/amp.py:13-45); same kernels as
                  * CY_BF16 with mfma_f32_32x32x16_f16, f32 accumulation; needs loss scaling (torch GradScaler) */

/* how source 1 of a 3x3 conv is addressed (arch/unet.py:67-70 MaxPool2d,
 * :38 Upsample(scale_factor=2) nearest, both folded into the conv's loads) */
#define CY_SRC_DIRECT 0 /* src1 is [N,H,W,C1] */
#define CY_SRC_POOL2 1  /* src1 is [N,2H,2W,C1]; 2x2 max taken on load */
#define CY_SRC_UP2 2    /* src1 is [N,H/2,W/2,C1]; nearest x2 on load */

/* ABI version; bumped whenever a signature changes.  This line is the only place the number is written: the library
 * returns it and the Python binding (cyhip/_lib.py, derived from this header) reads it from here. */
#define CY_ABI_VERSION 19
int cy_abi_version(void);
/* name of the offload arch the library was built for ("gfx950"). */
const char* cy_build_arch(void);
/* id of the HIP-graph capture `stream` currently belongs to, 0 when it is not capturing.  Host-side
 * only (hipStreamGetCaptureInfo): lets the binding tell apart events recorded in different captures
 * (an event recorded inside one capture must not be waited on inside another). */
unsigned long long cy_stream_capture_id(void* stream);
/* profiling aid: a one-thread kernel on `stream` stores the device wall clock (100 MHz ticks) into
 * buf[slot] (device memory); works inside a stream capture. */
int cy_debug_stamp(unsigned long long* buf, int slot, void* stream);
/* measurement aid: a one-lane kernel that holds `stream` for `micros` (<= 50000) microseconds of the device wall
 * clock, so that a host can enqueue work behind it and time back-to-back GPU execution with events. */
int cy_debug_spin(int micros, void* stream);
/* measurement aid: timing-only HIP events (hipEventDisableSystemFence: recording one does not write back and
 * invalidate the L2s, which a default event does -- inside the interval it measures).  elapsed_us synchronises on
 * e1 first. */
int cy_debug_event_create(void** ev);
int cy_debug_event_record(void* ev, void* stream);
int cy_debug_event_elapsed_us(void* e0, void* e1, float* us);
int cy_debug_event_destroy(void* ev);
/* Hand-over from a captured HIP graph to a stream outside it (the data-parallel optimizer starts the all-reduce of
 * the gradient buckets whose layers are done while the rest of the backward graph runs): `stream` waits until the
 * int32 counter in device memory, which a kernel of the graph increments, is >= at_least. */
int cy_stream_wait_value(void* stream, const int* counter, int at_least);

/* ------------------------------------------------------------------------
 * 3x3 convolution, stride 1, pad 1, no bias  (nn.Conv2d at
 * contrastyou/arch/unet.py:21,24,39) as an implicit GEMM on MFMA.
 *
 * Geometry: output [N,H,W,Cout].  Logical input = channel concat of source 1
 * (C1 channels, addressed per `mode1`) and optional source 2 (C2 channels,
 * always direct) -- torch.cat((skip, up), dim=1) at arch/unet.py:142,151,160,
 * 169 without the copy.  If `prologue` != 0 source 1 is a RAW conv output of
 * the previous layer and relu(scale[c]*x + shift[c]) (training-mode
 * BatchNorm2d + ReLU, arch/unet.py:22-23) is applied while loading it.
 * ------------------------------------------------------------------------ */
typedef struct cy_conv_desc {
  int32_t N, H, W;      /* output spatial geometry */
  int32_t C1, C2, Cout; /* channels of source 1, source 2 (0 = none), output */
  int32_t mode1;        /* CY_SRC_* for source 1 */
  int32_t prologue;     /* 1: relu(scale*x+shift) on source 1 while loading */
  int32_t in_dtype;     /* dtype of sources and packed weights */
  int32_t out_dtype;    /* dtype of the output tensor */
  int32_t ld1, ld2;     /* pixel pitch (elements) of source 1 / 2 */
  int32_t ldo;          /* pixel pitch of `out` */
  int32_t split_c;      /* >0: couts >= split_c go to out2 (pitch ldo2) */
  int32_t ldo2;
} cy_conv_desc;

/* Packed weight geometry for a (Cout,Cin) 3x3 kernel: [9][co_pad][ci_pad]. */
int cy_conv3x3_packed_dims(int Cout, int Cin, int* co_pad, int* ci_pad);

/* Elements of the packed image of a (Cout, Cin) kernel in `dtype`: the [9][co_pad][ci_pad] image, followed for
 * 16-bit dtypes with Cout % 64 == 0 and Cin % 16 == 0 by the stage-contiguous image of the LDS-DMA kernel
 * (csrc/cy_conv_flow.h): [Cout/64][Cin/16][tap][2][64 couts][8 channels] = 9*Cout*Cin elements. */
long long cy_conv3x3_packed_elems(int Cout, int Cin, int dtype);

/* Repack reference-layout weights w[Cout][Cin][3][3] (f32) into the forward
 * image wf (cy_conv3x3_packed_elems(Cout, Cin, dtype) elements: [tap][co_pad][ci_pad], then the stage-contiguous
 * image) and (if wd != NULL) the data-gradient image wd (cy_conv3x3_packed_elems(Cin, Cout, dtype) elements:
 * wd[tap][ci_pad'][co_pad'] = w[co][ci][2-kh][2-kw], then its stage-contiguous image), both of `dtype`. */
int cy_conv3x3_pack_weights(const float* w, void* wf, void* wd, int Cout, int Cin, int dtype,
                            void* stream);

/* All 3x3 weights of a network in ONE launch (the per-layer call above costs a launch per layer and
 * step: the weights change with every optimizer step).  `items` is a DEVICE array describing the
 * layers: source pointer, geometry, the element offsets of the layer's forward / data-gradient image
 * inside the two output arenas, and `first` = index of the layer's first work unit in the flattened
 * range [0, total).  A work unit is a 32 (co) x 32 (ci) tile; a layer has
 * ceil(max(co_pad, co_pad2) / 32) * ceil(max(ci_pad, ci_pad2) / 32) of them, co-major.
 * Offsets instead of pointers keep the table valid when the arenas are re-allocated per step. */
typedef struct cy_pack_item {
  const float* w;          /* [Cout][Cin][3][3] f32 */
  long long off_f, off_d;  /* element offsets into wf_arena / wd_arena */
  long long first;
  int Cout, Cin;
  int co_pad, ci_pad;      /* forward image  [9][co_pad][ci_pad]   (cy_conv3x3_packed_dims(Cout, Cin)) */
  int ci_pad2, co_pad2;    /* dgrad image    [9][ci_pad2][co_pad2] (cy_conv3x3_packed_dims(Cin, Cout)) */
  long long off_ff, off_fd; /* element offsets of the stage-contiguous images in the same arenas, or -1 (none) */
} cy_pack_item;
int cy_conv3x3_pack_weights_batched(const cy_pack_item* items, int n_items, long long total,
                                    void* wf_arena, void* wd_arena, int dtype, void* stream);

/* Number of per-tile statistic partials the forward kernel writes for `d`
 * (stats buffer is float[num_partials][2][Cout]: sum, sum of squares). */
int cy_conv3x3_num_partials(const cy_conv_desc* d);

/* The launch plan the library derives for `d`: which kernel instantiation cy_conv3x3_fwd will run.
 * Parity tests assert on it, so that every instantiation that appears in profiles/ is known to be
 * covered by a test that provably took it (the plan depends on N, H, W, channel counts and dtype). */
#define CY_CONV_KERNEL_IGEMM 0  /* conv3x3_igemm_kernel */
#define CY_CONV_KERNEL_PLANE 1  /* conv3x3_plane_kernel */
#define CY_CONV_KERNEL_STREAM 4 /* conv3x3_stream_kernel */
#define CY_CONV_KERNEL_FLOW 5   /* conv3x3_flow_kernel */
typedef struct cy_conv_plan {
  int32_t kernel;     /* CY_CONV_KERNEL_* */
  int32_t th, tw, bn; /* output tile (rows x columns) and output channels per workgroup */
  int32_t ksplit;     /* >1: split-K over input-channel chunks + conv_splitk_finish_kernel */
  int32_t one_per_cu; /* plane kernel, 128 couts: the one-workgroup-per-CU build with halo prefetch */
  int32_t partials;   /* = cy_conv3x3_num_partials(d) */
  int32_t workgroups; /* grid size of the conv launch */
} cy_conv_plan;
int cy_conv3x3_plan(const cy_conv_desc* d, cy_conv_plan* plan);

/* out = conv3x3(concat(src1', src2), w).  stats may be NULL.  Layers with too few
 * output tiles to fill the chip run split-K over input-channel chunks and need a
 * workspace of cy_conv3x3_fwd_ws_bytes(d) bytes (0 for the others; ws may then be NULL). */
size_t cy_conv3x3_fwd_ws_bytes(const cy_conv_desc* d);
int cy_conv3x3_fwd(const cy_conv_desc* d, const void* src1, const void* src2, const float* scale,
                   const float* shift, const void* w_packed, void* out, void* out2, float* stats,
                   void* ws, size_t ws_bytes, void* stream);

/* development aid: workgroup 0 of every following streaming-kernel launch (library built with -DCY_STREAM_STAMPS)
 * records shader-clock stamps of its waves into dev_buf[8][128] (DEVICE memory; NULL switches it off again). */
int cy_debug_conv_stamps(unsigned long long* dev_buf);
/* development aid: per-wave phase totals (shader clocks) of the twelve-wave weight-gradient kernel's tile loop
 * (library built with -DCY_WGRAD_STAMPS), [12 waves][8] = {request, mfma loop, commit, barrier, tiles}. */
int cy_debug_wgrad_stamps(unsigned long long* dev_buf);

/* Weight gradient dw[Cout][Cin][3][3] (f32, reference layout) =
 *   sum_p dy[p][co] * in[p+tap][ci]  with `in` addressed exactly as in
 * cy_conv3x3_fwd (same desc; desc.out_dtype/ldo describe dy).  ws is a
 * workspace of at least cy_conv3x3_wgrad_ws_bytes(d) bytes.  accumulate != 0:
 * dw += result (autograd's gradient accumulation folded into the reduction). */
size_t cy_conv3x3_wgrad_ws_bytes(const cy_conv_desc* d);
int cy_conv3x3_wgrad(const cy_conv_desc* d, const void* src1, const void* src2, const float* scale,
                     const float* shift, const void* dy, float* dw, int accumulate, void* ws,
                     size_t ws_bytes, void* stream);

/* Launch plan of the weight gradient for `d` (+ n_b images of a second segment, 0 for none). */
typedef struct cy_wgrad_plan {
  int32_t twelve;        /* 2: wgrad12s_kernel (wave-specialised, 64x64 blocks), 1: wgrad12_kernel, 0: wgrad_kernel */
  int32_t wco, wci, wk;  /* wave layout: 32x32 (co,ci) blocks per workgroup and pixel splits inside it */
  int32_t th, tw;        /* spatial tile */
  int32_t splits;        /* pixel splits = f32 slabs summed by wgrad_reduce_kernel */
  int32_t workgroups;
  int32_t dma;           /* wgrad12s_kernel: loader waves on LDS-DMA (32-bit buffer offsets: every tensor below 2 GiB) */
  int32_t blk_order;     /* wgrad12s_kernel: 4 x 4 pixel patches as k-steps (ABI v13: dma, blk_order appended) */
} cy_wgrad_plan;
int cy_conv3x3_wgrad_plan(const cy_conv_desc* d, int n_b, cy_wgrad_plan* plan);

/* The same layer's weight gradient over TWO batches in one launch: segment a is described by `d`
 * (d->N images), segment b has n_b images of the same geometry with its own tensors and -- if
 * d->prologue -- its own BN coefficients.  dw (+)= dw_a + dw_b (fixed summation order).  This is what
 * the two network passes of SemiSupervisedEpocher's two-stage step (epocher.py:348-360) contribute to
 * one weight; one launch instead of two halves the slab traffic and the launch count of the encoder.
 * bf16 only (CY_ERR_DTYPE otherwise). */
size_t cy_conv3x3_wgrad_pair_ws_bytes(const cy_conv_desc* d, int n_b);
int cy_conv3x3_wgrad_pair(const cy_conv_desc* d, const void* src1, const void* src2, const float* scale,
                          const float* shift, const void* dy, int n_b, const void* src1_b,
                          const void* src2_b, const float* scale_b, const float* shift_b,
                          const void* dy_b, float* dw, int accumulate, void* ws, size_t ws_bytes,
                          void* stream);

/* ---- The weight gradient's slab sum as a batched step of its own (ABI v14) ------------------------------------------
 * cy_conv3x3_wgrad / _pair / cy_conv3x3_first_wgrad are two launches: the MFMA (first layer: VALU) kernel writes f32
 * partial sums into `ws`, then a reduce launch adds them into dw.  The _deferred forms enqueue the first launch only and
 * fill *h_entry (host memory) with what the second would have done; cy_wgrad_reduce_batched then runs the reductions of
 * many such entries in ONE launch, each output with exactly the summation tree of its own reduce launch (bit-identical
 * results).  `ws` must stay untouched until that launch has run. */
#define CY_WGRAD_REDUCE_CONV 0  /* 3x3 conv slabs ws[S][9][co_pad][ci_pad] */
#define CY_WGRAD_REDUCE_FIRST 1 /* first-layer partials ws[S][Cout][Cin][9], summed in SG = 64 slices */
#define CY_WGRAD_REDUCE_MAX 32  /* entries per launch */
typedef struct cy_wgrad_reduce_entry {
  const float* ws;
  float* dw;               /* [Cout][Cin][3][3] f32 */
  int32_t kind;            /* CY_WGRAD_REDUCE_* */
  int32_t S, SG;           /* partial sums, slab groups: group g adds slabs g, g + SG, ... in order, then the groups in order */
  int32_t Cout, Cin, co_pad, ci_pad;
  int32_t accumulate;      /* dw = dw + sum (1) or dw = sum (0) */
  int32_t blocks;          /* workgroups of its reduction */
  int32_t first_block;     /* set by cy_wgrad_reduce_batched */
} cy_wgrad_reduce_entry;
int cy_conv3x3_wgrad_deferred(const cy_conv_desc* d, const void* src1, const void* src2, const float* scale,
                              const float* shift, const void* dy, float* dw, int accumulate, void* ws,
                              size_t ws_bytes, cy_wgrad_reduce_entry* h_entry, void* stream);
int cy_conv3x3_wgrad_pair_deferred(const cy_conv_desc* d, const void* src1, const void* src2, const float* scale,
                                   const float* shift, const void* dy, int n_b, const void* src1_b,
                                   const void* src2_b, const float* scale_b, const float* shift_b,
                                   const void* dy_b, float* dw, int accumulate, void* ws, size_t ws_bytes,
                                   cy_wgrad_reduce_entry* h_entry, void* stream);
int cy_conv3x3_first_wgrad_deferred(const float* x, const void* dy, float* dw, int accumulate, int N, int Cin,
                                    int H, int W, int Cout, int dy_dtype, void* ws, size_t ws_bytes,
                                    cy_wgrad_reduce_entry* h_entry, void* stream);
/* host-side queries, nothing launched: the entry (kind, S, SG, Cout, Cin, pads, blocks) the call with `d` (+ n_b images
 * of a second segment) / with these first-layer sizes would produce; ws, dw, accumulate are left zero */
int cy_conv3x3_wgrad_reduce_entry(const cy_conv_desc* d, int n_b, cy_wgrad_reduce_entry* h_entry);
int cy_conv3x3_first_wgrad_reduce_entry(int N, int Cin, int H, int W, int Cout, int dy_dtype,
                                        cy_wgrad_reduce_entry* h_entry);
/* the reductions of h_entries[0..n) (a HOST array; the table travels as a kernel argument, capturable) in table order.
 * A new launch begins after CY_WGRAD_REDUCE_MAX entries or where an entry's dw overlaps one already in the current
 * launch, so several entries on one dw take effect in table order. */
int cy_wgrad_reduce_batched(const cy_wgrad_reduce_entry* h_entries, int n, void* stream);

/* ---- BatchNorm sums without finalize launches (ABI v11; csrc/cy_bn_acc.h) -------------------------------------
 * A training-mode nn.BatchNorm2d (arch/unet.py:22,25,40) needs per-channel sums over the whole batch.  Instead of
 * per-workgroup partial rows + a finalize launch per layer (cy_bn_finalize / cy_bn_bwd_finalize below, still there),
 * the producing kernels ADD their partials into an accumulator -- 64-bit integer atomics on a two-limb fixed-point
 * split, so the result does not depend on the order of arrival -- and the consuming kernels derive the coefficients
 * themselves; the consumer's first workgroup leaves them in memory (`coef`) for the backward pass.
 * Accumulator: int64 words [R][4][C] ({sum hi, lo, sum of squares hi, lo} per replica) + R flag words; the caller
 * zeroes it before the producing launch.  R = cy_bn_acc_replicas(C, workgroups adding into a channel). */
typedef struct cy_bn_acc {
  void* acc;
  int32_t R, C;
} cy_bn_acc;
typedef struct cy_bn_fold {
  const void* acc;     /* the accumulator the previous conv filled */
  int32_t R, C;
  const float* gamma;  /* [C] or NULL (1) */
  const float* beta;   /* [C] or NULL (0) */
  double count;        /* N*H*W */
  float eps;
  int32_t reserved;
  float* coef;         /* [5][C] f32: scale, shift, mean, invstd, unbiased variance (for cy_bn_running_update) */
} cy_bn_fold;
int cy_bn_acc_replicas(int C, int workgroups);
size_t cy_bn_acc_bytes(int C, int R);
/* workgroups of cy_conv3x3_fwd(d) / cy_conv3x3_first_fwd that add into one channel's sums (for cy_bn_acc_replicas) */
int cy_conv3x3_stat_workgroups(const cy_conv_desc* d);
/* cy_conv3x3_fwd with either side of the convolution on accumulators: `in_fold` != NULL (and d->prologue): the
 * BN+ReLU coefficients of source 1 come from the previous layer's accumulator (kernels that cannot fold in place
 * run cy_bn_fold first); `out_acc` != NULL: the statistics of the output are added into it. */
int cy_conv3x3_fwd_bn(const cy_conv_desc* d, const void* src1, const void* src2, const cy_bn_fold* in_fold,
                      const float* scale, const float* shift, const void* w_packed, void* out, void* out2,
                      float* stats, const cy_bn_acc* out_acc, void* ws, size_t ws_bytes, void* stream);
int cy_conv3x3_first_fwd_acc(const float* x, const float* w, void* out, const cy_bn_acc* out_acc, int N, int Cin,
                             int H, int W, int Cout, int out_dtype, void* stream);
/* accumulator -> f->coef as its own launch (what a folding consumer does in its first workgroup) */
int cy_bn_fold_coef(const cy_bn_fold* f, void* stream);
/* out = relu(scale*y + shift) (+ 2x2 max) with the coefficients taken from the accumulator */
int cy_bn_relu_apply_fold(const void* y, const cy_bn_fold* f, void* out, long npix, int y_dtype, int out_dtype,
                          void* stream);
int cy_bn_relu_apply_pool_fold(const void* y, const cy_bn_fold* f, void* out, void* pooled, int N, int H, int W,
                               int y_dtype, int out_dtype, void* stream);
/* running statistics of up to 32 BatchNorm layers in ONE launch: running = (1 - momentum) * running + momentum *
 * batch moment, from the `coef` arrays their consumers left (rows 2 and 4).  `h_items` is a HOST array: the
 * pointers travel as kernel arguments (capturable, no device table). */
typedef struct cy_bn_run_item {
  const float* coef;
  float* running_mean;
  float* running_var;
  int32_t C;
  float momentum;
} cy_bn_run_item;
int cy_bn_running_update(const cy_bn_run_item* h_items, int n, void* stream);
/* backward: the sums of dz and dz*xhat into an accumulator (as cy_bn_relu_bwd_reduce / cy_maxpool2_bwd_bn write
 * partial rows); coef = the forward pass's [5][C] */
int cy_bn_relu_bwd_reduce_acc(const void* da, int ld_da, const void* y, const float* coef, const cy_bn_acc* acc,
                              long npix, int C, int dtype, void* stream);
int cy_bn_relu_bwd_workgroups(long npix, int C);
int cy_maxpool2_bwd_bn_acc(const void* x, const void* dpool, const void* add, int ld_add, void* dx, const void* y,
                           const float* coef, const cy_bn_acc* acc, int N, int H, int W, int C, int dtype,
                           void* stream);
/* cy_upsample2_bwd whose output is the dA of relu(bn(y)) (the last BatchNorm of the block the Upsample read): that
 * layer's backward sums are added into `acc` from the values in registers (what cy_maxpool2_bwd_bn_acc does for the
 * encoder).  (H, W) are the low-resolution dims; y is [N,H,W,C].  cy_upsample2_bwd_bn_workgroups: the adders per
 * channel (for cy_bn_acc_replicas), or CY_ERR_SHAPE where the form does not apply (256 % (C/8) != 0). */
int cy_upsample2_bwd_bn_workgroups(int N, int H, int W, int C);
int cy_upsample2_bwd_bn_acc(const void* dup, int ld_dup, void* dx, const void* y, const float* coef,
                            const cy_bn_acc* acc, int N, int H, int W, int C, int dtype, void* stream);
/* dy = scale*dz + k1*y + k0 with (k1, k0) derived from the accumulator; the first workgroup adds (accumulate != 0) or
 * stores dgamma / dbeta (either may be NULL) */
int cy_bn_relu_bwd_apply_fold(const void* da, int ld_da, const void* y, const float* coef, const cy_bn_acc* acc,
                              double count, int batch_stats, float* dgamma, float* dbeta, int accumulate, void* dy,
                              long npix, int C, int dtype, void* stream);

/* The data gradient of a 3x3 conv with the backward of the BatchNorm + ReLU behind that conv in its load path
 * (autograd of arch/unet.py:21-23 in one launch instead of cy_bn_relu_bwd_apply + cy_conv3x3_fwd):
 *   dy = scale * dA * [scale*y + shift > 0] + k1*y + k0     (formed in LDS from dA and y, (k1, k0) from `acc`)
 *   out = conv3x3(dy, w_packed)                             (w_packed = the data-gradient image of the layer)
 * and dy is also written to bn->dy for the weight gradient.  d describes the data-gradient convolution with
 * d->prologue == 2: C1 = the forward layer's output channels, C2 = 0, direct source; dA, y and dy share the pitch
 * d->ld1.  The first workgroup adds (accumulate) or stores dgamma / dbeta.  Only launch plans with room for the second
 * halo buffer take this path: ask cy_conv3x3_dgrad_bn_ok(d) (1 / 0) and fall back to the two launches otherwise. */
typedef struct cy_bn_bwd_in {
  const void* y;        /* the forward layer's raw conv output [N,H,W,C1] */
  const float* coef;    /* the forward pass's [5][C1] */
  const cy_bn_acc* acc; /* sums of dz and dz*xhat (cy_bn_relu_bwd_reduce_acc / cy_maxpool2_bwd_bn_acc) */
  double count;         /* N*H*W */
  int32_t batch_stats, accumulate;
  float* dgamma;        /* [C1] or NULL */
  float* dbeta;
  void* dy;             /* out: [N,H,W,C1] */
} cy_bn_bwd_in;
int cy_conv3x3_dgrad_bn_ok(const cy_conv_desc* d);
int cy_conv3x3_dgrad_bn(const cy_conv_desc* d, const void* dA, const cy_bn_bwd_in* bn, const void* w_packed, void* out,
                        void* out2, void* ws, size_t ws_bytes, void* stream);

/* A data gradient whose output (all couts, or the second part of a split output: channels [c0, c0 + C)) is the dA of
 * a BatchNorm + ReLU: the epilogue adds that layer's backward sums (dz = dA * [scale*y + shift > 0], dz * xhat) into
 * `acc` from the values it has in registers -- y of that layer is read once, at the output positions -- and the reduce
 * launch (cy_bn_relu_bwd_reduce_acc) is not needed.  Flow-kernel plans without split-K whose cout blocks align with the
 * range: ask cy_conv3x3_dgrad_dz_ok(d, c0, C). */
typedef struct cy_bn_dz_out {
  const void* y;        /* [N,H,W,C], contiguous */
  const float* coef;    /* that layer's forward [5][C] */
  const cy_bn_acc* acc;
  int32_t c0, C;
} cy_bn_dz_out;
int cy_conv3x3_dgrad_dz_ok(const cy_conv_desc* d, int c0, int C);
int cy_conv3x3_dgrad_dz(const cy_conv_desc* d, const void* dy, const void* w_packed, void* out, void* out2,
                        const cy_bn_dz_out* dz, void* ws, size_t ws_bytes, void* stream);

/* First layer (input_dim 1..4, arch/unet.py:72): x is the f32 NCHW image
 * [N,Cin,H,W]; w is the reference-layout f32 weight [Cout][Cin][3][3]. */
int cy_conv3x3_first_num_partials(int N, int H, int W, int Cout);
int cy_conv3x3_first_fwd(const float* x, const float* w, void* out, float* stats, int N, int Cin,
                         int H, int W, int Cout, int out_dtype, void* stream);
size_t cy_conv3x3_first_wgrad_ws_bytes(int N, int Cin, int H, int W, int Cout);
int cy_conv3x3_first_wgrad(const float* x, const void* dy, float* dw, int accumulate, int N, int Cin,
                           int H, int W, int Cout, int dy_dtype, void* ws, size_t ws_bytes,
                           void* stream);

/* ------------------------------------------------------------------------
 * BatchNorm2d (training statistics) + ReLU   (arch/unet.py:22-23,25-26,40-41)
 * ------------------------------------------------------------------------ */
/* Reduce conv-epilogue partials to per-channel mean / biased var, fold them
 * with gamma/beta into scale/shift, and update running stats
 * (momentum, unbiased var; torch.nn.BatchNorm2d semantics).
 * use_batch_stats=0 (module.eval()): scale/shift come from running stats.
 * update_running=0: track_running_stats disabled (utils/utils.py:225-237). */
int cy_bn_finalize(const float* partials, int num_partials, int C, double count,
                   const float* gamma, const float* beta, float* running_mean,
                   float* running_var, float momentum, float eps, int use_batch_stats,
                   int update_running, float* scale, float* shift, float* mean, float* invstd,
                   void* stream);

/* out = relu(scale[c]*y + shift[c]) over npix pixels of C channels. */
int cy_bn_relu_apply(const void* y, const float* scale, const float* shift, void* out,
                     long npix, int C, int y_dtype, int out_dtype, void* stream);

/* The same, and the 2x2 max of the result (nn.MaxPool2d(2) of the block output, contrastyou/arch/unet.py:108-121)
 * into `pooled` [N,H,W,C] in one pass; y / out are [N,2H,2W,C] (H, W: the POOLED dims).  out and pooled share
 * out_dtype = y_dtype; the pooled values are maxima of the stored (rounded) outputs. */
int cy_bn_relu_apply_pool(const void* y, const float* scale, const float* shift, void* out, void* pooled,
                          int N, int H, int W, int C, int y_dtype, int out_dtype, void* stream);

/* Backward of y -> relu(bn(y)).  Step 1: per-channel sums of
 * dz = da*(scale*y+shift > 0) and dz*xhat into partials
 * float[num_partials][2][C];  num_partials from cy_bn_bwd_num_partials. */
int cy_bn_bwd_num_partials(long npix, int C);
int cy_bn_relu_bwd_reduce(const void* da, int ld_da, const void* y, const float* scale,
                          const float* shift, const float* mean, const float* invstd,
                          float* partials, long npix, int C, int dtype, void* stream);
/* Step 2: dgamma/dbeta from the partials (fixed summation order; accumulate != 0
 * adds into them) and the per-channel coefficients coef[2][C] = {k1, k0} of step 3. */
int cy_bn_bwd_finalize(const float* partials, int num_partials, int C, const float* scale,
                       const float* mean, const float* invstd, double count, int batch_stats,
                       float* dgamma, float* dbeta, int accumulate, float* coef, void* stream);
/* Step 3: dy = scale*dz + k1*y + k0, i.e. scale*(dz - dbeta/M - xhat*dgamma/M) for batch
 * statistics and scale*dz (k1 = k0 = 0) for eval-mode BN. */
int cy_bn_relu_bwd_apply(const void* da, int ld_da, const void* y, const float* scale,
                         const float* shift, const float* coef, void* dy, long npix, int C,
                         int dtype, void* stream);

/* ------------------------------------------------------------------------
 * MaxPool2d(2,2) backward (arch/unet.py:67-70) and nearest-x2 backward
 * (arch/unet.py:38): the forward halves are folded into the conv loads.
 * ------------------------------------------------------------------------ */
/* dx[N,2H,2W,C] = route(dpool[N,H,W,C]) to the first arg-max of each 2x2
 * window of x (+ add[N,2H,2W,C] if add != NULL, pitch ld_add). */
int cy_maxpool2_bwd(const void* x, const void* dpool, const void* add, int ld_add, void* dx, int N,
                    int H, int W, int C, int dtype, void* stream);
/* dx[N,H,W,C] = sum of the 2x2 block of dup[N,2H,2W,C] (pitch ld_dup). */
/* cy_maxpool2_bwd whose output is the dA of a BatchNorm+ReLU (the block's last one, y = its raw conv output): also
 * writes that layer's backward partial sums (what cy_bn_relu_bwd_reduce would compute from dx and y in a second
 * pass), cy_maxpool2_bwd_bn_num_partials rows of [2][C]; feed them to cy_bn_bwd_finalize. */
int cy_maxpool2_bwd_bn_num_partials(int N, int H, int W, int C);
int cy_maxpool2_bwd_bn(const void* x, const void* dpool, const void* add, int ld_add, void* dx, const void* y,
                       const float* scale, const float* shift, const float* mean, const float* invstd,
                       float* partials, int N, int H, int W, int C, int dtype, void* stream);
int cy_upsample2_bwd(const void* dup, int ld_dup, void* dx, int N, int H, int W, int C, int dtype,
                     void* stream);

/* Launch plan of the BatchNorm, pool and upsample kernels (ABI v18; csrc/cy_norm_act.hip).  Host-side only, launches
 * nothing and needs no GPU.  Every launch of that file, and cy_bn_bwd_num_partials, cy_bn_relu_bwd_workgroups,
 * cy_maxpool2_bwd_bn_num_partials and cy_upsample2_bwd_bn_workgroups, take kernel, grid and LDS from this function.
 *   kind   what N * H * W counts                                         the launches it describes
 *   CY_NA_APPLY         pixels                                           cy_bn_relu_apply, _apply_fold
 *   CY_NA_APPLY_POOL    2x2 quads (H, W: the pooled dims)                cy_bn_relu_apply_pool, _apply_pool_fold
 *   CY_NA_BWD_REDUCE    pixels                                           cy_bn_relu_bwd_reduce, _reduce_acc
 *   CY_NA_BWD_APPLY     pixels                                           cy_bn_relu_bwd_apply, _apply_fold
 *   CY_NA_POOL_BWD(_BN) 2x2 quads (H, W: the pooled dims)                cy_maxpool2_bwd, (_bwd_bn, _bwd_bn_acc)
 *   CY_NA_UP_BWD(_BN)   source pixels (H, W: the low-resolution dims)    cy_upsample2_bwd, (_bwd_bn_acc)
 *   CY_NA_FINALIZE, CY_NA_BWD_FINALIZE   partial rows                    cy_bn_finalize, cy_bn_bwd_finalize
 *   CY_NA_FOLD_COEF     ignored (pass 1, 1, 1)                           cy_bn_fold_coef
 * dtype: the storage type (CY_F32 / CY_BF16 / CY_F16); the two applies that write another type than they read add
 * CY_NA_OUT(out_dtype).  fold: 0 for the forms fed coefficients or partial rows; R >= 1 (a power of two) for the forms on
 * an accumulator of R replicas (the fold applies, cy_bn_fold_coef; for the reduce and the fused forms: the accumulator
 * they add into).  Returns CY_ERR_ARG for a NULL `out`, an unknown kind, a dimension < 1 or such a `fold`; otherwise
 * CY_OK with `status` = what the launch itself answers for the shape. */
enum {
  CY_NA_APPLY = 0, CY_NA_APPLY_POOL = 1, CY_NA_BWD_REDUCE = 2, CY_NA_BWD_APPLY = 3, CY_NA_POOL_BWD = 4,
  CY_NA_POOL_BWD_BN = 5, CY_NA_UP_BWD = 6, CY_NA_UP_BWD_BN = 7, CY_NA_FINALIZE = 8, CY_NA_BWD_FINALIZE = 9,
  CY_NA_FOLD_COEF = 10
};
#define CY_NA_OUT(out_dtype) (((out_dtype) + 1) << 4)
typedef struct cy_norm_act_plan_t {
  int32_t status;        /* CY_OK, or what the launch returns: CY_ERR_SHAPE (C % 8; C > 1024 on the fold applies, > 2048 on
                            cy_bn_fold_coef; a fused form that does not apply), CY_ERR_DTYPE */
  int32_t kernel;        /* 0 bn_relu_apply_kernel<false>, 1 <true> (fold), 2 bn_relu_apply_pool_kernel<false>, 3 <true>,
                            4 bn_relu_bwd_reduce_kernel<DEEP>, 5 <not DEEP>, 6 bn_relu_bwd_apply_kernel<false>, 7 <true>,
                            8 maxpool2_bwd_kernel<false>, 9 <STATS>, 10 upsample2_bwd_kernel<false>, 11 <STATS>,
                            12 bn_finalize_kernel, 13 bn_bwd_finalize_kernel, 14 bn_fold_kernel.  A fused kind that does
                            not apply reports the unfused kernel (8 / 10) and its grid: what the caller then launches */
  int32_t type_in;       /* CY_F32 / CY_BF16 / CY_F16 */
  int32_t type_out;
  int32_t threads;       /* per workgroup */
  int32_t grid;          /* workgroups */
  int32_t lds_bytes;     /* static + dynamic */
  int32_t items;         /* units of the grid-stride loop (8 channels of a pixel, of a quad, of a source pixel; reduce:
                            pixels; finalize kinds: partial rows; fold_coef: channels), saturated at 2^31 - 1 */
  int32_t trips;         /* most trips a thread makes through that loop */
  int32_t one_trip_items;/* the grid's cap times `threads`: a second trip from one item more (0: the loop has no cap) */
  int32_t fold;          /* replicas R of the accumulator read (fold forms) or added into; 0 none */
  int32_t gather;        /* how a fold form sums the replicas: 0 none, 1 direct (R <= 8), 2 direct, wide (R = 16, 32 in the
                            elementwise kernels), 3 LDS atomics */
  int32_t pow2;          /* backward apply: C/8 is a power of two (shift and mask instead of the division) */
  int32_t deep;          /* reduce: the four-pixel form (grid < 512) */
  int32_t rows;          /* reduce: pixel rows of a workgroup, 256 / groups_per_page */
  int32_t groups_per_page; /* reduce: min(C/8, 256) */
  int32_t pages;         /* reduce: ceil((C/8) / 256) */
  int32_t last_page_groups; /* reduce: channel groups of the last page */
  int32_t pixels_per_workgroup; /* reduce: ceil(pixels / grid) */
  int32_t empty_workgroups;     /* reduce: trailing workgroups that get no pixel (they write zero rows) */
  int32_t round4;        /* reduce: 1 if some thread executes the four-pixel round */
  int32_t tail1;         /* reduce: 1 if some thread executes the one-pixel loop */
  int32_t idle_rows;     /* reduce: pixel rows beyond the pixels of a full workgroup */
  int32_t idle_threads;  /* reduce: 256 - rows * groups_per_page; finalize kinds: threads of the last workgroup past C */
  int32_t fused_ok;      /* kinds *_BN: 1 if the fused form applies (256 % (C/8) == 0), else 0 (status CY_ERR_SHAPE) */
  int32_t partial_rows;  /* rows of [2][C] partial sums written = workgroups adding into one channel's sums; 0: none */
  int32_t chain;         /* longest chain of f32 additions of non-zero terms behind one word of those sums (reduce: trips +
                            rows - idle_rows); 0: none */
} cy_norm_act_plan_t;
int cy_norm_act_plan(int kind, int N, int H, int W, int C, int dtype, int fold, cy_norm_act_plan_t* out);

/* ------------------------------------------------------------------------
 * 1x1 classifier head  nn.Conv2d(C, K, 1) + bias  (arch/unet.py:102)
 * logits are f32 [N,H,W,K].
 * ------------------------------------------------------------------------ */
int cy_head1x1_fwd(const void* x, const float* w, const float* b, float* logits, long npix, int C,
                   int K, int x_dtype, void* stream);
size_t cy_head1x1_bwd_ws_bytes(long npix, int C, int K);
int cy_head1x1_bwd(const void* x, const float* w, const float* dlogits, void* dx, float* dw,
                   float* db, long npix, int C, int K, int x_dtype, void* ws, size_t ws_bytes,
                   void* stream);
/* the same with the parameter gradients ADDED into dw [K][C] / db [K] (the live .grad buffers of the head: autograd's
 * accumulation folded into the reduction, as for the conv and BatchNorm parameters) */
int cy_head1x1_bwd_into(const void* x, const float* w, const float* dlogits, void* dx, float* dw,
                        float* db, long npix, int C, int K, int x_dtype, void* ws, size_t ws_bytes,
                        void* stream);

/* Launch plan of the 1x1 head (ABI v16): everything cy_head1x1_fwd / _bwd / _bwd_into decide from (npix, C, K) and from
 * which gradients are asked for.  Host-side only, launches nothing.  The launches and cy_head1x1_bwd_ws_bytes take
 * their kernel, grid and workspace size from this function.  CY_ERR_SHAPE exactly where the launches refuse: C % 8,
 * K outside 1 .. 128, (K*C + K) * 4 > 60000 bytes of LDS weights, C > 2048 with a parameter gradient on the VALU path.
 * Without need_dx: dx_kernel -1, dx_grid and dx_trips 0; without need_dw: every dw_* field 0. */
typedef struct cy_head_plan {
  int32_t fwd_kernel;       /* 0: head_fwd_kernel<T,16> (K <= 16), 1: head_fwd_kernel<T,128>, 2: matrix cores (LINEAR mode of
                               cluster_head_fwd_kernel; 16 < K <= 128 over 32 / 64 channels) */
  int32_t fwd_waves;        /* matrix cores: 8 or 4 waves per block; 0 on the VALU kernels */
  int32_t fwd_quads;        /* matrix cores: 1 when K % 4 == 0 (16-byte stores of the logits tile), else 0 */
  int32_t fwd_grid;         /* blocks */
  int32_t dx_kernel;        /* 0: head_bwd_dx_kernel (8 channels per thread), 1: head_bwd_dx_wide_kernel (32 channels per
                               thread), 2: matrix cores (cluster_head_bwd_kernel, LINEAR), -1: none */
  int32_t dx_grid;          /* blocks (matrix cores: of the one backward launch, which also gives dW) */
  int32_t dw_group;         /* head_bwd_dw_kernel<T,4> or <T,16>: outputs per pass over the pixels; 0 on the matrix cores */
  int32_t dw_vec_groups;    /* how many of the ceil(K / dw_group) passes load their dlogits as 16-byte vectors ... */
  int32_t dw_scalar_groups; /* ... and how many one float at a time (K % 4 != 0, or the partial last group) */
  int32_t dw_blocks;        /* blocks = rows of partial sums in the workspace (matrix cores: four slabs per block) */
  int32_t dw_rows;          /* VALU: pixel rows per block, 256 / min(C/8, 256); 0 on the matrix cores */
  int32_t fwd_trips;        /* the most trips any thread (VALU) or wave (matrix cores) makes round its grid-stride loop */
  int32_t dx_trips;         /* the same for the data gradient */
  int32_t dw_per;           /* pixels per dW block: ceil(npix / dw_blocks); matrix cores: 128 per trip of a block */
} cy_head_plan;
int cy_head1x1_plan(long npix, int C, int K, int need_dx, int need_dw, cy_head_plan* out);

/* ------------------------------------------------------------------------
 * Supervised loss  KL_div(softmax(logits), one_hot(target))
 * (semi_seg/epochers/epocher.py:317-318, contrastyou/losses/kl.py:112-125,
 *  contrastyou/utils/general.py:114-120):
 *   loss = mean_p -log((softmax(z_p)[t_p] + eps) / (1 + eps))
 * ------------------------------------------------------------------------ */
size_t cy_softmax_kl_ws_bytes(long npix);
int cy_softmax_kl_fwd(const float* logits, const int64_t* target, float* loss, long npix, int K,
                      float eps, void* ws, size_t ws_bytes, void* stream);
/* dlogits = gscale[0]/npix * dloss/dz  (gscale: device scalar, upstream grad) */
int cy_softmax_kl_bwd(const float* logits, const int64_t* target, const float* gscale,
                      float* dlogits, long npix, int K, float eps, void* stream);

/* ------------------------------------------------------------------------
 * Encoder projection head (contrastyou/projectors/heads.py:14-22,81-96,
 * projectors/nn.py:47-54): AdaptiveAvgPool2d(1) -> Linear -> LeakyReLU(0.01)
 * -> Linear -> x / max(||x||_2, 1e-12).
 * ------------------------------------------------------------------------ */
/* pooled[n][c] = mean_{hw} x[n,h,w,c]   (f32 out) */
int cy_avgpool_fwd(const void* x, float* pooled, int N, int HW, int C, int dtype, void* stream);
/* dx[n,h,w,c] = dpooled[n][c] / HW */
int cy_avgpool_bwd(const float* dpooled, void* dx, int N, int HW, int C, int dtype, void* stream);
/* y[m][o] = act(sum_i x[m][i]*w[o][i] + b[o]);  act: 0 none, 1 LeakyReLU(slope) */
int cy_linear_fwd(const float* x, const float* w, const float* b, float* y, int M, int I, int O,
                  int act, float slope, void* stream);
/* given dy (pre-activation gradient is formed inside from y when act=1):
 * dx[m][i], dw[o][i], db[o].  Any of dx/dw/db may be NULL. */
int cy_linear_bwd(const float* x, const float* w, const float* y, const float* dy, float* dx,
                  float* dw, float* db, int M, int I, int O, int act, float slope, void* stream);
/* the same, with dw / db ADDED into (the parameters' .grad buffers: no separate accumulation launch) */
int cy_linear_bwd_into(const float* x, const float* w, const float* y, const float* dy, float* dx,
                       float* dw, float* db, int M, int I, int O, int act, float slope, void* stream);
/* The whole ProjectionHead (contrastyou/projectors/heads.py:12-22,81-96, head_type "mlp", normalize) in one launch:
 * feat NHWC [B][HW][C] (dtype) -> pooled [B][C] -> y1 = lrelu(W1 pooled + b1) [B][hid] -> y2 = W2 y1 + b2 [B][out]
 * -> z = y2 / max(|y2|, eps), norms [B]; pooled / y1 / y2 / norms are what the backward needs.
 * Backward: dfeat (dtype, may be NULL), and dW1 [hid][C], db1, dW2 [out][hid], db2 written or ADDED into
 * (accumulate); ws: cy_proj_head_bwd_ws_bytes.  C % 8 == 0, hid % 4 == 0; C, hid, out <= 512. */
int cy_proj_head_fwd(const void* feat, const float* w1, const float* b1, const float* w2, const float* b2,
                     float* pooled, float* y1, float* y2, float* z, float* norms, int B, int HW, int C, int hid,
                     int out, float slope, float eps, int dtype, void* stream);
size_t cy_proj_head_bwd_ws_bytes(int B, int hid, int out);
int cy_proj_head_bwd(const float* dz, const float* pooled, const float* y1, const float* y2, const float* norms,
                     const float* w1, const float* w2, void* dfeat, float* dw1, float* db1, float* dw2, float* db2,
                     int accumulate, void* ws, size_t ws_bytes, int B, int HW, int C, int hid, int out, float slope,
                     float eps, int dtype, void* stream);
/* z = x / max(||x||,eps) row-wise; norms[m] saved for backward. */
int cy_l2norm_fwd(const float* x, float* z, float* norms, int M, int D, float eps, void* stream);
int cy_l2norm_bwd(const float* x, const float* norms, const float* dz, float* dx, int M, int D,
                  float eps, void* stream);

/* ------------------------------------------------------------------------
 * InfoNCE / SupCon loss  (contrastyou/losses/contrastive.py:14-20,31-100)
 * P = [z1; z2] is [R=2n][D] f32 (unit rows), labels[n] int32 (row i and
 * i+n share labels[i]); t = temperature.
 *   S = P P^T / t;  M = max(S) (incl. diagonal);  E = exp(S - M)
 *   loss = -mean_i [ sum_{j in pos(i)} ((S_ij - M) - log(sum_{k!=i, k in pos(i) or neg(i)} E_ik + 1e-16)) / |pos(i)| ]
 * row_stats (f32 [R][4]) keeps {denominator_i, |pos(i)|, sum_pos S_ij, M}
 * for the backward pass.  Rows with |pos(i)| == 0 give NaN exactly like the
 * reference (which then raises RuntimeError, contrastive.py:98).
 * ------------------------------------------------------------------------ */
/* Either labels (int32 [n]) or pos_mask must be non-NULL; labels win when both are given.
 * pos_mask (uint8 [n][n]) is the `mask=` argument of SupConLoss1.forward, one code per ORDERED pair, in every
 * cy_supcon_* entry below (contrastive.py:35-36):
 *     1 = positive,  0 = negative,  any other value (the criterion writes 2) = neither.
 * A "neither" pair enters no sum: not the denominator sum_k above, not the negative count of exclude_other_pos, and
 * cy_supcon_matrices reports it in neither mask.  The pair (i, j) of the 2n x 2n problem reads pos_mask[i mod n][j mod n];
 * the mask is taken as given and need not be symmetric (the gradient's transposed term reads [j mod n][i mod n]).
 * The diagonal i == j is left out whatever its code.  No signature changed with this contract (codes 1 and 0 mean what
 * they meant).
 * S: f32 [R][R] buffer that receives P P^T / t (kept for backward). */
int cy_supcon_fwd(const float* P, const int32_t* labels, const uint8_t* pos_mask, float* S,
                  float* loss, float* row_stats, int n, int D, float t, void* stream);
/* dP[R][D] = gscale[0] * dloss/dP.  G: f32 [R][R] scratch. */
int cy_supcon_bwd(const float* P, const int32_t* labels, const uint8_t* pos_mask, const float* S,
                  const float* row_stats, const float* gscale, float* G, float* dP, int n, int D,
                  float t, void* stream);
/* SupConLoss1(exclude_other_pos=True) (losses/contrastive.py:87-91): per positive pair the denominator holds that pair and
 * the negatives only, the negatives' sum rescaled by 1 / (neg / (pos + neg) + 1e-4).  On the materialised similarity
 * matrix S [2n][2n]; row_stats [2n][4] and tmp [4 * 2n + 1] are kept for the backward (tmp[8n] = the global maximum). */
int cy_supcon_excl_fwd(const float* P, const int32_t* labels, const uint8_t* pos_mask, float* S, float* loss,
                       float* row_stats, float* tmp, int n, int D, float t, void* stream);
int cy_supcon_excl_bwd(const float* P, const int32_t* labels, const uint8_t* pos_mask, const float* S,
                       const float* row_stats, const float* tmp, const float* gscale, float* G, float* dP, int n, int D,
                       float t, void* stream);
/* materialise sim_logits (S-M), sim_exp, pos_mask, neg_mask, each f32 [R][R]
 * (contrastive.py:79-82; read only for the TensorBoard figures). any may be NULL */
/* The same loss and gradient with S (and the gradient matrix) formed tile by tile in the MFMA accumulators and
 * never written: forward = row sums with the global shift M = max_i |P_i|^2 / t (the maximum of S lies on its
 * diagonal), backward = (1/t) G P with the S tile recomputed.  D <= 256, D % 8 == 0.  row_stats as above;
 * diag_out (optional) receives S_ii = |P_i|^2 / t, what SupConLoss1's unit-norm assertion looks at.
 * ws: cy_supcon_fused_ws_bytes(n, D) bytes, the same buffer for both calls. */
size_t cy_supcon_fused_ws_bytes(int n, int D);
int cy_supcon_fused_fwd(const float* P, const int32_t* labels, const uint8_t* pos_mask, float* loss,
                        float* row_stats, float* diag_out, void* ws, size_t ws_bytes, int n, int D, float t,
                        void* stream);
int cy_supcon_fused_bwd(const float* P, const int32_t* labels, const uint8_t* pos_mask, const float* row_stats,
                        const float* gscale, float* dP, void* ws, size_t ws_bytes, int n, int D, float t,
                        void* stream);
int cy_supcon_matrices(const float* S, const float* row_stats, const int32_t* labels,
                       const uint8_t* pos_mask, float* sim_logits, float* sim_exp,
                       float* pos_out, float* neg_out, int n, void* stream);
/* SelfPacedSupConLoss (losses/contrastive.py:103-212) on the tile machinery of the fused entries above: the loss of
 * cy_supcon_fused_fwd with every positive pair weighted by a constant w_ij of its own negative log-likelihood,
 *   llh_ij = (S_ij - M) - log D_i,  l_ij = -llh_ij,  D_i = sum_{k != i, pos or neg} E_ik + 1e-16,  c_i = |pos(i)|
 *   w_ij = [l_ij <= gamma] (soft == 0)  or  max(1 - l_ij / gamma, 0) (soft != 0)
 *   loss = -(1/R) sum_i (1/c_i) sum_{pos} w_ij llh_ij;   ratio = sum_{pos} w_ij / sum_i c_i
 *   correct_grad != 0 and ratio > 0: loss / ratio, the ratio a constant of the gradient
 * w needs the finished D_i: two passes over the tiles (row sums, then the weighted sums), S never written.
 *   row_stats f32 [R][4] = (D_i, c_i, W_i = sum_{pos} w_ij, M);  aux f32 [4] = (loss, ratio, scale, sum_i c_i) with
 *   scale = 1 / ratio or 1: what the backward multiplies the upstream gradient with.  diag_out as above (optional).
 * backward: dP = (1/t)(G + G^T) P,  G_ij = -(gscale[0] scale / R) [pos_ij w_ij / c_i - in_ij E_ij W_i / (c_i D_i)],
 * the weights recomputed from row_stats exactly as the forward formed them.
 * Checked before any launch: NULL P, outputs or ws, or labels and pos_mask both NULL -> CY_ERR_ARG; n <= 0, D <= 0,
 * D > 256, D % 8, !(t > 0), !(gamma > 0) -> CY_ERR_SHAPE; a short workspace -> CY_ERR_WORKSPACE.  Fixed summation
 * orders: two runs give the same bits.  ws: cy_supcon_sp_ws_bytes(n, D) bytes (0 where n or D is refused), one size
 * for both calls as with cy_supcon_fused_ws_bytes: diag[R] + M[4] + max(ns R 5, ns R D) floats for ns column splits.
 * The forward uses the first R + 4 + ns R 5 of them (0.4 MB at R = 4096, where the query answers 16 MiB for the
 * backward's [ns][R][D] partials); a caller that keeps one buffer for both directions allocates once. */
size_t cy_supcon_sp_ws_bytes(int n, int D);
int cy_supcon_sp_fwd(const float* P, const int32_t* labels, const uint8_t* pos_mask, float* aux, float* row_stats,
                     float* diag_out, void* ws, size_t ws_bytes, int n, int D, float t, float gamma, int soft,
                     int correct_grad, void* stream);
int cy_supcon_sp_bwd(const float* P, const int32_t* labels, const uint8_t* pos_mask, const float* row_stats,
                     const float* aux, const float* gscale, float* dP, void* ws, size_t ws_bytes, int n, int D, float t,
                     float gamma, int soft, void* stream);
/* f32 GEMM on the f32 MFMA: C[M][N] = alpha * A[M][K] * op(B); b_trans=1: B is
 * [N][K] (C = A B^T), b_trans=0: B is [K][N]. */
int cy_sgemm(const float* A, const float* B, float* C, int M, int N, int K, float alpha,
             int b_trans, void* stream);

/* ------------------------------------------------------------------------
 * In-step affine augmentation (semi_seg/augment.py:297-311, configured at
 * semi_seg/epochers/epocher.py:226-238; third-party `rising`, un-vendored):
 * nearest-neighbour resampling with a per-sample 2x3 matrix theta (f32 [N][6],
 * output-normalised -> input-normalised coordinates, align_corners=False,
 * zero padding) and optional gamma x**g (g f32[N], NULL = none) applied
 * BEFORE the geometry as the reference does for mode="image".
 * Tensors are NHWC of `dtype` (an [N,1,H,W] image is its own NHWC view).
 * ------------------------------------------------------------------------ */
int cy_affine_nearest_fwd(const void* x, void* out, const float* theta, const float* gamma, int N,
                          int C, int H, int W, int dtype, void* stream);
/* dx = gather-form adjoint (deterministic, no atomics). */
int cy_affine_nearest_bwd(const void* dout, void* dx, const float* theta, int N, int C, int H,
                          int W, int dtype, void* stream);

/* ------------------------------------------------------------------------
 * Segmentation metric helper: per-sample per-class intersection/union counts
 * of argmax(logits) vs target (contrastyou/meters/general_dice_meter.py:
 * 37-72,93-110).  counts is int64 [N][K][2] = {intersection, union}.
 * ------------------------------------------------------------------------ */
int cy_dice_counts(const float* logits, const int64_t* target, int64_t* counts, int N, int HW,
                   int K, void* stream);

/* ------------------------------------------------------------------------
 * Mean-teacher / consistency hooks (semi_seg/hooks/mt.py:49-82,
 * semi_seg/hooks/consistency.py:22-38)
 * ------------------------------------------------------------------------ */
/* teacher = (alpha*teacher + (1-alpha)*student) * (1 - weight_decay) over a
 * flat f32 buffer of n elements. */
int cy_ema_update(float* teacher, const float* student, long n, float alpha, float weight_decay,
                  void* stream);
/* loss = mean((softmax(a)-softmax(b))^2) over [npix][K] f32 logits, 1 <= K <= 64 (K > 16: the sixteen-lanes-per-pixel
 * form of csrc/cy_group_loss.hip; CY_ERR_SHAPE above 64) */
size_t cy_softmax_mse_ws_bytes(long npix);
int cy_softmax_mse_fwd(const float* a, const float* b, float* loss, long npix, int K, void* ws,
                       size_t ws_bytes, void* stream);
/* da (and db if not NULL) = gscale[0] * dloss/d{a,b} */
int cy_softmax_mse_bwd(const float* a, const float* b, const float* gscale, float* da, float* db,
                       long npix, int K, void* stream);

/* ------------------------------------------------------------------------
 * Multi-prototype ("multicore") supervised loss and metric (csrc/cy_group_loss.hip; entries added to ABI v15 -- no
 * existing signature changed, so cy_abi_version() stays 15).  The network has K = G * m outputs, class g owns the
 * contiguous channels [g*m, (g+1)*m) (the reference's `grouper(range(K), G)`).  Logits are [npix][K] f32 (NHWC),
 * 1 <= K <= 64, labels int64 in [0, G).  Every entry checks its arguments before any launch: a NULL pointer or a
 * count < 1 -> CY_ERR_ARG; K outside 1..64, G < 1 or K % G != 0 -> CY_ERR_SHAPE; a short workspace ->
 * CY_ERR_WORKSPACE.  K <= 16 runs one thread per pixel, 16 < K <= 64 sixteen lanes per pixel.
 * ------------------------------------------------------------------------ */
/* MultiCoreKL(groups)(softmax(logits), one_hot(target)) (contrastyou/losses/multicore_loss.py:41-60):
 *   P_p = sum_{k in group(t_p)} softmax(z_p)_k;  loss = mean_p -log((P_p + eps) / (1 + eps))
 * Workspace: one f64 partial per block = 8 * min(1024, ceil(npix / P)) bytes, P = 256 pixels per block for K <= 16 and
 * 16 for K > 16; the partials are summed in a fixed order (two runs give the same bits). */
size_t cy_softmax_group_kl_ws_bytes(long npix, int K);
int cy_softmax_group_kl_fwd(const float* logits, const int64_t* target, float* loss, long npix, int K, int G,
                            float eps, void* ws, size_t ws_bytes, void* stream);
/* dlogits_k = -(gscale[0]/npix) * p_k * ([k in group(t)] - P) / (P + eps)  (gscale: device scalar, upstream grad) */
int cy_softmax_group_kl_bwd(const float* logits, const int64_t* target, const float* gscale, float* dlogits,
                            long npix, int K, int G, float eps, void* stream);
/* UniversalDice counts of `reduced_simplex(softmax(logits)).max(1)[1]` against the target
 * (semi_seg/epochers/features/multicore_epocher.py:37-39,64-67,84-91): counts is int64 [N][G][2] = {intersection,
 * union}; the predicted class is the first maximal group sum of exp(z - max z). */
int cy_group_dice_counts(const float* logits, const int64_t* target, int64_t* counts, int N, int HW, int K, int G,
                         void* stream);

/* ------------------------------------------------------------------------
 * Adaptive over-segmented criteria: the K prototypes are mixed into C true classes by a dense matrix
 * (csrc/cy_mix_loss.hip; entries added to ABI v15 -- no existing signature changed, so cy_abi_version() stays 15).
 * Logits are [npix][K] f32 (NHWC), 1 <= K <= 64; labels int64 in [0, C), 1 <= C <= 16; `mix` is a dense [K][C] f32
 * matrix, row-major, of arbitrary non-negative numbers (the criteria pass softmax(translation matrix, 1); it need not be
 * row-stochastic).  With p = softmax(z), R_c = sum_k p_k mix[k][c] and P = npix:
 *   loss       = (1/P) sum_pix -log((R_t + eps) / (1 + eps))
 *   dlogits_k  = -(gscale[0]/P) * p_k * (mix[k][t] - R_t) / (R_t + eps)
 *   dmix[k][c] = -(gscale[0]/P) * sum_{pix : t = c} p_k / (R_t + eps)
 * (AdaptiveOverSegmentedLoss and its stricter variants, contrastyou/losses/multicore_loss.py:63-149.)
 * Every entry checks its arguments before any launch: a NULL pointer (except `dmix`, and `ws` of the backward pass
 * when dmix is NULL) or a count < 1 -> CY_ERR_ARG; K outside 1..64 or C outside 1..16 -> CY_ERR_SHAPE; a short
 * workspace -> CY_ERR_WORKSPACE.  No floating-point atomics: every sum runs in a fixed order, two runs give the same
 * bits.
 * ------------------------------------------------------------------------ */
/* Forward, two launches.  Workspace as cy_softmax_group_kl_ws_bytes: 8 * min(1024, ceil(npix / P)) bytes, P = 256 for
 * K <= 16 and 16 above. */
size_t cy_softmax_mix_kl_ws_bytes(long npix, int K);
int cy_softmax_mix_kl_fwd(const float* logits, const int64_t* target, const float* mix, float* loss, long npix, int K,
                          int C, float eps, void* ws, size_t ws_bytes, void* stream);
/* Backward.  dmix == NULL: one launch, dlogits only, ws and ws_bytes are not looked at.  Otherwise two launches: every
 * block leaves a [K][C] f32 partial in ws and a second launch sums the blocks;
 * ws_bytes >= 4 * K * C * min(1024, ceil(npix / 16)) = cy_softmax_mix_kl_bwd_ws_bytes (0 for a count < 1).
 * dlogits has the same bits with and without dmix. */
size_t cy_softmax_mix_kl_bwd_ws_bytes(long npix, int K, int C);
int cy_softmax_mix_kl_bwd(const float* logits, const int64_t* target, const float* mix, const float* gscale,
                          float* dlogits, float* dmix, long npix, int K, int C, float eps, void* ws, size_t ws_bytes,
                          void* stream);
/* UniversalDice counts of the reduced arg-max: counts is int64 [N][C][2] = {intersection, union}; the predicted class is
 * the first maximal c of sum_k exp(z_k - max z) * mix[k][c] (no division). */
int cy_mix_dice_counts(const float* logits, const int64_t* target, const float* mix, int64_t* counts, int N, int HW,
                       int K, int C, void* stream);

/* ------------------------------------------------------------------------
 * Pixel-wise regularisers of the semi-supervised baselines (csrc/cy_pixel_reg.hip; entries added to ABI v15 -- no
 * existing signature changed, so cy_abi_version() stays 15).  Logits are [npix][K] f32 (NHWC), 2 <= K <= 16.  Every entry checks its arguments before any launch: a NULL pointer,
 * npix < 1 or K outside 2..16 -> CY_ERR_ARG; a short workspace -> CY_ERR_WORKSPACE.  Forward: two launches (one
 * f64 partial per block into ws; one-block sum in a fixed order -- two runs give the same bits); backward: one
 * launch, scaled by the device scalar gscale[0].
 * ------------------------------------------------------------------------ */
/* Entropy(reduction="mean", eps)(softmax(logits, 1)) (semi_seg/hooks/entmin.py:29-30, contrastyou/losses/kl.py:48-56):
 * loss = mean_pix -sum_k p_k log(p_k + eps).  A p_k that underflows to 0 adds 0 to both passes. */
size_t cy_softmax_entropy_ws_bytes(long npix);
int cy_softmax_entropy_fwd(const float* logits, float* loss, long npix, int K, float eps, void* ws, size_t ws_bytes,
                           void* stream);
int cy_softmax_entropy_bwd(const float* logits, const float* gscale, float* dlogits, long npix, int K, float eps,
                           void* stream);
/* MSELoss()(softmax(logits, 1), one_hot(argmax)) (semi_seg/hooks/pseudolabel.py:30-36): the arg-max is taken over the
 * logits, first maximal index on ties; the one-hot is a constant of the gradient and is never written. */
size_t cy_softmax_selfmse_ws_bytes(long npix);
int cy_softmax_selfmse_fwd(const float* logits, float* loss, long npix, int K, void* ws, size_t ws_bytes,
                           void* stream);
int cy_softmax_selfmse_bwd(const float* logits, const float* gscale, float* dlogits, long npix, int K, void* stream);
/* UA-MT (semi_seg/hooks/mt.py:242-248,266-267): t = softmax(teacher), m = [-sum t log(t + 1e-16) < thr],
 * tau = t or (hard != 0) one_hot(argmax teacher), e = mean_k (tau_k - softmax(student)_k)^2;
 * result[0] = mean(m e) / (mean(m) + 1e-2), result[1] = mean(m).  The backward writes the student's gradient only
 * and reads mean(m) from `result`: the denominator is a constant, as through the reference's .item(). */
size_t cy_uamt_mse_ws_bytes(long npix);
int cy_uamt_mse_fwd(const float* teacher, const float* student, float* result, long npix, int K, float thr, int hard,
                    void* ws, size_t ws_bytes, void* stream);
int cy_uamt_mse_bwd(const float* teacher, const float* student, const float* result, const float* gscale,
                    float* dstudent, long npix, int K, float thr, int hard, void* stream);

/* ------------------------------------------------------------------------
 * Supervised criteria on the segmentation output (csrc/cy_seg_loss.hip; entries added to ABI v18): class-weighted KL_div with any reduction
 * (contrastyou/losses/kl.py:94-125, the criterion of semi_seg/epochers/epocher.py:317-318) and the soft Dice loss
 * (contrastyou/losses/dice_loss.py:46-105), both of softmax(logits) against integer labels.  Logits are [npix][K] f32
 * (NHWC), labels int64 in [0, K), 1 <= K <= 16.  Every entry checks its arguments before any launch: a NULL pointer
 * (`weight` alone may be NULL) or a count < 1 -> CY_ERR_ARG; K outside 1..16 -> CY_ERR_SHAPE; a short workspace ->
 * CY_ERR_WORKSPACE.  No atomics: two runs give the same bits.  Upstream gradients are device memory, never host scalars.
 * ------------------------------------------------------------------------ */
/* l_pix = -w[y] log((softmax(z)_y + eps) / (1 + eps)), w = weight [K] or all ones for NULL (the normalised weights
 * w / sum(w) * K of kl.py:108); the other classes add exactly 0.
 * cy_softmax_wkl_fwd: loss[0] = sum_pix l_pix / denom (denom = npix for "mean", 1 for "sum"; denom > 0).  Two launches:
 * one f64 partial per block into ws, then a one-block sum in block order.
 * ws_bytes >= 8 * min(1024, ceil(npix / 256)) = cy_softmax_wkl_ws_bytes(npix).
 * cy_softmax_wkl_map_fwd: map[pix] = l_pix (reduction "none"), one launch, no workspace. */
size_t cy_softmax_wkl_ws_bytes(long npix);
int cy_softmax_wkl_fwd(const float* logits, const int64_t* target, const float* weight, float* loss, long npix, int K,
                       float eps, double denom, void* ws, size_t ws_bytes, void* stream);
int cy_softmax_wkl_map_fwd(const float* logits, const int64_t* target, const float* weight, float* map, long npix,
                           int K, float eps, void* stream);
/* dz_k = G w[y] (-p_y / (p_y + eps)) (delta_ky - p_k); G = gscale[0] / denom, or dmap[pix] for the map form.  One
 * launch each. */
int cy_softmax_wkl_bwd(const float* logits, const int64_t* target, const float* weight, const float* gscale,
                       float* dlogits, long npix, int K, float eps, double denom, void* stream);
int cy_softmax_wkl_map_bwd(const float* logits, const int64_t* target, const float* weight, const float* dmap,
                           float* dlogits, long npix, int K, float eps, void* stream);
/* Soft Dice of p = softmax(z) per image n (npix = N * HW, image n is pixels [n HW, (n+1) HW)) and class c:
 *   A = sum_pix p_c [y = c], B = sum_pix p_c^P (P = 1 or 2), T = #{pix: y = c};
 *   num = A + smooth, den = B + T + smooth, L_nc = 1 - num / den (no factor 2, dice_loss.py:57-60).
 * reduction 0 "mean": result[0] = (1/K) sum_{c != ignore} mean_n L_nc; 1 "sum": sum_n; 2 "none": result[n], n < N.
 * The divisor K counts the ignored class (dice_loss.py:105); an `ignore` outside [0, K) ignores nothing.
 * Two launches: N x B blocks, B = min(ceil(HW / 256), max(1, 1024 / N)) per image (integer division; a block never
 * spans two images), each writing K {A, B} f64 pairs and K int64 counts into ws; then one block adds them in block order
 * and writes `table`, f64 [N][K][2] = {num, den} (the ignored class included), which the backward reads, and `result`.
 * ws_bytes >= 24 * N * B * K = cy_softmax_dice_ws_bytes(N, HW, K) (0 for a count < 1 or K outside 1..16).
 * P outside {1, 2} or reduction outside 0..2 -> CY_ERR_ARG. */
size_t cy_softmax_dice_ws_bytes(int N, long HW, int K);
int cy_softmax_dice_fwd(const float* logits, const int64_t* target, void* table, float* result, int N, long HW, int K,
                        int P, double smooth, int ignore, int reduction, void* ws, size_t ws_bytes, void* stream);
/* dloss/dp_c = g_c = (G_n r / K) (-[y = c] / den + num P p_c^(P-1) / den^2) for c != ignore, 0 otherwise; r = 1/N for
 * "mean", 1 otherwise; G_n = gup[0], or gup[n] for "none".  dz_k = p_k (g_k - sum_j p_j g_j).  One launch. */
int cy_softmax_dice_bwd(const float* logits, const int64_t* target, const void* table, const float* gup,
                        float* dlogits, int N, long HW, int K, int P, int ignore, int reduction, void* stream);

/* ------------------------------------------------------------------------
 * RAdam step over a flat f32 parameter buffer (torch.optim.RAdam semantics,
 * contrastyou/trainer/base.py:66-75, config/base.yaml:10-13).
 * `step` is the 1-based step count AFTER this update.
 * ------------------------------------------------------------------------ */
int cy_radam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n,
                  float lr, float beta1, float beta2, float eps, float weight_decay, long step,
                  void* stream);

/* ------------------------------------------------------------------------
 * Dense (pixel-wise) contrastive projector
 * (contrastyou/projectors/heads.py:31-41,99-123: Conv1x1(C,hid) -> LeakyReLU ->
 * Conv1x1(hid,out) -> AdaptiveAvgPool2d((sh,sw)) -> L2 norm) and point
 * sampling (semi_seg/hooks/infonce.py:31-46).
 * The second 1x1 conv commutes with the average pool, so the fused kernel
 * produces  hpool[bin][hid] = mean over the bin's pixels of
 * lrelu(W1 x + b1)  straight from the NHWC feature map x [N][H][W] (pixel
 * stride ldx, dtype); the [bins][hid] x [hid][out] product and the
 * normalisation use cy_linear_* / cy_l2norm_*.
 * bins: int32 [nb][3] = (image, bin row, bin col), distinct; NULL = all
 * N*sh*sw bins in row-major order.  Bin extents follow torch's adaptive
 * pooling: rows [floor(i*H/sh), ceil((i+1)*H/sh)).  Requires sh<=H, sw<=W.
 * ------------------------------------------------------------------------ */
int cy_dense_proj_fwd(const void* x, const float* w1, const float* b1, const int32_t* bins, int nb,
                      float* hpool, int N, int H, int W, int C, int ldx, int hid, int sh, int sw,
                      float slope, int dtype, void* stream);
size_t cy_dense_proj_bwd_ws_bytes(int nb, int C, int hid);
/* dx (dtype, NHWC, ldx) is ACCUMULATED into (zero it first; may be NULL);
 * dw1 [hid][C], db1 [hid] f32, written or accumulated; hid <= 256. */
int cy_dense_proj_bwd(const void* x, const float* w1, const float* b1, const int32_t* bins, int nb,
                      const float* dhpool, void* dx, float* dw1, float* db1, int accumulate, int N,
                      int H, int W, int C, int ldx, int hid, int sh, int sw, float slope, int dtype,
                      void* ws, size_t ws_bytes, void* stream);
/* cy_dense_proj_plan (host side, no GPU needed) is the rule cy_dense_proj_fwd, cy_dense_proj_bwd and
 * cy_dense_proj_bwd_ws_bytes follow when they choose their kernels.
 * The matrix-core forms take 16-bit maps, 128 or 256 hidden units and slope <= 1: C = 32, 64, 128 the register-resident
 * form, C = 256, 512 the streamed form (forward and dx; its dW1 / db1 run the VALU kernel: one pass); everything else, and every call when CY_DENSE_MFMA=0 is set (read once per
 * process), runs the VALU kernels.  out == NULL -> CY_ERR_ARG; C < 1, C % 8 != 0 or hid < 1 -> CY_ERR_SHAPE; an
 * unknown dtype -> CY_ERR_DTYPE. */
#define CY_DENSE_PROJ_VALU 0        /* any dtype, any C % 8 == 0 */
#define CY_DENSE_PROJ_MFMA_REG 1    /* pixel rows and W1 resident in registers / static LDS */
#define CY_DENSE_PROJ_MFMA_STREAM 2 /* forward, dx: accumulator resident, rows streamed, W1 in dynamic LDS per pass */
typedef struct cy_dense_proj_plan_t {
  int32_t form;              /* kernel form (CY_DENSE_PROJ_*) */
  int32_t channel_blocks;    /* channel blocks of 32 (VALU: staged chunks) */
  int32_t fwd_passes;        /* passes over the hidden units of the forward kernel */
  int32_t dw_passes;         /* ... of the dW1 kernel */
  int32_t lds_bytes;         /* dynamic LDS bytes (the largest of the three kernels'; <= 160 KiB) */
  int32_t bwd_launches;      /* launches of a backward with all bins that asks for dx and the parameter gradients */
  int32_t bwd_launches_list; /* ... with a bin list */
  int32_t w1_image_in_ws;    /* 1 when the dx kernel reads W1 from a 16-bit image in the workspace (hid * C * 2 bytes
                                behind the partials and the job table, counted by cy_dense_proj_bwd_ws_bytes), else 0 */
} cy_dense_proj_plan_t;
int cy_dense_proj_plan(int C, int hid, int dtype, float slope, cy_dense_proj_plan_t* out);
/* nn.AdaptiveAvgPool2d((sh,sw)) on an NHWC map -> f32 [nb][C] (same bin list
 * convention); backward for the all-bins case (gather form, deterministic). */
int cy_adaptive_avgpool_fwd(const void* x, const int32_t* bins, int nb, float* out, int N, int H,
                            int W, int C, int ldx, int sh, int sw, int dtype, void* stream);
int cy_adaptive_avgpool_bwd(const float* dpool, void* dx, int N, int H, int W, int C, int ldx,
                            int sh, int sw, int dtype, void* stream);
/* nn.AdaptiveMaxPool2d(size) (projectors/nn.py:16-23: pool_name="adaptive_max" of both projection heads) on an NHWC map:
 * out [N*sh*sw][C] f32 and arg [N*sh*sw][C] = pixel index (inside the image) of the first maximum in row-major order;
 * backward in gather form (bins may overlap: deterministic, no atomics). */
int cy_adaptive_maxpool_fwd(const void* x, float* out, int32_t* arg, int N, int H, int W, int C, int ldx, int sh,
                            int sw, int dtype, void* stream);
int cy_adaptive_maxpool_bwd(const float* dpool, const int32_t* arg, void* dx, int N, int H, int W, int C, int ldx,
                            int sh, int sw, int dtype, void* stream);
/* out[m][:] = src[idx[m]][:] (f32 rows of length D); backward scatters rows
 * (idx distinct). */
int cy_gather_rows_fwd(const float* src, const int32_t* idx, float* out, int M, int D,
                       void* stream);
int cy_gather_rows_bwd(const float* dout, const int32_t* idx, float* dsrc, int M, int D,
                       void* stream);

/* ------------------------------------------------------------------------
 * Cluster heads and discrete mutual-information losses
 * (contrastyou/projectors/heads.py:44-78,125-173; contrastyou/losses/discreteMI.py:
 * 90-170,201-261).  Probability maps are NHWC f32 [N][H][W][k], k <= 64.
 * ------------------------------------------------------------------------ */
/* ------------------------------------------------------------------------
 * Stacked cluster heads in one pass (DenseClusterHead / ClusterHead, head_type="linear",
 * projectors/heads.py:125-173): probs[S][M][k] = softmax over each sub-head's k of (W x + b) / T with
 * K = S*k <= 128 outputs and C in {32, 64} inputs, rows x[M][C] (bf16 / f16 / f32, NHWC pixels); exact f32
 * MFMA; the logits are never written.  Backward from (probs, dprobs): dx[M][C] (dtype of x; NULL: skipped),
 * dw[K][C], db[K] (NULL: skipped; ws from cy_cluster_head_bwd_ws_bytes).
 * ------------------------------------------------------------------------ */
int cy_cluster_head_fwd(const void* x, const float* w, const float* b, float* probs, long M, int C, int K, int S,
                        int k, float invT, int dtype, void* stream);
size_t cy_cluster_head_bwd_ws_bytes(long M, int C);
int cy_cluster_head_bwd(const void* x, const float* w, const float* probs, const float* dprobs, void* dx, float* dw,
                        float* db, long M, int C, int K, int S, int k, float invT, int dtype, void* ws,
                        size_t ws_bytes, void* stream);
/* Launch shape of the two kernels above (ABI v16; host-side only, launches nothing; CY_ERR_SHAPE as the launches). */
typedef struct cy_cluster_plan {
  int32_t fwd_waves;  /* 8 where eight waves' tiles fit the LDS next to the weights, else 4 */
  int32_t fwd_grid;   /* blocks, at most 256 */
  int32_t fwd_trips;  /* the most 32-pixel tiles a wave takes */
  int32_t bwd_grid;   /* blocks of four waves, at most 512 */
  int32_t bwd_trips;
  int32_t slabs;      /* per-wave dW / db slabs in the workspace */
} cy_cluster_plan;
int cy_cluster_head_plan(long M, int C, int S, int k, cy_cluster_plan* out);

/* logits [M][S*k] -> probs [S][M][k] = softmax(logits*invT) within each of the
 * S sub-heads (SoftmaxWithT, projectors/nn.py:35-44); S=1 is a row softmax. */
int cy_group_softmax_fwd(const float* logits, float* probs, long M, int S, int k, float invT,
                         void* stream);
int cy_group_softmax_bwd(const float* probs, const float* dprobs, float* dlogits, long M, int S,
                         int k, float invT, void* stream);
/* J[T*T][k][k], T = 2*pad+1:  J[(u,v)][i][j] = scale * sum_{n,a,b}
 * x1[n][a+u-pad][b+v-pad][i] * x2[n][a][b][j] (zero outside the image);
 * scale = 1/(N*H*W) if normalise else 1.  pad=0, normalise=1 is
 * compute_joint_2D_with_padding_zeros; pad>0 is the F.conv2d of
 * compute_joint_2D; H=W=1 gives compute_joint on [N][k] vectors. */
size_t cy_joint_ws_bytes(int N, int H, int W, int k, int pad);
int cy_joint_fwd(const float* x1, const float* x2, float* J, int N, int H, int W, int k, int pad,
                 int normalise, void* ws, size_t ws_bytes, void* stream);
/* dx1, dx2 (either may be NULL) = gscale[0] * adjoint of cy_joint_fwd applied to dJ */
int cy_joint_bwd(const float* x1, const float* x2, const float* dJ, const float* gscale, float* dx1,
                 float* dx2, int N, int H, int W, int k, int pad, int normalise, void* stream);
/* Launch plans of the information-loss kernels (ABI v17).  Host-side only, they launch nothing and need no GPU.
 * cy_joint_fwd, cy_joint_bwd, cy_joint_ws_bytes and the two softmax launches take every decision from these two
 * functions, and refuse exactly what they refuse.
 * Joints (compute_joint / compute_joint_2D / compute_joint_2D_with_padding_zeros, contrastyou/losses/discreteMI.py:
 * 201-261): 1 <= k <= 64, 0 <= pad < min(H, W), forward and backward alike (CY_ERR_SHAPE otherwise). */
typedef struct cy_joint_plan_t {
  int32_t fwd_kernel;   /* 0: joint_fwd_kernel, 64-pixel tiles, one displacement per blockIdx.y (pad 0, and pad > 0 where
                           the staged rows exceed 150 KB of LDS); 1: joint_fwd_multi_kernel, R image rows per tile, up to
                           nine displacements per blockIdx.y */
  int32_t fwd_vec;      /* 1: the tile is staged with 16-byte copies (k % 4 == 0; kernel 0: and pad 0), 0: scalar */
  int32_t kp;           /* k rounded up to 4: the row pitch of the staged tiles */
  int32_t nsl;          /* pixel slices per block: 256 / (kp/4)^2 */
  int32_t idle;         /* threads that own no slice: 256 - nsl * (kp/4)^2 */
  int32_t R;            /* kernel 1: image rows per tile, min(H, max(1, 256 / W)); kernel 0: 0 */
  int32_t tiles_h;      /* kernel 1: ceil(H / R); kernel 0: 0 */
  int32_t ntile;        /* tiles in all: kernel 1 N * tiles_h (a block walks them with stride nblk), kernel 0
                           ceil(npix / 64) */
  int32_t nblk;         /* blocks in x = partial joints per displacement: min(2048, ceil(npix / 1024)) */
  int32_t per;          /* kernel 0: pixels per block, a multiple of 64 (the last block takes what is left); kernel 1: 0 */
  int32_t grid_y;       /* kernel 0: T*T; kernel 1: ceil(T*T / 9) */
  int32_t nd_last;      /* displacements of the last blockIdx.y: T*T - 9 * (grid_y - 1) on kernel 1, 1 on kernel 0 */
  int32_t fwd_lds;      /* dynamic LDS bytes of the forward launch */
  int32_t reduce_trips; /* partial blocks each of the 64 slices of joint_reduce_kernel adds per element: ceil(nblk/64) */
  int32_t bwd_kernel;   /* 1: joint_bwd4_kernel (k % 4 == 0), 0: joint_bwd_kernel */
  int32_t bwd_grid;     /* blocks, at most 8192 */
  int32_t bwd_trips;    /* trips of the backward's grid-stride loop */
  int32_t bwd_lds;      /* dynamic LDS bytes: bwd_dchunk * k * k * 4 <= 64 KB */
  int32_t bwd_dchunk;   /* displacements of dJ staged at a time: min(T*T, 65536 / (4 k^2)) */
  int32_t bwd_nchunk;   /* ceil(T*T / bwd_dchunk); 1 = staged once per block */
} cy_joint_plan_t;
int cy_joint_plan(int N, int H, int W, int k, int pad, cy_joint_plan_t* out);
/* Grouped softmax (SoftmaxWithT, contrastyou/projectors/nn.py:35-44): S*k <= 255 in both directions, CY_ERR_SHAPE
 * beyond (from the plan and from both launches, before anything is launched). */
typedef struct cy_group_softmax_plan_t {
  int32_t fwd_rows; /* rows of logits per block: 64 */
  int32_t fwd_grid;
  int32_t fwd_lds;  /* fwd_rows * (S*k + 1) * 4 */
  int32_t fwd_ok;   /* 1: fwd_lds fits 64 KB */
  int32_t bwd_rows; /* 64 where the two tiles fit 64 KB (S*k <= 127), else 32 */
  int32_t bwd_grid;
  int32_t bwd_lds;  /* 2 * bwd_rows * (S*k + 1) * 4 */
  int32_t bwd_ok;
} cy_group_softmax_plan_t;
int cy_group_softmax_plan(long M, int S, int k, cy_group_softmax_plan_t* out);
/* loss on a joint.  mode 0: IIDSegmentationLoss padding 0; mode 1: padding>0
 * (subtract min, +1e-8, per-displacement and global normalisation, loss/T^2);
 * mode 2: IIDLoss on vectors (symmetrise if `symmetric`, normalise to 1).
 * out2[0] = loss(lamda), out2[1] = loss(lamda=1); P (may be NULL) = the
 * normalised joint; dJ (may be NULL) = dloss/dJ. */
size_t cy_iid_loss_ws_bytes(int TT, int k);
int cy_iid_loss(const float* J, float* out2, float* P, float* dJ, int TT, int k, int mode,
                int symmetric, float lamda, float eps, void* ws, size_t ws_bytes, void* stream);
/* Patch-wise IIC (IIDSegmentationSmallPathLoss / patch_generator, contrastyou/losses/discreteMI.py:173-198,264-272;
 * entries added to ABI v18).  The maps are cut into square patches
 * of side `patch` with step patch / 2: the origins along an axis of length L are 0, s, 2s, ... below L - patch, then
 * max(L - patch, 0); every patch is clipped to the map, so all P = nph * npw patches have the same extents eh x ew =
 * min(patch, H) x min(patch, W).  Patch q = ih * npw + iw.  With d = (du+pad)*T + (dv+pad), T = 2 pad + 1:
 *   J[q][d][i][j] = scale * sum_n sum_{(h,w) in q, (h+du,w+dv) in q} x1[n][h+du][w+dv][i] * x2[n][h][w][j]
 * -- the zero padding is at the PATCH border, not the image border -- scale = 1/(N eh ew) if normalise else 1.
 * Checked before any launch: a NULL pointer, a size < 1 or an unknown `kernel` -> CY_ERR_ARG; k outside 1..64, pad < 0,
 * patch < 2, pad >= min(eh, ew), more than 65535 patches, J of 2^31 elements or more, or a forced staged kernel whose
 * tile exceeds 150 KB of LDS ->
 * CY_ERR_SHAPE; a short workspace -> CY_ERR_WORKSPACE.  No atomics anywhere: two runs give the same bits.
 * cy_joint_patch_plan (host-side only, launches nothing) writes the launch rule; `kernel` = -1 asks for the rule's
 * choice of forward kernel, 0 / 1 force one.
 * cy_joint_patch_ws_bytes = 4 P T*T k*k nbx, the partial joints of that `kernel`, or 16 with nbx = 1 (0 where the sizes
 * are refused). */
typedef struct cy_joint_patch_plan_t {
  int32_t P, nph, npw; /* the patches, and their rows and columns */
  int32_t eh, ew;      /* the extents of every patch */
  int32_t fwd_kernel;  /* 1 = a block owns (patch, group of <= 9 displacements) and walks the (image, R patch rows) tiles
                          staged in LDS with their zero border; 0 = one displacement per block, 64-pixel tiles,
                          bounds-tested reads (where the staged tile exceeds 150 KB) */
  int32_t R;           /* min(eh, max(1, 256 / ew)) (kernel 1; else 0) */
  int32_t tiles_h;     /* ceil(eh / R) (kernel 1; else 0) */
  int32_t ntile;       /* tiles: N * tiles_h (kernel 1), ceil(N eh ew / 64) (kernel 0) */
  int32_t nbx;         /* blocks per (patch, group) = partial joints: kernel 1 min(tiles, ceil(1024 / (P * groups))),
                          kernel 0 min(2048, ceil(N eh ew / 1024)); 1 = the forward writes J itself and no reduction is
                          launched */
  int32_t grid_y;      /* gridDim.y: ceil(T*T / 9) (kernel 1), T*T (kernel 0) */
  int32_t fwd_lds;     /* dynamic LDS bytes */
  int32_t fwd_vec;     /* 16-byte staging (k % 4 == 0) */
  int32_t staged_fits; /* 1 if the staged tile fits */
  int32_t bwd_kernel;  /* 1 = four channels per thread (k % 4 == 0) */
  int32_t bwd_grid;    /* the backward's grid */
} cy_joint_patch_plan_t;
int cy_joint_patch_plan(int N, int H, int W, int k, int pad, int patch, int kernel, cy_joint_patch_plan_t* out);
size_t cy_joint_patch_ws_bytes(int N, int H, int W, int k, int pad, int patch, int kernel);
int cy_joint_patch_fwd(const float* x1, const float* x2, float* J, int N, int H, int W, int k, int pad, int patch,
                       int normalise, int kernel, void* ws, size_t ws_bytes, void* stream);
/* The loss of cy_iid_loss (mode 0 or 1, never symmetric) on each of the P joints J[P][TT][k][k], one block per patch:
 * losses[q]; Pj (may be NULL) [P][TT][k][k] the final joints; dJ (may be NULL) = (1/P) dlosses[q]/dJ[q];
 * loss[0] = mean_q losses[q] in a fixed order.  ws_bytes >= P * cy_iid_loss_ws_bytes(TT, k). */
size_t cy_iid_patch_loss_ws_bytes(int P, int TT, int k);
int cy_iid_patch_loss(const float* J, float* loss, float* losses, float* Pj, float* dJ, int P, int TT, int k, int mode,
                      float lamda, float eps, void* ws, size_t ws_bytes, void* stream);
/* dx1, dx2 [N][H][W][k] (either may be NULL) = gscale[0] * adjoint of cy_joint_patch_fwd applied to dJ[P][T*T][k][k], in
 * gather form: every pixel adds its patches in ascending q, then the displacements valid inside that patch. */
int cy_joint_patch_bwd(const float* x1, const float* x2, const float* dJ, const float* gscale, float* dx1, float* dx2,
                       int N, int H, int W, int k, int pad, int patch, int normalise, void* stream);

/* ------------------------------------------------------------------------
 * PICA losses, Jensen-Shannon divergence, entropy prior (csrc/cy_pica.hip; entries added to ABI v18 -- no existing
 * signature changed and no struct added).  Every entry checks its arguments before any launch: a NULL required pointer
 * or a count < 1 -> CY_ERR_ARG; classes outside 1..64 or maps outside 2..8 -> CY_ERR_SHAPE; a short workspace ->
 * CY_ERR_WORKSPACE.  f64 inside, no atomics, fixed-order sums.  Upstream gradients are device memory.
 * ------------------------------------------------------------------------ */
/* PUILoss (contrastyou/losses/pica_loss.py:10-39) on rows x, y [N][K]; J[K][K] = sum_n x_ni y_nj is cy_joint_fwd with
 * H = W = 1.  cy_pui_stats (one block): stats[3][K] = column sums of x^2, of y^2 and of x.
 * cy_pui_loss (one block): a_i = max(|x_.i|_2, 1e-12), b_j likewise, pui_ij = J_ij / (a_i b_j), p = mean_n x,
 *   out[0] = mean_i [logsumexp_j pui_ij - pui_ii] + lamda (log K + sum_i p_i log p_i)   (no eps);
 * dJ (may be NULL) = dout/dJ at fixed norms; coef[3][K]: the rest of the gradient,
 *   dout/dx_ni = (adjoint of J)(dJ) + x_ni coef[0][i] + coef[2][i],  dout/dy_nj = (adjoint)(dJ) + y_nj coef[1][j]
 * (a clamped norm is a constant).  cy_rows_axpb: dx[r][c] += g[0] (x[r][c] a[c] + b[c]) over rows [R][K], b may be NULL. */
int cy_pui_stats(const float* x, const float* y, float* stats, long N, int K, void* stream);
int cy_pui_loss(const float* J, const float* stats, float* out, float* dJ, float* coef, long N, int K, float lamda,
                void* stream);
int cy_rows_axpb(const float* x, const float* a, const float* b, const float* g, float* dx, long R, int K, void* stream);
/* PUISegLoss (pica_loss.py:42-85).  J[TT][k][k] is cy_joint_fwd of (x_out, x_tf_out) at the loss's padding, x the NHWC
 * x_out as M = N H W rows of k.  q_d = (J_d - min J + 1e-16) / sum(J_d - min J + 1e-16), P = mean_d (q_d + q_d^T) / 2,
 *   out[0] = -(1/k^2) sum_i log(P_ii + 1e-16) + lamda (log M + sum_m p_m log p_m),  p_m = (1/k) sum_c x[m][c]
 * (the balance term runs over the permuted tensor, so p is the per-pixel mean over the classes; no eps).  dJ (may be
 * NULL) = dout/dJ with the minimum held constant.  Two launches: the streaming sum of p log p, then one block.
 * cy_puiseg_balance_bwd: dx[m][c] += g[0] lamda (log p_m + 1) / k.
 * ws_bytes >= 8 * (min(1024, ceil(M / 256)) + 2 TT) = cy_puiseg_ws_bytes (0 where the sizes are refused). */
size_t cy_puiseg_ws_bytes(long M, int TT, int k);
int cy_puiseg_loss(const float* J, const float* x, float* out, float* dJ, int TT, int k, long M, float lamda, void* ws,
                   size_t ws_bytes, void* stream);
int cy_puiseg_balance_bwd(const float* x, const float* g, float* dx, long M, int k, float lamda, void* stream);
/* JSD_div (contrastyou/losses/kl.py:142-174) of m maps (2..8; `maps` is a host array of m device pointers), C <= 64
 * classes, R positions.  Position r, class c is element r*C + c (rows / NHWC: S = 1) or (r / S)*C*S + c*S + r % S (NCHW
 * with S positions per image; R % S == 0).  v_r = H(mean_i x_i[r]) - mean_i H(x_i[r]), H(p) = -sum_c p log(p + eps).
 * reduction 0: out[R] = v; 1: out[0] = mean_r v_r; 2: out[0] = sum_r v_r (f64 block partials, fixed-order final sum;
 * ws_bytes >= 8 * min(1024, ceil(R / 256)) = cy_stream_sum_ws_bytes(R); reduction 0 needs no workspace).
 * Backward, one launch: dmaps[i] (host array of m device pointers in the maps' layout; an entry may be NULL) =
 * u_r (1/m) [(log(x + eps) + x / (x + eps)) - (log(mean + eps) + mean / (mean + eps))], u_r = g[r], g[0] / R or g[0]. */
size_t cy_stream_sum_ws_bytes(long R);
int cy_jsd_fwd(const float* const* maps, int m, float* out, long R, int C, long S, int reduction, float eps, void* ws,
               size_t ws_bytes, void* stream);
int cy_jsd_bwd(const float* const* maps, int m, const float* g, float* const* dmaps, long R, int C, long S,
               int reduction, float eps, void* stream);
/* EntropyPrior (kl.py:63-78) on rows x [R][C], prior [C] (NULL: uniform):
 *   out[0] = log C + (1/R) sum_r sum_c x_rc (log(prior_c + eps) - log(x_rc + eps))   = log C - KL_div()(prior, x);
 *   dx = g[0] / R (log(prior_c + eps) - log(x + eps) - x / (x + eps)); the prior is a constant.
 * ws_bytes >= cy_stream_sum_ws_bytes(R). */
int cy_entropy_prior_fwd(const float* x, const float* prior, float* out, long R, int C, float eps, void* ws,
                         size_t ws_bytes, void* stream);
int cy_entropy_prior_bwd(const float* x, const float* prior, const float* g, float* dx, long R, int C, float eps,
                         void* stream);

/* ------------------------------------------------------------------------
 * UNet2.Block = Conv2d(3x3, bias) -> GroupNorm(G, C) -> SiLU
 * (contrastyou/arch/unet2.py:208-224).  The conv runs on cy_conv3x3_* without
 * bias; these kernels fold the bias into the normalisation:
 * out = silu(gamma * ((y + bias) - mean_g) * rstd_g + beta), NHWC `dtype`.
 * mean_rstd: f32 [N][G][2], written by fwd, read by bwd.
 * ------------------------------------------------------------------------ */
size_t cy_gn_ws_bytes(int N, int C);
int cy_gn_silu_fwd(const void* y, int ldy, const float* bias, const float* gamma, const float* beta,
                   void* out, int ldo, float* mean_rstd, int N, int HW, int C, int G, float eps,
                   int dtype, void* ws, size_t ws_bytes, void* stream);
/* du = dloss/d(conv output); dgamma, dbeta, dbias f32 [C] (NULL to skip). */
int cy_gn_silu_bwd(const void* y, int ldy, const void* dz, int ldd, const float* bias,
                   const float* gamma, const float* beta, const float* mean_rstd, void* du, int ldu,
                   float* dgamma, float* dbeta, float* dbias, int accumulate, int N, int HW, int C,
                   int G, int dtype, void* ws, size_t ws_bytes, void* stream);
/* The same with the time-embedding modulation of ResnetBlock / Block (contrastyou/arch/unet2.py:216-220,240-246):
 * out = SiLU(GroupNorm(y + bias) * (mod_scale[n][c] + 1) + mod_shift[n][c]); mod_* are f32 [N][C].  Backward also gives
 * dmod_scale / dmod_shift [N][C] (NULL to skip). */
int cy_gn_silu_mod_fwd(const void* y, int ldy, const float* bias, const float* gamma, const float* beta,
                       const float* mod_scale, const float* mod_shift, void* out, int ldo, float* mean_rstd, int N,
                       int HW, int C, int G, float eps, int dtype, void* ws, size_t ws_bytes, void* stream);
int cy_gn_silu_mod_bwd(const void* y, int ldy, const void* dz, int ldd, const float* bias, const float* gamma,
                       const float* beta, const float* mod_scale, const float* mod_shift, const float* mean_rstd,
                       void* du, int ldu, float* dgamma, float* dbeta, float* dbias, float* dmod_scale,
                       float* dmod_shift, int accumulate, int N, int HW, int C, int G, int dtype, void* ws,
                       size_t ws_bytes, void* stream);
/* F.interpolate(x, size=(h,w), mode="bilinear", align_corners=False) on an NHWC
 * tensor (semi_seg/hooks/cc.py:132, ccblock.py:300). */
int cy_bilinear_fwd(const void* x, void* out, int N, int H, int W, int C, int h, int w, int dtype,
                    void* stream);

/* ------------------------------------------------------------------------
 * Cross-correlation regulariser (ABI v15; csrc/cy_cc.hip), f32.  Maps are [N][H][W] f32, contiguous.
 * All sums run in a fixed order: two calls on the same inputs give the same bits.
 * ------------------------------------------------------------------------ */
/* Edge strength of an NHWC f32 image [N,H,W,C], C <= 4 (semi_seg/hooks/ccblock.py:287-293,302; cc.py:119-125,134):
 *   d = mean_c sqrt((x - roll(x,1,H))^2 + (x - roll(x,1,W))^2);  out = ((d - min) / (max - min + 1e-6)) ^ power
 * with the extrema of each image.  Two launches (raw map + extrema partials; normalise).  ws: _ws_bytes(N). */
size_t cy_cc_edge_map_ws_bytes(int N);
int cy_cc_edge_map(const float* img, float* out, int N, int H, int W, int C, float power, void* ws, size_t ws_bytes,
                   void* stream);
/* Entropy map of probability rows p [N*HW][K], K <= 128 (Entropy(reduction="none"), contrastyou/losses/kl.py:31-55;
 * ccblock.py:303, cc.py:136): out = (e - min) / (max - min + 1e-6), e = -sum_c p log(p + 1e-16), with the extrema of
 * each image (slicewise != 0) or of the whole batch; mm [N][2] receives the {min, max} used per image.  Two launches.
 * Backward: dp = dloss/dp from dmap = dloss/dout; the extrema carry no gradient (min().detach()).  One launch. */
size_t cy_entropy_map_ws_bytes(int N);
int cy_entropy_map_fwd(const float* p, float* out, float* mm, int N, long HW, int K, int slicewise, void* ws,
                       size_t ws_bytes, void* stream);
int cy_entropy_map_bwd(const float* p, const float* mm, const float* dmap, float* dp, int N, long HW, int K,
                       void* stream);
/* CCLoss(win=(k,k), eps)(y_true = I, y_pred = J) (contrastyou/losses/cross_correlation.py:22-74; ccblock.py:305,
 * cc.py:138): zero-padded k x k box sums of I, J, I^2, J^2, IJ, the three clamped terms, loss = -mean(cross^2 /
 * (I_var * J_var)).  k odd, 3..15 (CY_ERR_SHAPE otherwise).  Forward: two launches (per-tile sums; ordered final sum).
 * Backward: dI and / or dJ (either may be NULL) = gscale[0] * dloss/d{I, J}; one launch, recomputes the sums. */
size_t cy_ccloss_ws_bytes(int N, int H, int W);
int cy_ccloss_fwd(const float* I, const float* J, float* loss, int N, int H, int W, int win, float eps, void* ws,
                  size_t ws_bytes, void* stream);
int cy_ccloss_bwd(const float* I, const float* J, const float* gscale, float* dI, float* dJ, int N, int H, int W,
                  int win, float eps, void* stream);

/* ------------------------------------------------------------------------
 * The glue of the reference's second backbone, `UNet2` (contrastyou/arch/unet2.py): everything that is not a
 * 3x3 conv + GroupNorm + SiLU block.  f32, NHWC maps viewed as [pixels][channels] matrices.
 *   7x7 stem (:45), Downsample = Conv2d(4, 2, 1) (:180-181), 1x1 projections      -> cy_im2col + cy_gemm_strided
 *   Upsample = ConvTranspose2d(4, 2, 1) (:176-177) and every data gradient        -> cy_gemm_strided + cy_col2im
 *   LayerNorm over channels (:183-194)                                            -> cy_chan_layernorm_*
 *   LinearAttention (:245-271): q.softmax(-2) * scale, k.softmax(-1), two einsums  -> cy_head_softmax_*,
 *                                                                                    cy_col_softmax_*, cy_gemm_strided
 *   Attention (:274-304): softmax(q k^T) v over the positions of the bottleneck   -> cy_gemm_strided, cy_row_softmax_*
 * ------------------------------------------------------------------------ */
typedef struct {
  long rs, cs; /* element (i, j) of a matrix at i*rs + j*cs (in elements) */
  long s1, s2; /* batch (b1, b2) starts at b1*s1 + b2*s2 */
} cy_mat_layout;
/* C[b] = alpha * A[b] (M x K) * B[b] (K x N) (+ bias[n]) (+ C[b] when accumulate) for nb1 x nb2 batches, every
 * operand addressed through its layout (so transposes, channel slices of a wider map and per-head blocks need no
 * copies), on the f32 MFMA.  ksplit > 1 splits K into that many ranges whose partial products go through `ws`
 * (cy_gemm_strided_ws_bytes) and are summed in a fixed order: run-to-run identical results. */
size_t cy_gemm_strided_ws_bytes(int M, int N, int nbatch, int ksplit);
int cy_gemm_strided(const float* A, const cy_mat_layout* la, const float* B, const cy_mat_layout* lb, float* C,
                    const cy_mat_layout* lc, const float* bias, int M, int N, int K, int nb1, int nb2, float alpha,
                    int accumulate, int ksplit, float* ws, size_t ws_bytes, void* stream);
/* cols[(n, ho, wo)][(kh, kw, c)] = x[n, ho*stride - pad + kh, wo*stride - pad + kw, c] (zero outside);
 * Ho = (H + 2 pad - KH) / stride + 1.  x [N,H,W,C], cols [N*Ho*Wo][KH*KW*C]. */
int cy_im2col(const float* x, float* cols, int N, int H, int W, int C, int KH, int KW, int stride, int pad,
              void* stream);
/* the adjoint of cy_im2col as a gather: out[n,h,w,c] = bias[c] (or 0) + the sum of the cols entries that were read
 * from (n,h,w,c).  H, W are those of `out`. */
int cy_col2im(const float* cols, const float* bias, float* out, int N, int H, int W, int C, int KH, int KW, int stride,
              int pad, void* stream);
/* out[n] (+)= sum_m x[m][n], two ordered stages (bias gradients) */
size_t cy_colsum_ws_bytes(long M, int N);
int cy_colsum(const float* x, float* out, long M, int N, int accumulate, float* ws, size_t ws_bytes, void* stream);
/* y[p][c] = (x[p][c] - mean_p) / sqrt(var_p + eps) * g[c] + b[c] over the C channels of each of M pixels */
int cy_chan_layernorm_fwd(const float* x, const float* g, const float* b, float* y, long M, int C, float eps,
                          void* stream);
size_t cy_chan_layernorm_bwd_ws_bytes(long M, int C);
/* dx, and dg / db (both or neither) */
int cy_chan_layernorm_bwd(const float* x, const float* g, const float* dy, float* dx, float* dg, float* db, long M,
                          int C, float eps, float* ws, size_t ws_bytes, void* stream);
/* y[p][h][d] = scale * softmax_d(x[p][off + h*dh + d]) for rows of ld floats (q of the linear attention) */
int cy_head_softmax_fwd(const float* x, int ld, int off, float* y, long M, int heads, int dh, float scale,
                        void* stream);
/* its backward, written into columns off.. of rows of ld_dx floats */
int cy_head_softmax_bwd(const float* y, const float* dy, float* dx, int ld_dx, int off, long M, int heads, int dh,
                        float scale, void* stream);
/* y[b][p][c] = softmax over the n positions p of image b of x[(b*n + p)*ld + off + c] (k of the linear attention) */
size_t cy_col_softmax_ws_bytes(int B, int n, int Ch);
int cy_col_softmax_fwd(const float* x, int ld, int off, float* y, int B, int n, int Ch, float* ws, size_t ws_bytes,
                       void* stream);
/* dx[(b*n + p)*ld_dx + off + c] = y * (dy - t[b][c]) with t[b][c] = sum_p y * dy supplied by the caller */
int cy_col_softmax_bwd(const float* y, const float* dy, const float* t, float* dx, int ld_dx, int off, int B, int n,
                       int Ch, void* stream);
/* softmax of every row of x [rows][n], in place; backward: dp <- p * (dp - sum_j p * dp) */
int cy_row_softmax_fwd(float* x, long rows, int n, void* stream);
int cy_row_softmax_bwd(const float* p, float* dp, long rows, int n, void* stream);
/* UNet2's time embedding (contrastyou/arch/unet2.py:51-58,161-173,230-231): SinusoidalPosEmb(dim) of time [B] ->
 * out [B][dim] (sin half, cos half); elementwise SiLU (kind 0) / exact GELU (kind 1) of the embedding MLPs, f32 */
int cy_sinusoidal_emb(const float* time, float* out, int B, int dim, void* stream);
int cy_act_fwd(const float* x, float* y, long n, int kind, void* stream);
int cy_act_bwd(const float* x, const float* dy, float* dx, long n, int kind, void* stream);

/* ------------------------------------------------------------------------
 * The adversarial baseline's discriminator, everything around its convolutions (csrc/cy_disc.hip; 12 entries added to
 * ABI v15 -- no existing signature changed, so cy_abi_version() stays 15).  f32, NHWC rows.  Every entry checks its
 * arguments before any launch: a NULL pointer, a count < 1, K outside 2..16, Ci outside 0..4, C outside 1..1024, a
 * label other than 0 or 1, or a row base that is not 16-byte aligned where rows are read 16 bytes at a time (K == 4,
 * C % 4 == 0) -> CY_ERR_ARG; a short workspace -> CY_ERR_WORKSPACE.  No floating-point atomics: reductions write f64
 * partials that a later launch sums in a fixed order, so two runs give the same bits.
 * ------------------------------------------------------------------------ */
/* torch.cat([image, logits.softmax(1)], 1) (semi_seg/epochers/comparable.py:150-153,172-182): out[p] =
 * (image[p][0..Ci), softmax(logits[p][0..K))), rows of Ci + K floats.  Ci == 0 with image == NULL is the
 * dis_consider_image=False form.  One launch. */
int cy_softmax_cat_fwd(const float* image, const float* logits, float* out, long npix, int Ci, int K, void* stream);
/* dlogits = p * (g - sum_k p_k g_k), g = the last K columns of dout's rows of Ci + K floats; the softmax is
 * recomputed, the image columns carry no gradient.  One launch. */
int cy_softmax_cat_bwd(const float* logits, const float* dout, float* dlogits, long npix, int Ci, int K,
                       void* stream);
/* nn.BatchNorm2d(C) in training mode followed by nn.LeakyReLU(slope) (contrastyou/arch/discriminator.py:26-35) over
 * rows x[M][C], M = N*H*W.  ws_bytes = 16 * C * chunks, chunks = min(256, ceil(M / (8 * (256 / lpr)))), lpr = the
 * smallest power of two >= C / V capped at 64, V = 4 when C % 4 == 0, else 1 (0 for M < 1 or a C out of range).
 * cy_bn_rows_stats (two launches, M >= 2): mean[C] and the biased variance var[C]; the partial sums are f64 sums of
 * x - x[0][c] and its square (exact differences; no E[x^2] - E[x]^2 cancellation).  With running_mean / running_var
 * (both or neither) it also does running = (1 - momentum) * running + momentum * {mean, var * M / (M - 1)}, and with
 * num_batches_tracked (int64) adds 1 to it. */
size_t cy_bn_rows_ws_bytes(long M, int C);
int cy_bn_rows_stats(const float* x, float* mean, float* var, long M, int C, float* running_mean, float* running_var,
                     long long* num_batches_tracked, float momentum, void* ws, size_t ws_bytes, void* stream);
/* y = lrelu(gamma * (x - mean) / sqrt(var + eps) + beta, slope); handed the running statistics it is the eval-mode
 * layer.  One launch. */
int cy_bn_lrelu_fwd(const float* x, const float* mean, const float* var, const float* gamma, const float* beta,
                    float* y, long M, int C, float eps, float slope, void* stream);
/* dz = dy * lrelu'(gamma * xhat + beta) with the pre-activation recomputed from x; dgamma = sum dz * xhat,
 * dbeta = sum dz.  Two launches. */
int cy_bn_lrelu_bwd_reduce(const float* x, const float* dy, const float* mean, const float* var, const float* gamma,
                           const float* beta, float* dgamma, float* dbeta, long M, int C, float eps, float slope,
                           void* ws, size_t ws_bytes, void* stream);
/* batch_stats != 0: dx = gamma * invstd * (dz - dbeta / M - xhat * dgamma / M) (M >= 2); batch_stats == 0 (running
 * statistics): dx = gamma * invstd * dz, dgamma / dbeta may be NULL.  One launch. */
int cy_bn_lrelu_bwd_apply(const float* x, const float* dy, const float* mean, const float* var, const float* gamma,
                          const float* beta, const float* dgamma, const float* dbeta, float* dx, long M, int C,
                          float eps, float slope, int batch_stats, void* stream);
/* nn.LeakyReLU(slope) without a BatchNorm in front (discriminator.py:23): y = x > 0 ? x : x * slope; the backward
 * works from the input: dx = x > 0 ? dy : dy * slope.  One launch, two when n % 4 != 0. */
int cy_leaky_relu_fwd(const float* x, float* y, long n, float slope, void* stream);
int cy_leaky_relu_bwd(const float* x, const float* dy, float* dx, long n, float slope, void* stream);
/* nn.BCELoss()(sigmoid(scores), full_like(scores, label)) (comparable.py:125,155-156,176-184) without forming
 * 1 - sigmoid(s): mean over n of min(softplus(-s), 100) for label 1, of min(softplus(s), 100) for label 0 (torch clamps
 * the logarithm at -100).  ws_bytes = 8 * min(1024, ceil(n / 256)).  Forward: two launches.  Backward (one launch):
 * dscores = gscale[0] * (sigmoid(s) - label) / n, 0 where the forward was clamped. */
size_t cy_sigmoid_bce_ws_bytes(long n);
int cy_sigmoid_bce_fwd(const float* scores, float label, float* loss, long n, void* ws, size_t ws_bytes,
                       void* stream);
int cy_sigmoid_bce_bwd(const float* scores, float label, const float* gscale, float* dscores, long n, void* stream);

/* ------------------------------------------------------------------------
 * The discriminator's convolutions (contrastyou/arch/discriminator.py:22-40 of the reference: nn.Conv2d(Cin, Cout, 4,
 * 2, 1, bias=False) four times and nn.Conv2d(Cin, 1, 4, 1, 0, bias=False)) as implicit GEMMs on the f32 MFMA
 * (csrc/cy_conv4x4.hip; 5 entries added to ABI v16 -- no existing signature changed, so cy_abi_version() stays 16).
 * f32, NHWC: x [N][H][W][Cin], y / dy [N][Ho][Wo][Cout], Ho = (H + 2 pad - 4) / stride + 1.  No patch matrix is
 * written and there is no im2col / col2im launch.  Every entry checks its arguments before any launch: a NULL
 * pointer, a size < 1, Cin or Cout above 2^20, or N * H * W above 2^31 - 1 (pixel indices are 32-bit, element offsets
 * 64-bit) -> CY_ERR_ARG; (ksize, stride, pad) other than (4, 2, 1) and (4, 1, 0), or a padded input smaller than the
 * kernel -> CY_ERR_SHAPE; a short workspace -> CY_ERR_WORKSPACE.  Rows are read 16 bytes at a time where the
 * contiguous channel count is a multiple of 4 and the base is 16-byte aligned, 4 bytes at a time otherwise (chosen by
 * that rule per call; a misaligned base is never read 16 bytes at a time).  Cout >= 32 runs the MFMA kernels, Cout <
 * 32 VALU forms (the data gradient also for Cin < 32).  No floating-point atomics: two runs give the same bits.
 * ------------------------------------------------------------------------ */
/* w [Cout][Cin][4][4] (torch's layout) -> packed [Cout][kh][kw][Cin] (transposed == 0: what cy_conv4x4_fwd reads) or
 * [Cin][kh][kw][Cout] (transposed != 0: what cy_conv4x4_dgrad reads).  One launch. */
int cy_conv4x4_pack_weights(const float* w, float* packed, int Cin, int Cout, int transposed, void* stream);
/* y = conv(x, w); wp packed with transposed == 0.  One launch. */
int cy_conv4x4_fwd(const float* x, const float* wp, float* y, int N, int H, int W, int Cin, int Cout, int ksize,
                   int stride, int pad, void* stream);
/* dx [N][H][W][Cin] from dy, every element written (zero where no output reaches it); wpt packed with transposed
 * != 0.  Stride 2: four gather GEMMs over the 2 x 2 taps of each (h, w) parity class, in one launch. */
int cy_conv4x4_dgrad(const float* dy, const float* wpt, float* dx, int N, int H, int W, int Cin, int Cout, int ksize,
                     int stride, int pad, void* stream);
/* dw [Cout][Cin][4][4] from x and dy.  The M = N * Ho * Wo output positions are split into `splits` ranges whose f32
 * partial sums go through ws and are added in ascending order by a second launch.
 *   ws_bytes = 4 * splits * Cout * 16 * Cin,  splits = max(1, min(ceil(256 / tiles), ceil(M / rows_min), 256)),
 *   Cout >= 32: tiles = ceil(Cout / 128) * ceil(16 * Cin / 128), rows_min = 512;
 *   Cout <  32: tiles = ceil(Cout * 16 * Cin / 256),             rows_min = 64
 * (0 where the launch would refuse its arguments).  Two launches. */
size_t cy_conv4x4_wgrad_ws_bytes(int N, int H, int W, int Cin, int Cout, int ksize, int stride, int pad);
int cy_conv4x4_wgrad(const float* x, const float* dy, float* dw, int N, int H, int W, int Cin, int Cout, int ksize,
                     int stride, int pad, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Surface-distance statistics at inference (csrc/cy_surface.hip; 2 entries added to ABI v17 -- no existing signature
 * changed, so cy_abi_version() stays 17).  Replaces SurfaceMeter._evalue (contrastyou/meters/surface_meter.py:93-112)
 * and the three functions of contrastyou/meters/surface_distance.py:11-31, which go through medpy's
 * __surface_distances (binary erosion + exact Euclidean distance transform on the host).
 * pred and target are class-index volumes, int64 [D][H][W], read as they are; classes is a HOST array of R reported
 * class indices.  Per reported class r and direction d (0: pred -> target, 1: target -> pred), with a = (volume of d ==
 * class) and b = (the other volume == class):
 *   border(a)(v) = a(v) && !(all face neighbours of v in a); a neighbour outside the volume is background; ndim == 3
 *                  tests the depth neighbours too, ndim == 2 (D must be 1) does not;
 *   d2(v)        = min over border(b) voxels u of |v - u|^2, exact in int32 (separable min-plus passes along W, H, D,
 *                  one line staged in LDS per output); 2^30 everywhere when border(b) is empty;
 *   count[d][r]  = |border(a)|, sum[d][r] = sum over border(a) of sqrt((double)d2), maxd2[d][r] = max over border(a).
 * Outputs are device arrays [2][R].  d2_maps (int32 [2][R][V]) and border_maps (uint8 [2][R][V]), V = D*H*W, are
 * optional (NULL: not written): d2_maps[d][r] is the distance map direction d reads, border_maps[d][r] is border(a).
 * No atomics: f64 partials per block (at most 1024 blocks of 256) and one fixed-order final sum, so two runs give
 * the same bits.  Six launches per class, classes one after the other through the same workspace:
 *   ws_bytes = roundup(2 V, 16) + 8 V + 2 * 1024 * 24   (two border masks, two d2 maps, the partials).
 * Checked before any launch: a NULL pointer (the two map pointers excepted), a size < 1 or V > 2^31 - 1 -> CY_ERR_ARG;
 * D, H or W > CY_SURFACE_MAX_LINE, R outside 1 .. CY_SURFACE_MAX_CLASSES, ndim not 2 or 3, ndim == 2 with D != 1 ->
 * CY_ERR_SHAPE; a short workspace -> CY_ERR_WORKSPACE.  cy_surface_ws_bytes is 0 where the sizes are refused.
 * ------------------------------------------------------------------------ */
#define CY_SURFACE_MAX_LINE 1024   /* the LDS line buffer: 8 lines * 1024 * 4 bytes */
#define CY_SURFACE_MAX_CLASSES 64
size_t cy_surface_ws_bytes(int D, int H, int W);
int cy_surface_stats(const int64_t* pred, const int64_t* target, const int32_t* classes, int R, int D, int H, int W,
                     int ndim, int64_t* count, double* sum, int32_t* maxd2, int32_t* d2_maps, uint8_t* border_maps,
                     void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Per-row projector: the dense projection head without pooling, and point evaluation of it (csrc/cy_pixel_mlp.hip;
 * 4 entries added to ABI v18).  Replaces, for
 * pool_name in ("identical", "none", None), the Conv2d(1x1) -> LeakyReLU -> Conv2d(1x1) -> Identical -> F.normalize of
 * DenseProjectionHead.forward (contrastyou/projectors/heads.py:99-123, projectors/nn.py:16-23) on every pixel, or on
 * the pixels the dense InfoNCE hook samples (semi_seg/hooks/infonce.py:31-46).
 *   y[m] = W2 lrelu(W1 x[r(m)] + b1, slope) + b2   (hid > 0)        x: rows of `dtype`, pixel pitch ldx >= C elements
 *   y[m] = W1 x[r(m)] + b1                          (hid == 0)       w1 f32 [hid or out][C], w2 f32 [out][hid]
 *   r(m) = idx ? idx[m] : m                                          idx: int32 [M], distinct rows of x; NULL = all rows
 *   normalize: y[m] *= inv[m], inv[m] = 1 / max(||y[m]||_2, 1e-12)   y f32 [M][out], inv f32 [M] (may be NULL otherwise)
 * Fused range 1 <= C <= 256, 0 <= hid <= 256, 1 <= out <= 256; sizes are zero-padded to multiples of 32 inside the
 * kernels.  16-bit rows: bf16 / f16 MFMA with f32 accumulation, W1 and W2 rounded to the storage type, bias and
 * LeakyReLU in f32, the hidden tile rounded to the storage type once for the second product; it lives in LDS and is
 * never written to memory.  f32 rows: f32 MFMA, nothing is rounded.  One launch.
 * Backward (recomputes the hidden tile; dY is formed from dy, y and inv when `normalize`; dY and dH are rounded to the
 * storage type for their products): dx (dtype, pitch ldx; may be NULL) is ACCUMULATED into, at the rows r(m) only
 * (zero it first), as cy_dense_proj_bwd does; dw1, db1, dw2, db2 (f32, each may be NULL) are written, or added to
 * with `accumulate`.  The parameter gradients go through one partial slab per workgroup in ws and a second launch that
 * adds the slabs in slab order: no atomics, two runs give the same bits.
 * cy_pixel_mlp_plan (host side, no GPU needed) is the launch rule both launches and the workspace query follow.
 *   ws_bytes = 4 * slabs * (J Cp + J + (hid ? Op Hp + Op : 0)) with Cp, Hp, Op the sizes rounded up
 *   to 32 and J = hid ? Hp : Op: it does not grow with M past the cap (0 where the sizes are refused).
 * Checked before any launch: a NULL required pointer -> CY_ERR_ARG; M < 1, a size outside the fused range or
 * ldx < C -> CY_ERR_SHAPE; a short workspace (when a parameter gradient is asked for) -> CY_ERR_WORKSPACE.
 * ------------------------------------------------------------------------ */
#define CY_PIXEL_MLP_MFMA16 1 /* bf16 / f16 rows: 64 rows per tile */
#define CY_PIXEL_MLP_MFMA32 2 /* f32 rows: 32 rows per tile */
typedef struct cy_pixel_mlp_plan_t {
  int32_t form;          /* kernel form (CY_PIXEL_MLP_*) */
  int32_t rows_per_tile; /* rows per tile */
  int32_t fwd_grid;      /* forward workgroups (<= 1024) */
  int32_t fwd_trips;     /* forward loop trips */
  int32_t bwd_grid;      /* backward workgroups (<= 256) */
  int32_t bwd_trips;     /* backward loop trips */
  int32_t slabs;         /* partial slabs */
  int32_t lds_bytes;     /* dynamic LDS bytes (the larger of the two kernels') */
} cy_pixel_mlp_plan_t;
int cy_pixel_mlp_plan(long M, int C, int hid, int out, int dtype, cy_pixel_mlp_plan_t* plan);
int cy_pixel_mlp_fwd(const void* x, const int32_t* idx, const float* w1, const float* b1, const float* w2,
                     const float* b2, float* y, float* inv, long M, int C, int ldx, int hid, int out, float slope,
                     int normalize, int dtype, void* stream);
size_t cy_pixel_mlp_bwd_ws_bytes(long M, int C, int hid, int out, int dtype);
int cy_pixel_mlp_bwd(const void* x, const int32_t* idx, const float* w1, const float* b1, const float* w2,
                     const float* y, const float* inv, const float* dy, void* dx, float* dw1, float* db1, float* dw2,
                     float* db2, int accumulate, long M, int C, int ldx, int hid, int out, float slope, int normalize,
                     int dtype, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * IMSAT: marginal and conditional entropy of probability rows (csrc/cy_imsat.hip; entries added to ABI v18).  For p [R][K] f32, every row a probability simplex, and
 * eps the module-level entropy_criterion's 1e-8 (semi_seg/hooks/midl.py:13; not IMSATLoss.eps, which the reference
 * never reads):
 *   cond = (1/R) sum_r -sum_k p_rk log(p_rk + eps)      m_k = (1/R) sum_r p_rk      marg = -sum_k m_k log(m_k + eps)
 *   dcond/dp_rk = -(log(p_rk + eps) + p_rk/(p_rk + eps)) / R        dmarg/dp_rk = c_k = -(log(m_k + eps) + m_k/(m_k + eps)) / R
 * p_rk = 0 adds exactly 0 to cond and has the gradient entry -log(eps) / R.  Rows may come in any order (a 4-D
 * [b,K,H,W] map is its b*H*W rows).  The forward is two launches: every block writes one f64 partial of cond and K f64
 * column sums into ws, then one block adds the partials of all blocks in an order the grid alone decides (computing
 * m_k, c_k and marg in f64) and writes
 *   out [2] = {marg, cond},  coef [K] = c_k,  mean [K] = m_k.
 * The backward is one launch: dp_rk = g[1] * dcond/dp_rk + g[0] * c_k, with g the two upstream gradients in device
 * memory.  No atomics: two runs give the same bits.  Every entry checks its arguments before any launch: a NULL
 * pointer or R < 1 -> CY_ERR_ARG; K outside 2..64 (2..16 from logits) -> CY_ERR_SHAPE; a short workspace ->
 * CY_ERR_WORKSPACE.  The *_ws_bytes queries return 0 where the sizes are refused.
 * ------------------------------------------------------------------------ */
#define CY_IMSAT_ROWS 0   /* cy_imsat_* */
#define CY_IMSAT_PAIR 1   /* cy_imsat_pair_* */
#define CY_IMSAT_LOGITS 2 /* cy_softmax_imsat_* */
/* The launch rule of the three groups (host-side only, launches nothing; the launches and the workspace queries take
 * every decision from it), in the style of cy_pixel_mlp_plan.  `align`: the bytes every tensor base pointer of the call
 * is aligned to (the launches work it out from their pointers; 16 and more count as 16).
 * Rows and pair: the buffer is swept flat, thread t of a block reading `vec` floats at vec * t of each chunk, with
 * `threads` = the largest T <= 256 with (vec * T) % K == 0 working threads, so that a thread keeps its columns.
 * vec = 4 where align is a multiple of 16, else 1 -- the only two kernel forms.  Logits: one thread per pixel; kt = K
 * for the compiled K = 2, 4, 8 where the rows are aligned to their 8 / 16 bytes, else 0 (run-time K, one float at a
 * time).  K == 4 rows are read 16 bytes at a time in both forms: a misaligned base is CY_ERR_ARG.
 * Returns what the launches answer: CY_ERR_ARG for a NULL `out`, an unknown form, R < 1, align < 1 or misaligned
 * K == 4 logits; CY_ERR_SHAPE for K out of range; otherwise CY_OK. */
typedef struct cy_imsat_plan_t {
  int32_t vec;       /* floats per memory access (rows / pair 4 or 1; logits 2 (kt 2), 4 (kt 4, 8) or 1) */
  int32_t kt;        /* logits: the compiled K (2, 4, 8) or 0; rows / pair: 0 */
  int32_t threads;   /* working threads of the 256 of a block */
  int32_t tile;      /* rows / pair: floats per block and trip = threads * vec * 4; logits: pixels = 256 */
  int32_t fwd_grid;  /* min(1024, tiles) blocks = rows of partials */
  int32_t fwd_trips; /* of the busiest block */
  int32_t bwd_grid;  /* min(2048, tiles) */
  int32_t bwd_trips;
  int32_t slots;     /* f64 partials per block = 1 + K, pair 3 + 2 K */
} cy_imsat_plan_t;
int cy_imsat_plan(int form, long R, int K, int align, cy_imsat_plan_t* out);
/* imsat_with_entropy(p) / imsat_loss(p, lamda) = cond - lamda * marg / IMSATDynamicWeight's -w * marg + cond
 * (contrastyou/losses/discreteMI.py:20-87,275-297; the combination is left to the caller, on the two device scalars).
 * ws_bytes >= 8 * (1 + K) * min(1024, ceil(R K / (4 K floor(256 / K)))) = cy_imsat_ws_bytes(R, K): the grid of
 * the 4-byte form, which is never the smaller one. */
size_t cy_imsat_ws_bytes(long R, int K);
int cy_imsat_fwd(const float* p, float* out, float* coef, float* mean, long R, int K, float eps, void* ws,
                 size_t ws_bytes, void* stream);
int cy_imsat_bwd(const float* p, const float* coef, const float* g, float* dp, long R, int K, float eps, void* stream);
/* Two views x1, x2 [R][K] and their consistency, what _DiscreteIMSATEpochHook evaluates per sub-head
 * (semi_seg/hooks/discretemi.py:148-167: IMSATLoss(x1, x2) and nn.MSELoss()(x1, x2)), each input read once:
 *   out [5] = {marg1, cond1, marg2, cond2, mse},  mse = sum (x1 - x2)^2 / (R K);  coef, mean [2][K].
 * Backward, one launch, both gradients from the five upstream scalars g [5] (same order as out).  The inputs are
 * usually the halves of one [2R][K] tensor, so a base is only known to be 4-byte aligned: see cy_imsat_plan.
 * ws_bytes >= 8 * (3 + 2 K) * (the blocks of cy_imsat_ws_bytes). */
size_t cy_imsat_pair_ws_bytes(long R, int K);
int cy_imsat_pair_fwd(const float* x1, const float* x2, float* out, float* coef, float* mean, long R, int K, float eps,
                      void* ws, size_t ws_bytes, void* stream);
int cy_imsat_pair_bwd(const float* x1, const float* x2, const float* coef, const float* g, float* dx1, float* dx2,
                      long R, int K, float eps, void* stream);
/* The same of softmax(logits, 1), logits [npix][K] f32 (NHWC), 2 <= K <= 16 (_IMSATEpochHook,
 * semi_seg/hooks/midl.py:83-90); outputs as cy_imsat_fwd.  The backward recomputes the softmax:
 *   a_k = g[1] * dcond/dp_k + g[0] * c_k,  dz_k = p_k (a_k - sum_j p_j a_j).
 * ws_bytes >= 8 * (1 + K) * min(1024, ceil(npix / 256)). */
size_t cy_softmax_imsat_ws_bytes(long npix, int K);
int cy_softmax_imsat_fwd(const float* logits, float* out, float* coef, float* mean, long npix, int K, float eps,
                         void* ws, size_t ws_bytes, void* stream);
int cy_softmax_imsat_bwd(const float* logits, const float* coef, const float* g, float* dlogits, long npix, int K,
                         float eps, void* stream);

/* ------------------------------------------------------------------------
 * MixUp and interpolation-consistency training (csrc/cy_mixup.hip; entries added to ABI v18).
 * Image n of a batch of N is mixed with image index[n]; `index` is int32 [N]
 * in device memory and a gather: any values in [0, N), not only permutations (the caller checks the range; the kernels
 * trust it).  w_self and w_other are lam and 1 - lam, formed in f64 on the host and rounded to f32 each, which is what
 * `lam * x + (1 - lam) * x[index]` (semi_seg/hooks/utils.py:284-297) does; no kernel forms 1 - w.  Logits are
 * [npix][K] f32 rows (NHWC), npix = N * HW, image n owning the pixels [n HW, (n + 1) HW); 2 <= K <= 16.  Every entry
 * checks its arguments before any launch: a NULL pointer, N < 1, a size < 1 or a base that is not 4-byte aligned ->
 * CY_ERR_ARG; K out of range -> CY_ERR_SHAPE; a short workspace -> CY_ERR_WORKSPACE.  The losses are one thread per
 * pixel, grid-stride; the forward writes one f64 partial per block and one block sums them in block order, the
 * backward is one launch.  No atomics: two runs give the same bits.  Upstream gradients are device memory.
 * ------------------------------------------------------------------------ */
#define CY_MIX_IMAGES 0 /* cy_mix_images */
#define CY_MIX_KL 1     /* cy_softmax_mixkl_* */
#define CY_MIX_MSE 2    /* cy_softmax_mixmse_* */
/* The launch rule of the three groups (host-side only, launches nothing; the launches take every decision from it), in
 * the style of cy_imsat_plan.  `per_image`: E of cy_mix_images, HW of the losses.  `align`: the bytes every tensor base
 * pointer of the call is aligned to (the launches work it out from their pointers; 16 and more count as 16).
 * Returns what the launches answer: CY_ERR_ARG for a NULL `out`, an unknown form, N < 1, per_image < 1 or such an
 * align; CY_ERR_SHAPE for K out of range (losses; images ignore K); otherwise CY_OK. */
typedef struct cy_mix_plan_t {
  int32_t vec;       /* floats per memory access.  Images: 4 where per_image % 4 == 0 and align is a multiple of 16,
                        else 1.  Losses: 2 (kt 2), 4 (kt 4, 8) or 1 */
  int32_t kt;        /* losses: the compiled K (2, 4, 8) where the rows are aligned to their 8 / 16 bytes, else 0
                        (run-time K, one float at a time; K == 4 rows are read 16 bytes at a time in both forms: a
                        misaligned base is CY_ERR_ARG).  Images: 0 */
  int32_t fwd_grid;  /* losses min(1024, ceil(npix / 256)) blocks = the f64 partials; images rows * columns, with
                        columns = min(ceil(per_image / vec / 256), 2048 / rows) blocks striding over one image */
  int32_t fwd_trips; /* loop trips of the busiest block */
  int32_t bwd_grid;  /* 2 * fwd_grid (images: 0) */
  int32_t bwd_trips; /* (images: 0) */
  int32_t rows;      /* images: min(N, 1024) grid rows striding over the images; losses: 0 */
} cy_mix_plan_t;
int cy_mix_plan(int form, int N, long per_image, int K, int align, cy_mix_plan_t* out);
/* out[n][e] = w_self * x[n][e] + w_other * x[index[n]][e], E contiguous f32 elements per image (any memory format, the
 * same for x and out; out must not be x).  Two correctly rounded products and one correctly rounded sum, never an
 * FMA: the bits of torch's CPU f32 evaluation of the reference expression. */
int cy_mix_images(const float* x, const int32_t* index, float w_self, float w_other, float* out, int N, long E,
                  void* stream);
/* MixUp (semi_seg/hooks/mixup.py:49-58): KL_div(eps)(softmax(logits), t), t = w_self onehot(target) + w_other
 * onehot(target)[index], without the one-hot tensors: per pixel a = target[pix], b = target[index[n] HW + hw],
 *   l = -sum_{k in {a, b}} t_k log((p_k + eps) / (t_k + eps)),  t_a = w_self, t_b = w_other (a == b: the one term with
 *   t_a = w_self + w_other, summed in f32);  loss[0] = sum l / npix.
 * A weight of exactly 0 adds exactly 0; a label outside [0, K) selects no class (p = 0) and nothing is read out of
 * range.  Backward: dz_j = (gscale[0] / npix) sum_{k in {a, b}} t_k p_k / (p_k + eps) (p_j - [k == j]).
 * ws_bytes >= 8 * min(1024, ceil(npix / 256)). */
size_t cy_softmax_mixkl_ws_bytes(int N, long HW);
int cy_softmax_mixkl_fwd(const float* logits, const int64_t* target, const int32_t* index, float w_self, float w_other,
                         float* loss, int N, long HW, int K, float eps, void* ws, size_t ws_bytes, void* stream);
int cy_softmax_mixkl_bwd(const float* logits, const int64_t* target, const int32_t* index, float w_self, float w_other,
                         const float* gscale, float* dlogits, int N, long HW, int K, float eps, void* stream);
/* ICT (semi_seg/hooks/mt.py:301-319): MSE of softmax(student) against m = w_self softmax(teacher[pix]) + w_other
 * softmax(teacher[index[n] HW + hw]), loss[0] = sum (softmax(s)_k - m_k)^2 / (npix K).  Backward, student only (the
 * teacher carries no gradient): d = 2 gscale[0] (p - m) / (npix K), ds = p (d - <d, p>).  Workspace as above. */
size_t cy_softmax_mixmse_ws_bytes(int N, long HW);
int cy_softmax_mixmse_fwd(const float* student, const float* teacher, const int32_t* index, float w_self,
                          float w_other, float* loss, int N, long HW, int K, void* ws, size_t ws_bytes, void* stream);
int cy_softmax_mixmse_bwd(const float* student, const float* teacher, const int32_t* index, float w_self,
                          float w_other, const float* gscale, float* dstudent, int N, long HW, int K, void* stream);

/* ------------------------------------------------------------------------
 * DAE prior and orthogonal prototypes (csrc/cy_prior.hip; entries added to ABI v18).
 * Every entry checks its arguments before any launch: a NULL pointer, a count < 1 or a
 * base that is not 4-byte aligned -> CY_ERR_ARG; K, Cimg, the activation or K * C out of range -> CY_ERR_SHAPE; a short
 * workspace -> CY_ERR_WORKSPACE.  No atomics: two runs give the same bits.  Upstream gradients are device memory.
 * ------------------------------------------------------------------------ */
#define CY_PRIOR_DAE 0   /* cy_dae_* */
#define CY_PRIOR_ORTHO 1 /* cy_ortho_* */
#define CY_PRIOR_ACT_SIGMOID 0
#define CY_PRIOR_ACT_TANH 1
/* The launch rule of both groups (host-side only, launches nothing; the launches take every decision from it), in the
 * style of cy_mix_plan.  DAE: n = npix, C = Cimg, `align` = the bytes the logits' base is aligned to (16 and more count
 * as 16).  Orthogonality: K prototypes of C floats; n and align are not looked at.
 * Returns what the launches answer: CY_ERR_ARG for a NULL `out`, an unknown form, npix < 1, C < 1 (orthogonality) or
 * an align that is no multiple of 4; CY_ERR_SHAPE for K outside 2..64, Cimg outside 1..4 or K * C > 16384. */
typedef struct cy_prior_plan_t {
  int32_t variant;   /* DAE: the compiled K (2, 4, 8) where the rows are aligned to their 8 / 16 bytes, else 0 (run-time
                        K, the row read 16 floats at a time).  Orthogonality: 0 = a thread per Gram entry (C <= 64),
                        1 = a wave */
  int32_t vec;       /* floats per access of a logits row: 2 (variant 2), 4 (variants 4, 8; variant 0 where K % 4 == 0
                        on a 16-byte base), else 1.  Orthogonality: 1 */
  int32_t fwd_grid;  /* DAE: min(1024, ceil(npix / 256)) blocks = the f64 partials per quantity.  Orthogonality: 1 */
  int32_t fwd_trips; /* DAE: loop trips of the busiest block.  Orthogonality: trips of the Gram loop (ceil(K^2 / 256),
                        or ceil(K^2 / 4) for the wave form) */
  int32_t bwd_grid;  /* as fwd_grid */
  int32_t bwd_trips; /* DAE: loop trips of the busiest block.  Orthogonality: trips of the sweeps over [K][C]
                        (ceil(K C / 256)) */
  int32_t k_chunks;  /* DAE: 16-float pieces a row is read in: ceil(K / 16) for variant 0, else 1.  Orthogonality: 0 */
  int32_t fwd_lds;   /* bytes of LDS per block: static for DAE, dynamic for orthogonality (rows) */
  int32_t bwd_lds;   /* ... (orthogonality: rows and the K x K matrix) */
  int32_t aux;       /* DAE: the threads of a block that work in the backward's flat sweep, floor(256 / K) * K.
                        Orthogonality: the floats between two rows in LDS (C | 1 for the thread form, C for the wave
                        form) */
} cy_prior_plan_t;
int cy_prior_plan(int form, long n, int K, int C, int align, cy_prior_plan_t* out);
/* The denoising-auto-encoder prior (semi_seg/hooks/autoencoder.py:52-57: F.mse_loss(AuxiliaryLayer(logits), image),
 * the layer a 1x1 convolution K -> 1 and a sigmoid or tanh).  Logits are [npix][K] f32 rows (NHWC), npix = N * HW,
 * 2 <= K <= 64; w[K], b[1] f32; image [N][Cimg][HW] f32 planar, 1 <= Cimg <= 4; act CY_PRIOR_ACT_*.
 *   r_p = act(b + sum_k w_k z_pk) (the sum in f64);  loss[0] = sum_p sum_c (r_p - image_pc)^2 / (npix Cimg):
 * the one-channel reconstruction broadcasts over the image's channels as F.mse_loss broadcasts it.
 * Backward, with g_p = 2 gscale[0] act'(.) sum_c (r_p - image_pc) / (npix Cimg):  dlogits_pk = g_p w_k,
 * dw_k = sum_p g_p z_pk, db = sum_p g_p (f64 per block, then in block order).  The image carries no gradient.
 * ws_bytes >= 8 * min(1024, ceil(npix / 256)) forward, (K + 1) times that backward = cy_dae_ws_bytes (0 for a
 * count < 1). */
size_t cy_dae_ws_bytes(long npix, int K, int backward);
int cy_dae_fwd(const float* logits, const float* w, const float* b, const float* image, float* loss, int N, long HW,
               int K, int Cimg, int act, void* ws, size_t ws_bytes, void* stream);
int cy_dae_bwd(const float* logits, const float* w, const float* b, const float* image, const float* gscale,
               float* dlogits, float* dw, float* db, int N, long HW, int K, int Cimg, int act, void* ws,
               size_t ws_bytes, void* stream);
/* The orthogonal-prototype regulariser (semi_seg/hooks/orthogonal.py:45-50).  prototypes [K][C] f32, 2 <= K <= 64,
 * K * C <= 16384:  n_i = v_i / max(|v_i|_2, 1e-12), G = n n^T, loss[0] = sum (G - I)^2 / K^2.  One block each way; the
 * backward recomputes n and G and writes dprototypes [K][C] = gscale[0] dloss/dv (a row whose norm was clamped gets
 * the clamped quotient's derivative, 1e12 times the gradient of its n, as torch gives it). */
int cy_ortho_fwd(const float* prototypes, float* loss, int K, int C, void* stream);
int cy_ortho_bwd(const float* prototypes, const float* gscale, float* dprototypes, int K, int C, void* stream);

/* ------------------------------------------------------------------------
 * Differentiable mean teacher (csrc/cy_teacher.hip; entries added to ABI v18).
 * The teacher's state lives in flat f32 buffers; every update of it is one
 * streaming launch.  Every entry checks its arguments before any launch: a NULL pointer, a count < 1, step < 1 or a
 * base that is not 4-byte aligned -> CY_ERR_ARG; K or the tensor count out of range -> CY_ERR_SHAPE; a short workspace
 * -> CY_ERR_WORKSPACE.  No atomics: two runs give the same bits.
 * ------------------------------------------------------------------------ */
#define CY_TEACHER_ADAM 0      /* cy_adam_step */
#define CY_TEACHER_AXPY 1      /* cy_axpy */
#define CY_TEACHER_EMA_MULTI 2 /* cy_ema_update_multi */
#define CY_TEACHER_GATHERMSE 3 /* cy_softmax_gathermse_* */
/* The launch rule of the four families (host-side only, launches nothing; the launches take every decision from it), in
 * the style of cy_mix_plan.  `n`: the elements (Adam, axpy), the tensors (multi-tensor EMA) or the pixels N * HW
 * (gather-MSE).  `align`: the bytes every tensor base of the call is aligned to (16 and more count as 16).  K is looked
 * at by gather-MSE only.
 * Returns what the launches answer: CY_ERR_ARG for a NULL `out`, an unknown form, n < 1 or an align that is no multiple
 * of 4; CY_ERR_SHAPE for more than 4096 tensors or K outside 2..16. */
typedef struct cy_teacher_plan_t {
  int32_t variant;   /* gather-MSE: the compiled K (2, 4, 8) where the rows are aligned to their 8 / 16 bytes, else 0
                        (run-time K, one float at a time, any 4-byte-aligned base).  Otherwise 0 */
  int32_t vec;       /* floats per memory access.  Adam, axpy: 4 where align is a multiple of 16 and n >= 4 (the n % 4
                        tail goes one float at a time), else 1.  Multi-tensor EMA: 1.  Gather-MSE: 2 (variant 2),
                        4 (variants 4, 8), 1 */
  int32_t fwd_grid;  /* Adam, axpy: min(2048, ceil(n / vec / 256)) blocks.  Multi-tensor EMA: the blocks striding over
                        one tensor, clamp(8192 / n, 2, 64).  Gather-MSE: min(1024, ceil(n / 256)) blocks = the f64
                        partials */
  int32_t fwd_trips; /* loop trips of the busiest block; multi-tensor EMA (the sizes are device data): the elements of
                        a tensor that one trip covers, 256 * fwd_grid */
  int32_t bwd_grid;  /* gather-MSE: 2 * fwd_grid; otherwise 0 */
  int32_t bwd_trips; /* gather-MSE; otherwise 0 */
  int32_t rows;      /* multi-tensor EMA: the grid's second dimension = n; otherwise 0 */
} cy_teacher_plan_t;
int cy_teacher_plan(int form, long n, int K, int align, cy_teacher_plan_t* out);
/* torch.optim.Adam(amsgrad=False, maximize=False) on flat f32 buffers of n elements; `step` is the 1-based count after
 * this update.  g += wd p (wd != 0);  m += (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g^2;
 * p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), bc_i = 1 - beta_i^step formed in f64 on the host as cy_radam_step
 * forms them, lr / bc1 and sqrt(bc2) rounded to f32 once. */
int cy_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1,
                 float beta2, float eps, float weight_decay, long step, void* stream);
/* y += a x over flat f32 buffers of n elements, one fused multiply-add per element. */
int cy_axpy(float* y, const float* x, long n, float a, void* stream);
/* The expression of cy_ema_update, bit for bit, over `count` tensors in one launch.  `table` is [count][3] int64 in
 * device memory, 8-byte aligned: the teacher tensor's address, the student's, the number of f32 elements; a row with a
 * null address or a count < 1 is skipped.  1 <= count <= 4096, anything else is CY_ERR_SHAPE. */
int cy_ema_update_multi(const int64_t* table, int count, float alpha, float weight_decay, void* stream);
/* The consistency term of the differentiable mean teacher (semi_seg/hooks/dmt.py:177-197): the MSE of softmax(student)
 * against the teacher's probabilities warped by the step's nearest-neighbour affine map with zero padding.  teacher and
 * student are f32 logits [N][HW][K] (NHWC rows), the teacher's unwarped; map is int32 [N][HW]: the source pixel in
 * [0, HW) of the same image, or -1 (any value outside [0, HW)) for a source outside the image.
 *   q = softmax(teacher[n][map[n][hw]]) or the all-zero vector outside;  loss[0] = sum (q_k - softmax(s)_k)^2 / (npix K)
 * Backward, student only, p = softmax(s):  ds_k = gscale[0] (2 / (npix K)) p_k ((p_k - q_k) - sum_j p_j (p_j - q_j)).
 * 2 <= K <= 16.  ws_bytes >= 8 * min(1024, ceil(npix / 256)) = cy_softmax_gathermse_ws_bytes (0 for a count < 1). */
size_t cy_softmax_gathermse_ws_bytes(int N, long HW);
int cy_softmax_gathermse_fwd(const float* teacher, const int32_t* map, const float* student, float* loss, int N,
                             long HW, int K, void* ws, size_t ws_bytes, void* stream);
int cy_softmax_gathermse_bwd(const float* teacher, const int32_t* map, const float* student, const float* gscale,
                             float* dstudent, int N, long HW, int K, void* stream);

/* ------------------------------------------------------------------------
 * SGD, Adam and AdamW on the flat buffers (csrc/cy_optim.hip; entries added to ABI v18).  They replace torch.optim.SGD / Adam / AdamW's per-tensor (or
 * foreach) step in contrastyou/optim: FusedSGD, FusedAdam(amsgrad=True) and FusedAdamW launch them once per run of
 * updated parameters (contrastyou/optim/flat_optimizer.py: FlatOptimizer.step); FusedAdam(amsgrad=False) keeps
 * cy_adam_step.  Every entry checks its arguments before any launch: a NULL pointer, n < 1, step < 1, a base that is
 * not 4-byte aligned -> CY_ERR_ARG, as cy_adam_step answers.  The gradient is read only.  No atomics: two runs give the
 * same bits.  HBM-bound: 20 B/element for SGD with momentum (12 without), 28 for Adam(W), 36 with amsgrad.
 * ------------------------------------------------------------------------ */
#define CY_OPTIM_SGD 0   /* cy_sgd_step */
#define CY_OPTIM_ADAMW 1 /* cy_adamw_step */
/* The launch rule of the two (host-side only, launches nothing; the launches take every decision from it): the rule
 * cy_teacher_plan gives CY_TEACHER_ADAM.  `align`: the bytes every buffer base of the call is aligned to (16 and more
 * count as 16).
 * CY_ERR_ARG for a NULL `out`, an unknown form, n < 1 or an align that is no multiple of 4. */
typedef struct cy_optim_plan_t {
  int32_t vec;   /* floats per memory access: 4 where align is a multiple of 16 and n >= 4, else 1 -- a run of touched
                    parameters starts at an arbitrary parameter offset, so training reaches both */
  int32_t grid;  /* min(2048, ceil(n / vec / 256)) blocks of 256 */
  int32_t trips; /* loop trips of the busiest block */
  int32_t tail;  /* the n % 4 elements that the first threads of block 0 finish one float at a time (vec == 4), else 0 */
} cy_optim_plan_t;
int cy_optim_plan(int form, long n, int align, cy_optim_plan_t* out);
/* torch.optim.SGD(maximize=False) on flat f32 buffers of n elements.  g += wd p (wd != 0); with momentum:
 * buf = g when `first` (the buffer's content is not read), else buf = momentum buf + (1 - dampening) g; then
 * g += momentum buf (nesterov) or g = buf;  p -= lr g.  `momentum_buf` is NULL exactly when momentum == 0: any other
 * pairing is CY_ERR_ARG. */
int cy_sgd_step(float* param, const float* grad, float* momentum_buf, long n, float lr, float momentum,
                float dampening, float weight_decay, int nesterov, int first, void* stream);
/* torch.optim.AdamW (decoupled = 1: p *= 1 - lr wd first, no L2 term) or torch.optim.Adam (decoupled = 0: g += wd p) on
 * flat f32 buffers of n elements; `step` is the 1-based count after this update.  A non-NULL `max_exp_avg_sq` is
 * amsgrad: vmax = max(vmax, v) and the denominator is sqrt(vmax) / sqrt(bc2) + eps.  Moments, bias corrections and the
 * update are cy_adam_step's, term for term (bc_i in f64 on the host, lr / bc1 and sqrt(bc2) rounded to f32 once);
 * 1 - lr wd is formed in f64 and rounded to f32 once. */
int cy_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, long n,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled, long step,
                  void* stream);

/* ------------------------------------------------------------------------
 * Wide-K regularisers (csrc/cy_wide_reg.hip; entries added to ABI v18).  The entropy, self-MSE, UA-MT and ICT losses above on multi-prototype logits,
 * 16 < K <= 64: the same arguments, values and launch counts as cy_softmax_entropy_*, cy_softmax_selfmse_*,
 * cy_uamt_mse_* and cy_softmax_mixmse_*, in the sixteen-lanes-per-pixel form of cy_softmax_group_kl_* (lane j of a row
 * holds logits 4j..4j+3; 16 pixels per block and loop trip).  The arg-max of self-MSE and hard UA-MT is the first
 * maximal index.  Every entry checks its arguments before any launch: a NULL pointer, a count < 1 or a base that is not
 * 4-byte aligned -> CY_ERR_ARG; K outside 17..64 -> CY_ERR_SHAPE (the entries above keep K <= 16); a short workspace ->
 * CY_ERR_WORKSPACE.  The forward writes one f64 partial per block (UA-MT two) and one block sums them in block order,
 * the backward is one launch.  No atomics: two runs give the same bits.  Upstream gradients are device memory.
 * ------------------------------------------------------------------------ */
#define CY_WIDE_ENTROPY 0 /* cy_softmax_entropy_row_* */
#define CY_WIDE_SELFMSE 1 /* cy_softmax_selfmse_row_* */
#define CY_WIDE_UAMT 2    /* cy_uamt_mse_row_* */
#define CY_WIDE_MIXMSE 3  /* cy_softmax_mixmse_row_* */
/* The launch rule of the four families (host-side only, launches nothing; the launches take every decision from it), in
 * the style of cy_mix_plan.  `npix`: the pixels N * HW.  `align`: the bytes every tensor base pointer of the call is
 * aligned to (the launches work it out from their pointers; 16 and more count as 16).
 * Returns what the launches answer: CY_ERR_ARG for a NULL `out`, an unknown family, npix < 1 or an align that is no
 * multiple of 4; CY_ERR_SHAPE for K outside 17..64; otherwise CY_OK. */
typedef struct cy_wide_reg_plan_t {
  int32_t vec;            /* floats per memory access: 4 where K % 4 == 0 and align is a multiple of 16, else 1 */
  int32_t rows_per_block; /* pixels a block covers per loop trip, 16 */
  int32_t fwd_grid;       /* min(4096, ceil(npix / 16)) blocks = the f64 partials (UA-MT: two per block) */
  int32_t fwd_trips;      /* loop trips of every block */
  int32_t bwd_grid;       /* = fwd_grid */
  int32_t bwd_trips;
} cy_wide_reg_plan_t;
int cy_wide_reg_plan(int family, long npix, int K, int align, cy_wide_reg_plan_t* out);
/* ws_bytes >= 8 * fwd_grid (16 * fwd_grid for UA-MT) = the *_row_ws_bytes queries (0 for a count < 1). */
size_t cy_softmax_entropy_row_ws_bytes(long npix);
int cy_softmax_entropy_row_fwd(const float* logits, float* loss, long npix, int K, float eps, void* ws,
                               size_t ws_bytes, void* stream);
int cy_softmax_entropy_row_bwd(const float* logits, const float* gscale, float* dlogits, long npix, int K, float eps,
                               void* stream);
size_t cy_softmax_selfmse_row_ws_bytes(long npix);
int cy_softmax_selfmse_row_fwd(const float* logits, float* loss, long npix, int K, void* ws, size_t ws_bytes,
                               void* stream);
int cy_softmax_selfmse_row_bwd(const float* logits, const float* gscale, float* dlogits, long npix, int K,
                               void* stream);
size_t cy_uamt_mse_row_ws_bytes(long npix);
int cy_uamt_mse_row_fwd(const float* teacher, const float* student, float* result, long npix, int K, float thr,
                        int hard, void* ws, size_t ws_bytes, void* stream);
int cy_uamt_mse_row_bwd(const float* teacher, const float* student, const float* result, const float* gscale,
                        float* dstudent, long npix, int K, float thr, int hard, void* stream);
size_t cy_softmax_mixmse_row_ws_bytes(int N, long HW);
int cy_softmax_mixmse_row_fwd(const float* student, const float* teacher, const int32_t* index, float w_self,
                              float w_other, float* loss, int N, long HW, int K, void* ws, size_t ws_bytes,
                              void* stream);
int cy_softmax_mixmse_row_bwd(const float* student, const float* teacher, const int32_t* index, float w_self,
                              float w_other, const float* gscale, float* dstudent, int N, long HW, int K,
                              void* stream);

/* ------------------------------------------------------------------------
 * On-device SLIC superpixels (csrc/cy_slic.hip; 6 entries added to ABI v18).
 * Replaces the offline pass the superpixel InfoNCE hook depends on:
 * skimage.segmentation.slic(img, n_segments=40, sigma=5, compactness=0.1) of script/create_superpixel.py:27
 * (compactness 0.001 in semi_seg/postprocess/superpixel.py:23) and the `superpixel/` folder read by
 * _load_superpixel_image (semi_seg/hooks/infonce.py:24-27).  Not label-for-label skimage: DESIGN.md "On-device
 * superpixels" lists the deviations.  images: f32 [N][H][W] in 0..1.
 *   blur_q   separable Gaussian along H then W, radius r = int(4 sigma + 0.5), weights exp(-0.5 (i/sigma)^2)
 *            normalised in f64 then cast to f32, scipy.ndimage's `reflect` boundary, taps i = -r..r accumulated in
 *            order in f32 (product and sum rounded separately); sigma == 0 skips the blur.
 *            q = floor(clamp(v,0,1) * 65535 + 0.5) of the f32 value v, evaluated exactly (in f64);
 *            int32 [N][H][W].
 *   grid     s = sqrt(H W / n_segments) (f64), S = s rounded half to even, start = floor(s / 2); centres at
 *            y = start + i S < H, x = start + j S < W, k row-major, K of them; cq_k = q there.
 *   cluster  max_iter rounds, all of them.  Labels start at 0.  Assignment: among the centres with |y - cy_k| <= 2S and
 *            |x - cx_k| <= 2S the smallest (q - cq_k)^2 S^2 + (dy^2 + dx^2) M^2 (int64), M = compactness * 65535 rounded
 *            half to even, ties to the smallest k; a pixel no window covers keeps its label.  Update: cnt and the int64
 *            sums of y, x, q per label; c = (2 sum + cnt) / (2 cnt); cnt == 0 leaves the centre.
 *            labels int32 [N][H][W]; centres int32 [N][K][3] = (cy, cx, cq) after the last update.
 *   connect  4-connected components of equal label, root = smallest linear index; min_size = (H W) / (2 K); a
 *            component with size >= min_size or root 0 is kept, any other takes the final id of the component owning the
 *            pixel left of its root (above it when the root is in column 0); sizes are each component's own; kept
 *            components are numbered 0, 1, ... by increasing root.  ids uint8 [N][H][W], count int32 [N] (< 208).
 *            Any int32 label map is accepted.
 * cy_slic is the three stages through the workspace.  Everything goes onto `stream`; no host read, no allocation;
 * integer sums only after the blur, so two runs give the same bits.
 * Checked before any launch, in this order: a NULL pointer or max_iter < 0 -> CY_ERR_ARG; N < 1 -> CY_ERR_ARG, H or W
 * outside 1..CY_SLIC_MAX_SIDE or N > 65535 -> CY_ERR_SHAPE; a negative or NaN sigma -> CY_ERR_ARG, sigma >
 * CY_SLIC_MAX_SIGMA or r > min(H, W) -> CY_ERR_SHAPE; a non-finite compactness or M outside 1..65535 -> CY_ERR_ARG;
 * n_segments < 1 -> CY_ERR_ARG, S < 1, K outside 1..CY_SLIC_MAX_K or H W < 64 K -> CY_ERR_SHAPE; a short workspace ->
 * CY_ERR_WORKSPACE.  Each stage checks the arguments it takes.  cy_slic_ws_bytes (one size for all four entries;
 * blur_q alone needs N H W 4 bytes) is 0 where the sizes are refused.
 * cy_slic_plan fills a cy_slic_plan_t (all 0 but `status` where the call is refused) and returns the status cy_slic
 * would: the geometry, the blur form with its grid and LDS bytes per pass, the grid of the per-pixel kernels
 * (assignment and the components; blocks of 256, grid.y = N), the tiles of 1024 pixels the numbering block steps
 * through and the number of launches.
 * ------------------------------------------------------------------------ */
#define CY_SLIC_MAX_SIDE 1024
#define CY_SLIC_MAX_K 100
#define CY_SLIC_MAX_SIGMA 16
#define CY_SLIC_BLUR_QUANT 0    /* sigma == 0: slic_quant_kernel */
#define CY_SLIC_BLUR_TWO_PASS 1 /* slic_blur_kernel along H, then along W with the quantisation */
typedef struct cy_slic_plan_t {
  int32_t status;                   /* the refusal (CY_OK: none) */
  int32_t r, S, start, Ky, Kx, K, M, min_size; /* the geometry */
  int32_t blur_form;                /* CY_SLIC_BLUR_* */
  int32_t blur_grid_x, blur_grid_y; /* the blur's grid */
  int32_t blur_lds_h, blur_lds_w;   /* LDS bytes of the pass along H and of the pass along W */
  int32_t pixel_grid_x;             /* the grid of the per-pixel kernels (blocks of 256, grid.y = N) */
  int32_t assign_lds;               /* LDS bytes of the assignment */
  int32_t update_grid;              /* blocks of the centre update */
  int32_t scan_tiles;               /* tiles of 1024 pixels the numbering block steps through */
  int32_t launches;
} cy_slic_plan_t;
size_t cy_slic_ws_bytes(int N, int H, int W, int n_segments);
int cy_slic_plan(int N, int H, int W, int n_segments, double sigma, double compactness, int max_iter,
                 cy_slic_plan_t* out);
int cy_slic_blur_q(const float* images, int32_t* q, int N, int H, int W, double sigma, void* ws, size_t ws_bytes,
                   void* stream);
int cy_slic_cluster(const int32_t* q, int32_t* labels, int32_t* centres, int N, int H, int W, int n_segments,
                    double compactness, int max_iter, void* ws, size_t ws_bytes, void* stream);
int cy_slic_connect(const int32_t* labels, uint8_t* ids, int32_t* count, int N, int H, int W, int n_segments, void* ws,
                    size_t ws_bytes, void* stream);
int cy_slic(const float* images, uint8_t* ids, int32_t* count, int N, int H, int W, int n_segments, double sigma,
            double compactness, int max_iter, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * On-device loader augmentation (csrc/cy_augment.hip; 2 entries added to ABI v18).  Replaces the host-side Pillow / torchvision pipelines of semi_seg/augment.py:36-283
 * (augment_zoo) as contrastyou/augment/synchronize.py:76-165 applies them: the *application* of given parameters is
 * Pillow's bit for bit (Image.rotate BILINEAR / NEAREST, transpose, ImageOps.expand, crop, ImageEnhance.Brightness and
 * .Contrast, ToTensor, ToLabel); the parameters are drawn on the host (contrastyou/augment/device.py).
 * Store: store_img / store_lab are uint8 arenas of arena_bytes each; slice s is the H x W row-major block at byte
 * h_table[3s] with (H, W) = h_table[3s+1], h_table[3s+2] in both arenas (int64 [slices][3], on the HOST: the device
 * never reads a table, each record carries the row of its slice).
 * One record per output view v, the same for the image and for the label of the view:
 *   ip[v][CY_AUG_IP_LEN] int32   SLICE, and its table row as OFF_LO, OFF_HI (the low and high 32 bits of the byte
 *                                offset), SRC_H, SRC_W: what the kernel reads; the pre-window PY, PX, CH, CW: canvas c[y][x] = source[y+PY][x+PX], 0 outside
 *                                the source; ROT 0/1 with A0..A5 = Pillow's FIX() of the matrix (below); FLIPV, FLIPH
 *                                0/1, applied to the rotated canvas; the post-window QY, QX: out[y][x] = pixel
 *                                (y+QY, x+QX) of the rotated and flipped canvas, 0 outside it; NJIT 0..3 and KIND0..2
 *                                (CY_AUG_BRIGHTNESS / CY_AUG_CONTRAST) in the order they are applied.
 *   fp[v][CY_AUG_FP_LEN] double  M0..M5, the matrix exactly as Image.rotate computes it for the CH x CW canvas
 *                                (x_in = M0 x + M1 y + M2, y_in = M3 x + M4 y + M5); F0..F2, the jitter factors (f32
 *                                values held in doubles).
 * Stage A (aug_geometry_kernel, blocks of CY_AUG_GEO_BLOCK output pixels, grid.y = views, grid.z = image / label):
 * walks output -> post-window -> flips -> rotation -> canvas -> source.
 *   label, ROT:  xin = (A2 + y A1 + x A0) >> 16, yin = (A5 + y A4 + x A3) >> 16 (int64, arithmetic shift); c[yin][xin]
 *                inside the canvas, else 0 (affine_fixed, nearest).  A0, A1, A3, A4 = FIX(M0, M1, M3, M4),
 *                A2 = FIX(M2 + M0 0.5 + M1 0.5), A5 = FIX(M5 + M3 0.5 + M4 0.5), FIX(v) = floor(v 65536 + 0.5): the
 *                host computes them, the kernel holds integers only.
 *   image, ROT:  xin = M0 (x+0.5) + M1 (y+0.5) + M2, yin likewise (f64, every product and sum rounded on its own, no
 *                fma); outside [0,CW) x [0,CH) -> 0; else xin -= 0.5, yin -= 0.5, x0 = floor(xin), dx = xin - x0 (y
 *                alike), columns and the first row clamped to the canvas, v1 = a + dx (b - a) on row y0, v2 the same on
 *                row y0+1 when that is inside the canvas, else v1; (uint8)(v1 + dy (v2 - v1)) (bilinear_filter8).
 *   labels go through label_lut (uint8 [256]: ToLabel's mapping) into labels int64 [views][out_h][out_w]; images as
 *   uint8 into scratch [views][out_h][out_w].
 * Stage B (aug_jitter_kernel, one block of CY_AUG_JIT_BLOCK threads per view): the jitter steps are maps of 0..255, so
 * the block composes them into one 256-entry table and reads the scratch once per contrast step (its mean) and once to
 * write.  Brightness: t = (uint8) clip(trunc(F (float)t), 0, 255).  Contrast: mean = (2 sum + count) / (2 count) of
 * the current image in integers, t = (uint8) clip(trunc((float)mean + F ((float)t - (float)mean)), 0, 255), f32, each
 * operation rounded on its own.  images[v] = tensor_lut[t[scratch]] (f32 [256]: ToTensor's i / 255, computed by the
 * caller) as f32 [views][out_h][out_w].
 * store_lab and labels may both be NULL: image views only.  Everything goes onto `stream`; no host read of device
 * memory, no allocation, no atomics; two runs give the same bits.
 * Checked on the host before any launch, from h_table and h_ip (the host copy of ip; nothing is read through the
 * device pointers, and what the kernel reads of the store is in the records that were checked): a NULL pointer (but the label pair), or only one of store_lab / labels -> CY_ERR_ARG; views
 * outside 1..CY_AUG_MAX_VIEWS, out_h or out_w outside 1..CY_AUG_MAX_OUT, slices < 1 -> CY_ERR_SHAPE; per view: SLICE
 * outside the table, a table row with H or W outside 1..CY_AUG_MAX_SIDE or leaving the arena, CH or CW outside
 * 1..CY_AUG_MAX_SIDE, an offset beyond +-CY_AUG_MAX_OFFSET -> CY_ERR_SHAPE; OFF_LO, OFF_HI, SRC_H, SRC_W that are not
 * the table row of SLICE, a flag that is not 0 / 1, NJIT outside 0..3, an unknown KIND -> CY_ERR_ARG; scratch_bytes < views out_h out_w -> CY_ERR_WORKSPACE.
 * cy_aug_plan fills a cy_aug_plan_t (all 0 but `status` where the sizes are refused) and returns the status the sizes
 * alone decide: the kernel form, both grids, the trips of stage B's block over a view, its LDS bytes, the scratch
 * bytes and the number of launches.
 * ------------------------------------------------------------------------ */
#define CY_AUG_MAX_SIDE 1024
#define CY_AUG_MAX_OUT 512
#define CY_AUG_MAX_VIEWS 4096
#define CY_AUG_MAX_OFFSET 4096
#define CY_AUG_GEO_BLOCK 256
#define CY_AUG_JIT_BLOCK 1024
#define CY_AUG_BRIGHTNESS 1
#define CY_AUG_CONTRAST 2
#define CY_AUG_FORM_TWO_STAGE 0 /* aug_geometry_kernel then aug_jitter_kernel: the only form */
#define CY_AUG_IP_LEN 24
#define CY_AUG_IP_SLICE 0
#define CY_AUG_IP_PY 1
#define CY_AUG_IP_PX 2
#define CY_AUG_IP_CH 3
#define CY_AUG_IP_CW 4
#define CY_AUG_IP_ROT 5
#define CY_AUG_IP_FLIPV 6
#define CY_AUG_IP_FLIPH 7
#define CY_AUG_IP_QY 8
#define CY_AUG_IP_QX 9
#define CY_AUG_IP_NJIT 10
#define CY_AUG_IP_KIND0 11
#define CY_AUG_IP_A0 14
#define CY_AUG_IP_OFF_LO 20
#define CY_AUG_IP_OFF_HI 21
#define CY_AUG_IP_SRC_H 22
#define CY_AUG_IP_SRC_W 23
#define CY_AUG_FP_LEN 9
#define CY_AUG_FP_M0 0
#define CY_AUG_FP_F0 6
typedef struct cy_aug_plan_t {
  int32_t status;                 /* the refusal (CY_OK: none) */
  int32_t form;                   /* CY_AUG_FORM_* */
  int32_t geo_grid_x, geo_grid_y; /* stage A: blocks of CY_AUG_GEO_BLOCK output pixels, the views */
  int32_t geo_grid_z;             /* 2: the plan is that of the call with labels; without them the launch has 1 */
  int32_t jit_grid;               /* stage B: one block per view */
  int32_t jit_trips;              /* trips of stage B's block over a view */
  int32_t jit_lds;                /* its LDS bytes */
  int32_t scratch_bytes;
  int32_t launches;
} cy_aug_plan_t;
int cy_aug_plan(int views, int out_h, int out_w, cy_aug_plan_t* out);
int cy_aug_views(const uint8_t* store_img, const uint8_t* store_lab, const int64_t* h_table, int slices,
                 long long arena_bytes, const int32_t* ip, const int32_t* h_ip, const double* fp, int views, int out_h,
                 int out_w, const uint8_t* label_lut, const float* tensor_lut, float* images, int64_t* labels,
                 uint8_t* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CONTRASTYOU_HIP_H */
