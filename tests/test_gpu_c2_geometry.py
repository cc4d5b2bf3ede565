"""Parity of the conv kernels AT THE BENCHMARKED GEOMETRIES: the 3x3 layers of UNet(max_channel=512)
(contrastyou/arch/unet.py:72-103) at the image sizes, batch sizes and storage types of bench.py's three workloads
(tests/c2_layers.py WORKLOADS) -- c2: 224 x 224, N = 16 (labeled pass) and 32 (unlabeled pass), bf16; c4: 256 x 256,
N = 16 and 32, fp16; c5: the nine encoder layers at N = 512 (256 slices x 2 views), bf16 -- forward + BN statistics
(partial rows, and on accumulators the way the step takes them, incl. the consumer's fold= prologue), data gradient
(concat layers also in the two-tensor form of the step), weight gradient, and the paired weight gradient of the encoder
(both passes of a two-stage step in one launch) -- against torch's CPU convolution on the same 16-bit-representable
inputs.  Each case takes its launch plans from the queries tests/test_plan_coverage.py uses and asserts what a launch
shows of them; that file checks (on the CPU) that the cases below cover every plan of the three workloads.
Also: the C4 geometry in bf16 (N = 4), one layer just above the 2 GiB limit of the 32-bit-offset kernels, and one
full-size f32 C2 step against the oracle.

Reference: chunk of images by chunk of images (N = 512 does not fit as f32 otherwise); forward and data gradient are
compared per chunk, the weight gradient and the per-channel sums are accumulated over the chunks in float64.

Tolerance: 16-bit storage, f32 accumulation: 1.2e-2 (bf16) / 2e-3 (fp16) of the tensor's max magnitude for activations
(one rounding of the output + accumulation-order noise), 2e-3 for f32 weight gradients, 1e-4 for the statistics against
the f64 sums of the output the kernel wrote.  The statistics against the REFERENCE's f64 sums: every output value is off
by at most the activation tolerance of its own magnitude, so the mean is within that share of the channel's RMS and the
mean square within that share of itself -- the activation tolerance, relative to max RMS / max mean square."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import c2_layers as cl
from tests.bn_acc_checks import assert_acc_equals_partial_rows, assert_fold_matches_scale_shift

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
EPS = 1e-5


def nhwc(t, dtype=None):
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def cpu(t):
    return t.detach().float().cpu()


def assert_close(a, b, rel, what, scale=None):
    a, b = cpu(a), b.detach().float().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = (b.abs().max().item() if scale is None else scale) + 1e-30
    err = (a - b).abs().max().item()
    assert err <= rel * scale, f"{what}: max err {err:.3e} > {rel:.1e} * {scale:.3e}"


def act_tol(dtype):
    return {BF: 1.2e-2, torch.float16: 2e-3}.get(dtype, 2e-5)


def _chunks(N, layer):
    """image ranges of the reference: at most 2^26 elements of the widest tensor per chunk (256 MB as f32), at least 32
    images (the cases at N <= 32 are one chunk)"""
    name, H, C1, C2, Cout, mode, pro = layer
    per_image = H * H * max(C1 + C2, Cout)
    n = max(32, (1 << 26) // per_image)
    return [(i, min(i + n, N)) for i in range(0, N, n)]


class _Inputs:
    """the inputs of one case, drawn chunk by chunk from seeded generators (chunk j of any N is the same images); chunk 0
    also draws the weights, between the sources and dy"""

    def __init__(self, N, layer, dtype, seed):
        self.N, self.layer, self.dtype, self.seed = N, layer, dtype, seed
        self.chunks = _chunks(N, layer)
        self.w = self.extra = None

    def chunk(self, j):
        """(x1, x2, dy) of chunk j as f32 holding `dtype`-representable values"""
        name, H, C1, C2, Cout, mode, pro = self.layer
        i0, i1 = self.chunks[j]
        n = i1 - i0
        g = torch.Generator().manual_seed(self.seed + 7919 * j)
        r = lambda *s: (torch.rand(*s, generator=g) * 2 - 1)  # noqa: E731
        dt = self.dtype
        sh = 2 * H if mode == 1 else (H // 2 if mode == 2 else H)
        x1 = r(n, C1, sh, sh).to(dt).float()
        x2 = r(n, C2, H, H).to(dt).float() if C2 else None
        w = (r(Cout, C1 + C2, 3, 3) / math.sqrt(9 * (C1 + C2))).to(dt).float() if j == 0 else None
        dy = r(n, Cout, H, H).to(dt).float()
        if j == 0 and self.w is None:
            self.w = w
            if pro:  # the producer conv's weights and the BatchNorm's affine parameters
                self.extra = ((r(C1, C1, 3, 3) / math.sqrt(9 * C1)).to(dt).float(), r(C1) * 0.5 + 1.0, r(C1) * 0.5)
        return x1, x2, dy


def _conv_input(x1, x2, mode, scale, shift, dtype):
    a = x1
    if scale is not None:  # the kernel rounds relu(scale*x+shift) to the storage type before the MFMA
        a = F.relu(a * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).to(dtype).float()
    if mode == 1:
        a = F.max_pool2d(a, 2, 2)
    elif mode == 2:
        a = F.interpolate(a, scale_factor=2, mode="nearest")
    if x2 is not None:
        a = torch.cat((a, x2), 1)
    return a


def _reference_chunk(a_in, w, dy):
    """(conv output, data gradient, weight gradient) of one chunk of images in f32 on the CPU"""
    wv = w.clone().requires_grad_(True)
    ref = F.conv2d(a_in, wv, None, 1, 1)
    (ref * dy).sum().backward()
    return ref.detach(), F.conv_transpose2d(dy, w, None, 1, 1), wv.grad


def _to_gpu(inp):
    """the inputs of a case as NHWC tensors on the GPU, uploaded chunk by chunk (nothing of size N stays on the host)"""
    from cyhip import ops
    name, H, C1, C2, Cout, mode, pro = inp.layer
    N, dt = inp.N, inp.dtype
    if len(inp.chunks) == 1:
        x1, x2, dy = inp.chunk(0)
        return nhwc(x1, dt), (None if x2 is None else nhwc(x2, dt)), nhwc(dy, dt)
    sh = 2 * H if mode == 1 else (H // 2 if mode == 2 else H)
    g1 = ops.empty_nhwc(N, C1, sh, sh, dt, DEV)
    g2 = ops.empty_nhwc(N, C2, H, H, dt, DEV) if C2 else None
    gdy = ops.empty_nhwc(N, Cout, H, H, dt, DEV)
    for j, (i0, i1) in enumerate(inp.chunks):
        x1, x2, dy = inp.chunk(j)
        g1[i0:i1].copy_(nhwc(x1, dt))
        if C2:
            g2[i0:i1].copy_(nhwc(x2, dt))
        gdy[i0:i1].copy_(nhwc(dy, dt))
        del x1, x2, dy
    return g1, g2, gdy


def _run_layer(N, layer, dtype, seed, expect_kernel=None, expect_wgrad=None):
    """one layer at N images: every launch form of the step against the chunked CPU reference.  Returns the plans."""
    from cyhip import ops
    name, H, C1, C2, Cout, mode, pro = layer
    plans = cl.layer_plans(layer, N, dtype)
    plan, dplan, wplan = plans["fwd"], plans["dgrad"], plans["wgrad"]
    if expect_kernel is not None:
        assert plan["kernel"] in expect_kernel, (name, plan)
    if expect_wgrad is not None:
        for k, v in expect_wgrad.items():
            assert wplan[k] == v, (name, k, wplan)
    for k, p in plans.items():
        if k == "wgrad":
            continue
        # split-K leaves through an f32 workspace (ksplit slabs of the output) and conv_splitk_finish_kernel; the other
        # plans take no workspace
        if p["ksplit"] > 1:
            assert p["ws_bytes"] >= p["ksplit"] * N * H * H * (Cout if k == "fwd" else C1 + C2) * 4, (name, k, p)
        else:
            assert p["ws_bytes"] == 0, (name, k, p)
    tol = act_tol(dtype)
    sixteen = dtype in (BF, torch.float16)
    inp = _Inputs(N, layer, dtype, seed)
    g1, g2, gdy = _to_gpu(inp)
    w = inp.w
    wf, wd = ops.pack_weights(w.to(DEV), dtype)
    scale = shift = None
    cnt = N * H * H
    if pro:
        # the layer reads relu(bn(y)) of the conv before it: produce y with a conv of the same shape, take its batch
        # statistics both ways (partial rows -> finalize launch -> scale / shift; accumulator -> fold= in the consumer)
        w0, gm, bt = inp.extra
        wf0, _ = ops.pack_weights(w0.to(DEV), dtype, want_dgrad=False)
        gm, bt = gm.to(DEV), bt.to(DEV)
        ya, part0 = ops.conv3x3_fwd(g1, None, wf0, C1)
        ya2, acc0 = ops.conv3x3_fwd(g1, None, wf0, C1, stats_acc=True)
        assert torch.equal(ya, ya2), f"{name} N={N}: producer output differs between the two statistics forms"
        rm, rv = torch.zeros(C1, device=DEV), torch.ones(C1, device=DEV)
        scale, shift, _, _ = ops.bn_finalize(part0, cnt, gm, bt, rm, rv, 0.1, EPS, True, True, C1, DEV)
        fold = ops.BnState(acc0, gm, bt, cnt, EPS, DEV)
        g1 = ya
        del ya2
    kw = dict(mode=mode, scale=scale, shift=shift)
    # ---- the launches
    out, stats = ops.conv3x3_fwd(g1, g2, wf, Cout, **kw)
    assert stats.shape[0] == plan["partials"], (name, stats.shape, plan)
    out_a, acc = ops.conv3x3_fwd(g1, g2, wf, Cout, stats_acc=True, **kw)
    assert torch.equal(out, out_a), f"{name} N={N}: output differs between partial rows and accumulator"
    del out_a
    a1, a2 = assert_acc_equals_partial_rows(acc, stats, plan["kernel"] == "conv3x3_stream_kernel", f"{name} N={N}")
    if pro:
        out_f, _ = ops.conv3x3_fwd(g1, None, wf, Cout, fold=fold, want_stats=False)
        assert_fold_matches_scale_shift(out_f, out, dtype, f"{name} N={N} {plan}")
        del out_f
    din, _ = ops.conv3x3_fwd(gdy, None, wd, C1 + C2, want_stats=False)
    if C2:  # the data gradient of a concat layer leaves as two tensors (skip branch / upsampled branch)
        (d1, d2), _ = ops.conv3x3_fwd(gdy, None, wd, C1 + C2, want_stats=False, split=C1)
    dw = ops.conv3x3_wgrad(g1, g2, gdy, **kw)
    torch.cuda.synchronize()
    # ---- the reference, chunk by chunk
    sc_c, sh_c = (None, None) if scale is None else (scale.cpu(), shift.cpu())
    dw_ref = torch.zeros(Cout, C1 + C2, 3, 3, dtype=torch.float64)
    r1, r2, o1, o2 = (torch.zeros(Cout, dtype=torch.float64) for _ in range(4))
    for j, (i0, i1) in enumerate(inp.chunks):
        x1, x2, dy = inp.chunk(j)
        if pro:
            x1 = cpu(g1[i0:i1]).contiguous()
        ref, din_ref, dw_c = _reference_chunk(_conv_input(x1, x2, mode, sc_c, sh_c, dtype), w, dy)
        what = f"{name} N={N} images {i0}..{i1 - 1}"
        assert_close(out[i0:i1], ref, tol, f"{what} fwd {plan}")
        assert_close(din[i0:i1], din_ref, tol, f"{what} dgrad {dplan}")
        if C2:
            big = din_ref.abs().max().item()
            assert_close(d1[i0:i1], din_ref[:, :C1], tol, f"{what} dgrad split 1 {plans['dgrad_split']}", scale=big)
            assert_close(d2[i0:i1], din_ref[:, C1:], tol, f"{what} dgrad split 2 {plans['dgrad_split']}", scale=big)
        dw_ref += dw_c.double()
        rd, od = ref.double(), cpu(out[i0:i1]).double()
        r1 += rd.sum(dim=(0, 2, 3))
        r2 += (rd * rd).sum(dim=(0, 2, 3))
        o1 += od.sum(dim=(0, 2, 3))
        o2 += (od * od).sum(dim=(0, 2, 3))
        del x1, x2, dy, ref, din_ref, dw_c, rd, od
    assert_close(dw, dw_ref, 2e-3 if sixteen else 2e-5, f"{name} N={N} wgrad {wplan}")
    s = cpu(stats).double().sum(0)
    for what, got1, got2 in (("partial rows", s[0], s[1]), ("accumulator", a1.cpu(), a2.cpu())):
        assert_close(got1 / cnt, o1 / cnt, 1e-4, f"{name} N={N} stat sum ({what})")
        assert_close(got2 / cnt, o2 / cnt, 1e-4, f"{name} N={N} stat sumsq ({what})")
        assert_close(got1 / cnt, r1 / cnt, tol, f"{name} N={N} stat sum ({what}) against the reference",
                     scale=math.sqrt((r2 / cnt).max().item()))
        assert_close(got2 / cnt, r2 / cnt, tol, f"{name} N={N} stat sumsq ({what}) against the reference")
    return plans


def _run_pair(layer, n_a, n_b, dtype, seeds):
    """cy_conv3x3_wgrad_pair: two batches of one layer (own tensors, own BN coefficients) in one launch = the gradient
    over all their images"""
    from cyhip import ops
    name, H, C1, C2, Cout, mode, pro = layer
    wplan = cl.pair_plan(layer, n_a, n_b, dtype)
    segs, ref = [], torch.zeros(Cout, C1 + C2, 3, 3, dtype=torch.float64)
    for n, seed in ((n_a, seeds[0]), (n_b, seeds[1])):
        inp = _Inputs(n, layer, dtype, seed)
        assert len(inp.chunks) == 1
        x1, x2, dy = inp.chunk(0)
        g = torch.Generator().manual_seed(seed + 1)
        scale = shift = None
        if pro:
            scale = torch.rand(C1, generator=g) * 2 - 0.8
            shift = (torch.rand(C1, generator=g) * 2 - 1) * 0.3
        ref += _reference_chunk(_conv_input(x1, x2, mode, scale, shift, dtype), inp.w, dy)[2].double()
        segs.append((nhwc(x1, dtype), None if x2 is None else nhwc(x2, dtype), nhwc(dy, dtype),
                     None if scale is None else scale.to(DEV), None if shift is None else shift.to(DEV)))
    out = torch.zeros(Cout, C1 + C2, 3, 3, device=DEV)
    (a1, a2, ady, asc, ash), (b1, b2, bdy, bsc, bsh) = segs
    ops.conv3x3_wgrad_pair(a1, a2, ady, asc, ash, b1, b2, bdy, bsc, bsh, mode=mode, out=out)
    assert_close(out, ref, 2e-3, f"pair wgrad {name} {n_a}+{n_b} {wplan}")


# the parameter lists of the geometry cases, per workload: (layers, images per launch, layers of the paired weight
# gradient).  tests/test_plan_coverage.py derives from THESE lists which launch plans the cases below reach.
C2_LAYERS = cl.workload_layers("c2")
C2_BATCHES = list(cl.WORKLOADS["c2"]["batches"])
C2_PAIR_LAYERS = cl.workload_pair_layers("c2")
C4_LAYERS = cl.workload_layers("c4")
C4_BATCHES = list(cl.WORKLOADS["c4"]["batches"])
C4_PAIR_LAYERS = cl.workload_pair_layers("c4")
C5_LAYERS = cl.workload_layers("c5")
C5_BATCHES = list(cl.WORKLOADS["c5"]["batches"])
GEOMETRY_CASES = {"c2": (C2_LAYERS, C2_BATCHES, C2_PAIR_LAYERS), "c4": (C4_LAYERS, C4_BATCHES, C4_PAIR_LAYERS),
                  "c5": (C5_LAYERS, C5_BATCHES, [])}
# the kernel family a workload's layers run in (another answer of the planner is a failure of the case, not a skip)
C2_KERNELS = ("conv3x3_plane_kernel", "conv3x3_flow_kernel", "conv3x3_stream_kernel")
# c5, (forward, data gradient); layers not named: the flow kernel both ways
C5_KERNELS = {"Conv1b": ("conv3x3_stream_kernel", "conv3x3_stream_kernel"),
              "Conv2a": ("conv3x3_stream_kernel", "conv3x3_stream_kernel"),
              "Conv2b": ("conv3x3_flow_kernel", "conv3x3_stream_kernel")}


@pytest.mark.parametrize("N", C2_BATCHES)
@pytest.mark.parametrize("layer", C2_LAYERS, ids=[l[0] for l in C2_LAYERS])
def test_c2_layer_bf16(layer, N):
    plans = _run_layer(N, layer, BF, seed=1000 + N, expect_kernel=C2_KERNELS)
    # the claims of VERDICT r01 / ADVICE r01: these geometries reach split-K above 1, 512-channel operands and
    # (where the plane kernel is planned) the one-workgroup-per-CU build
    name = layer[0]
    if name == "Conv5b" and N == 16:
        assert plans["fwd"]["ksplit"] > 1, plans["fwd"]


@pytest.mark.parametrize("N", C4_BATCHES)
@pytest.mark.parametrize("layer", C4_LAYERS, ids=[l[0] for l in C4_LAYERS])
def test_c4_layer_fp16(layer, N):
    """the C4 benchmark's launches: 256 x 256, 16 / 32 images, fp16.  Widths are multiples of 16, not of 14: the igemm
    kernel where 32 output channels are written (256 x 256 level), the flow kernel with 16-column tiles elsewhere;
    the weight gradient wave-specialised with LDS-DMA loaders and patch-ordered k-steps, except 32 -> 64 channels (the
    2 x 1 wave layout has no specialised build) and the concat of two 32-channel sources (a 64-channel block would
    read both): wgrad12_kernel"""
    name, H, C1, C2, Cout, mode, pro = layer
    family = lambda co: "conv3x3_igemm_kernel" if co == 32 else "conv3x3_flow_kernel"  # noqa: E731
    unspecialised = (C1 + C2 == 32 and Cout == 64) or (C2 and C1 == 32)
    plans = _run_layer(N, layer, torch.float16, seed=4100 + N, expect_kernel=(family(Cout),),
                       expect_wgrad={"twelve": 1, "dma": 0} if unspecialised else {"twelve": 2, "dma": 1, "blk_order": 1})
    for k, p in plans.items():
        if k != "wgrad":
            assert p["kernel"] == family(Cout if k == "fwd" else C1 + C2), (name, k, p)
            assert p["kernel"] == "conv3x3_igemm_kernel" or p["tw"] == 16, (name, k, p)
    if name == "Conv5b":
        assert plans["fwd"]["ksplit"] > 1, plans["fwd"]
    if name == "Conv5a":
        assert plans["dgrad"]["ksplit"] > 1, plans["dgrad"]


@pytest.mark.parametrize("N", C5_BATCHES)
@pytest.mark.parametrize("layer", C5_LAYERS, ids=[l[0] for l in C5_LAYERS])
def test_c5_encoder_layer_bf16(layer, N):
    """the C5 benchmark's launches: the encoder at 512 images (256 slices x 2 views), bf16.  The streaming kernel on
    the 224 x 224 level, for Conv2a and for Conv2b's data gradient (C5_KERNELS); everything else in the flow kernel
    without split-K, below 112 x 112 in tiles of 32 rows of the N * H row space x 14 columns: on the 28- and 14-row
    images every tile holds rows of two or three images"""
    name, H, C1, C2, Cout, mode, pro = layer
    fwd_kernel, dgrad_kernel = C5_KERNELS.get(name, ("conv3x3_flow_kernel", "conv3x3_flow_kernel"))
    plans = _run_layer(N, layer, BF, seed=5000, expect_kernel=(fwd_kernel,),
                       expect_wgrad={"twelve": 1, "dma": 0} if name == "Conv2a" else {"twelve": 2, "dma": 1})
    assert plans["dgrad"]["kernel"] == dgrad_kernel, plans["dgrad"]
    for k in ("fwd", "dgrad"):
        if plans[k]["kernel"] == "conv3x3_flow_kernel":
            assert plans[k]["th"] == 32 and plans[k]["ksplit"] == 1, (k, plans[k])
            assert H > 56 or plans[k]["tw"] == 14, (k, plans[k])


def test_layer_above_the_2gib_limit_takes_the_64_bit_offset_kernels():
    """224 x 224, 32 -> 32 channels, bf16, at the first N whose tensors pass 2^31 - 1 bytes (669 images, 2.148 GB): the
    planners must leave the kernels with 32-bit buffer offsets (streaming kernel, LDS-DMA weight gradient) for the
    plane kernel and wgrad12_kernel, and those must address the whole tensor"""
    n = (2 ** 31 - 1) // (224 * 224 * 32 * 2) + 1
    layer = ("Conv1b", 224, 32, 0, 32, 0, 1)
    plans = _run_layer(n, layer, BF, seed=6000, expect_kernel=("conv3x3_plane_kernel",),
                       expect_wgrad={"twelve": 1, "dma": 0, "blk_order": 0})
    assert plans["dgrad"]["kernel"] == "conv3x3_plane_kernel", plans["dgrad"]


STREAM_LAYERS = [l for l in C2_LAYERS if l[0] in ("Conv1b", "Up2", "Up_conv2a", "Up_conv2b")]


@pytest.mark.parametrize("dtype", [BF, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("layer", STREAM_LAYERS, ids=lambda l: l[0])
def test_c2_low_channel_layers_take_the_streaming_kernel(layer, dtype):
    """the 224 x 224 level (Cin, Cout in {32, 64}) runs in the persistent LDS-DMA kernel (csrc/cy_conv_stream.h):
    forward with BN statistics (upsample / concat / BN+ReLU-prologue loads) and data gradient (incl. the split
    epilogue of the concat layer), both 16-bit storage types"""
    plans = _run_layer(16, layer, dtype, seed=555, expect_kernel=("conv3x3_stream_kernel",))
    assert plans["dgrad"]["kernel"] == "conv3x3_stream_kernel", plans["dgrad"]
    if layer[3]:
        assert plans["dgrad_split"]["kernel"] == "conv3x3_stream_kernel", plans["dgrad_split"]


@pytest.mark.parametrize("layer", [l for l in C2_LAYERS if l[0] in ("Conv1b", "Conv3a", "Conv4b", "Conv5b", "Up_conv5a", "Up4", "Up2")],
                         ids=lambda l: l[0])
def test_c2_layer_f32(layer):
    _run_layer(16, layer, torch.float32, seed=77)


@pytest.mark.parametrize("layer", C2_PAIR_LAYERS, ids=lambda l: l[0])
def test_c2_encoder_wgrad_pair(layer):
    """cy_conv3x3_wgrad_pair at the step's own sizes: the labeled pass's 16 images and the unlabeled pass's 32
    (own tensors, own BN coefficients) in one launch = the gradient over all 48"""
    n_a, n_b = cl.WORKLOADS["c2"]["pair"]
    _run_pair(layer, n_a, n_b, BF, (31, 32))


@pytest.mark.parametrize("layer", C4_PAIR_LAYERS, ids=lambda l: l[0])
def test_c4_encoder_wgrad_pair_fp16(layer):
    """the fp16 two-stage step pairs too (the library refuses two segments only for the four-wave f32 kernel): the
    unlabeled pass's 32 images parked, the labeled pass's 16 joining, 256 x 256"""
    n_a, n_b = cl.WORKLOADS["c4"]["pair"]
    _run_pair(layer, n_a, n_b, torch.float16, (41, 42))


C4_LAYERS_BF16 = cl.unet_layers(256, 512)


@pytest.mark.parametrize("layer", C4_LAYERS_BF16, ids=[l[0] for l in C4_LAYERS_BF16])
def test_c4_layer_bf16_igemm_path(layer):
    """BASELINE config 4 geometry: 256 x 256 inputs (widths 256..16: the igemm kernel), 4 images"""
    _run_layer(4, layer, BF, seed=4000, expect_kernel=("conv3x3_igemm_kernel", "conv3x3_flow_kernel"))


def test_full_size_c2_step_f32_matches_oracle():
    """one SemiSupervisedEpocher + InfoNCE step at the benchmark's own size (16 labeled + 16 unlabeled slices
    of 224 x 224, UNet(max_channel=512)) in f32 verification mode against oracle/step.py: losses and logits
    within 1e-4 (BASELINE.json north_star)"""
    from tests.step_harness import compare_step_with_oracle
    r = compare_step_with_oracle(n_l=16, n_unl=16, hw=224, max_channel=512, dtype=torch.float32, py_seed=3)
    assert r["rel_sup"] < 1e-4 and r["rel_reg"] < 1e-4 and r["rel_total"] < 1e-4, r
    assert r["rel_logits"] < 1e-4 and r["rel_logits_tf"] < 1e-4, r
    assert r["rel_running_mean"] < 1e-4, r
