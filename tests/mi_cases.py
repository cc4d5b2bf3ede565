"""The cases tests/test_gpu_mi_dispatch.py is parametrised with, and what tests/test_mi_plan_coverage.py requires of
them: the information-loss kernels of csrc/cy_mi.hip (grouped softmax, joints, displaced joints, joint backward, the
one-block loss).  A plain module (no GPU, no library call at import): the GPU tests and the CPU guard read the launch
plan of a case through the same host-side queries, cyhip.ops.joint_plan / group_softmax_plan.

Shapes are (N, H, W); vectors are (n, 1, 1).  Every shape is the smallest that reaches its branch; BIG is the one large
case (2.1 M pixels, k = 4): the forward's cap of 2048 partial blocks and the backward's second trip past 8192 blocks."""
from collections import namedtuple

# raw joint: ops.joint_fwd against a float64 einsum / conv2d.  masked: whole pixels of both maps zero
JointCase = namedtuple("JointCase", "shape k pad masked note")
# adjoint: ops.joint_bwd with a random dJ.  need: "1", "2" or "12" (which inputs ask for a gradient)
BwdCase = namedtuple("BwdCase", "shape k pad need normalise gscale note")
# ops.iid_loss on a given joint.  kind: "rand", "zeros" (two classes that never co-occur), "min_later" (mode 1: the
# global minimum sits in the last displacement).  lamda and want_grad are looped over inside the test.
LossCase = namedtuple("LossCase", "TT k mode symmetric kind")
# ops.group_softmax_fwd / _bwd.  Logits are offset +-80 per row (LOGIT_OFFSET), so the max-subtraction matters
SoftmaxCase = namedtuple("SoftmaxCase", "M S k T")
# IIDFn end to end on softmax inputs: loss, P and both input gradients against oracle/next_rows.py
IIDCase = namedtuple("IIDCase", "shape k mode pad symmetric lamda note")

VEC37 = (37, 1, 1)       # less than one 64-pixel tile
TWO_BLOCKS = (1, 33, 37)  # 1221 pixels: two blocks of 640, the second ends in a 5-pixel tile
REDUCE65 = (1, 260, 256)  # 66 560 pixels: 65 partial blocks, one more than the 64 slices of the reduction
BIG = (3, 840, 840)      # 2 116 800 pixels
DISP = (2, 9, 11)        # one row tile per image: a block walks two tiles
ROWTAIL = (2, 10, 40)    # R = 6: two row tiles per image, the second has 4 rows
WIDE = (1, 3, 260)       # W > 256: one row per tile
LDS150 = (1, 8, 64)      # k >= 61: the staged rows exceed 150 KB, one launch row per displacement

K_EDGES = (1, 4, 5, 12, 20, 33, 61, 64)  # 256 slices | scalar staging | idle threads | ... | one slice

JOINT_CASES = (
    [JointCase(TWO_BLOCKS, k, 0, False, "tile") for k in K_EDGES]
    + [JointCase(VEC37, 20, 0, False, "tile, 16-byte staging, lim tail inside the only tile"),
       JointCase(VEC37, 5, 0, False, "tile, scalar staging"),
       JointCase(TWO_BLOCKS, 20, 0, True, "masked map"),
       JointCase(REDUCE65, 8, 0, False, "reduce past 64 blocks"),
       JointCase(BIG, 4, 0, False, "nblk at its cap")]
    + [JointCase(DISP, 8, pad, False, "multi, 16-byte staging") for pad in (1, 2, 3)]  # nd of the last group 9, 7, 4
    + [JointCase(ROWTAIL, 20, 1, False, "multi, tiles_h = 2, 4-row tail"),
       JointCase(ROWTAIL, 21, 1, False, "multi, scalar staging, 4-row tail"),
       JointCase(ROWTAIL, 20, 1, True, "multi, masked map"),
       JointCase(WIDE, 4, 1, False, "multi, W > 256"),
       JointCase(DISP, 4, 1, False, "multi, nsl > W"),
       JointCase((1, 9, 11), 12, 2, False, "multi, idle threads"),
       JointCase(LDS150, 64, 1, False, "fallback"),
       JointCase(LDS150, 61, 1, False, "fallback, scalar k"),
       JointCase(LDS150, 64, 2, False, "fallback, grid_y = 25")])

BWD_CASES = (
    [BwdCase(DISP, k, pad, "12", pad == 0, 1.0, "vec4" if k % 4 == 0 else "scalar") for k in (8, 5) for pad in (0, 1, 2)]
    + [BwdCase(DISP, 8, 1, "1", False, 0.37, "need1 only, gscale"),
       BwdCase(DISP, 5, 1, "2", False, -2.5, "need2 only, gscale"),
       BwdCase(DISP, 8, 0, "12", False, 1.0, "pad 0 without normalise"),
       BwdCase(DISP, 5, 2, "12", True, 1.0, "pad 2 with normalise"),
       BwdCase(LDS150, 64, 0, "12", True, 1.0, "k = 64: the largest dJ of one displacement"),
       BwdCase(LDS150, 64, 1, "12", False, 1.0, "refused before ABI 17: chunks of 4, 4, 1 displacements"),
       BwdCase(LDS150, 32, 2, "12", False, 1.0, "refused before ABI 17: chunks of 16, 9"),
       BwdCase((1, 5, 7), 33, 2, "12", False, 0.5, "refused before ABI 17: scalar kernel, chunks of 15, 10"),
       BwdCase(BIG, 4, 0, "12", True, 1.0, "second trip past 8192 blocks")])

LOSS_CASES = (
    [LossCase(1, k, mode, sym, "rand") for k in (1, 20) for mode in (0, 2) for sym in (False, True)]
    + [LossCase(TT, k, 1, sym, "rand") for TT, k in ((9, 20), (25, 12), (9, 64), (25, 64)) for sym in (False, True)]
    + [LossCase(1, 20, 0, False, "zeros"), LossCase(1, 20, 2, True, "zeros"), LossCase(9, 20, 1, True, "zeros"),
       LossCase(9, 20, 1, False, "min_later"), LossCase(25, 12, 1, True, "min_later")])
LAMDAS = (1.0, 1.5)

LOGIT_OFFSET = 80.0
SK_ALL = ((1, 1), (1, 2), (3, 6), (5, 20), (10, 20), (1, 255), (1, 127), (1, 128))
M_ALL = (1, 63, 64, 65, 1000)
SOFTMAX_CASES = (
    [SoftmaxCase(65, S, k, T) for S, k in SK_ALL for T in (1.0, 0.1)]
    # every M at one shape with 64 rows per backward block, and at two with 32 (the widened backward, S*k > 127)
    + [SoftmaxCase(M, S, k, 1.0) for S, k in ((3, 6), (10, 20), (1, 255)) for M in M_ALL if M != 65])
SOFTMAX_REFUSED = ((1, 256), (16, 16), (13, 20))  # S*k > 255: both directions, before any launch

IID_CASES = [
    IIDCase(TWO_BLOCKS, 20, 0, 0, False, 1.5, "tile kernel, segmentation loss"),
    IIDCase(VEC37, 20, 2, 0, True, 1.5, "tile kernel, vectors"),
    IIDCase(ROWTAIL, 20, 1, 1, True, 1.0, "multi kernel"),
    IIDCase(LDS150, 64, 1, 1, False, 1.0, "fallback; chunked backward"),
]


def npix(shape):
    n, h, w = shape
    return n * h * w


def case_id(c):
    n, h, w = c.shape if hasattr(c, "shape") else (0, 0, 0)
    if isinstance(c, JointCase):
        return f"k{c.k}-pad{c.pad}-{n}x{h}x{w}" + ("-masked" if c.masked else "")
    if isinstance(c, BwdCase):
        return f"k{c.k}-pad{c.pad}-{n}x{h}x{w}-need{c.need}-{'norm' if c.normalise else 'raw'}-g{c.gscale}"
    if isinstance(c, LossCase):
        return f"TT{c.TT}-k{c.k}-mode{c.mode}-{'sym' if c.symmetric else 'asym'}-{c.kind}"
    if isinstance(c, SoftmaxCase):
        return f"M{c.M}-S{c.S}-k{c.k}-T{c.T}"
    return f"k{c.k}-mode{c.mode}-pad{c.pad}-{n}x{h}x{w}"


def plan(c):
    from cyhip import ops
    return ops.joint_plan(*c.shape, c.k, c.pad)


def softmax_plan(c):
    from cyhip import ops
    return ops.group_softmax_plan(c.M, c.S, c.k)


def sentinel_pixels(shape, p):
    """flat pixel indices (n, h, w order) where the forward kernels change what they do: the ends, the block and tile
    boundaries of the plan `p`, the image corners and one pixel of every border row and column"""
    N, H, W = shape
    n = N * H * W
    s = {0, n - 1}
    flat = lambda i, h, w: (i * H + h) * W + w  # noqa: E731
    for i in {0, N - 1}:
        s |= {flat(i, 0, 0), flat(i, 0, W - 1), flat(i, H - 1, 0), flat(i, H - 1, W - 1)}            # corners
        s |= {flat(i, 0, W // 2), flat(i, H - 1, W // 2), flat(i, H // 2, 0), flat(i, H // 2, W - 1)}  # borders
        if p["fwd_kernel"] == 1 and p["tiles_h"] > 1:
            h0 = (p["tiles_h"] - 1) * p["R"]  # the tail tile's first row; the row tile before it ends at h0 - 1
            s |= {flat(i, p["R"] - 1, W - 1), flat(i, p["R"], 0), flat(i, h0 - 1, W - 1), flat(i, h0, 0)}
    if p["fwd_kernel"] == 0:
        for b in {1, (n - 1) // p["per"]} - {0}:  # the first block boundary and the last one before a block with pixels
            if b * p["per"] < n:
                s |= {b * p["per"] - 1, b * p["per"]}
        s |= {(n - 1) // 64 * 64, max((n - 1) // 64 * 64 - 1, 0)}  # the first pixel of the tail tile, and the one before
    assert all(0 <= q < n for q in s)
    return sorted(s)


# ---------------------------------------------------------------- float64 references (torch on the CPU)
def disp(d, pad):
    """displacement (du, dv) of joint d: J[d][i][j] = sum_q x1[q + (du, dv)][i] * x2[q][j]"""
    T = 2 * pad + 1
    return d // T - pad, d % T - pad


def raw_joint(x1, x2, pad):
    """x1, x2 [N,H,W,k] float64 -> [T*T, k, k] unnormalised joint, zero outside the image.  pad 0: an einsum over the
    pixels; pad > 0: the F.conv2d of compute_joint_2D (losses/discreteMI.py:225-243) with x1 as input, x2 as weight."""
    import torch
    import torch.nn.functional as F
    k = x1.shape[-1]
    if pad == 0:
        return torch.einsum("nhwi,nhwj->ij", x1, x2).view(1, k, k)
    T = 2 * pad + 1
    p = F.conv2d(x1.permute(3, 0, 1, 2), x2.permute(3, 0, 1, 2), padding=(pad, pad))  # [k1, k2, T, T]
    return p.permute(2, 3, 0, 1).reshape(T * T, k, k)


def loss_from_joint(J, mode, symmetric, lamda, eps):
    """the information loss as a function of the raw joint J [TT,k,k] (float64, differentiable): (loss, joint P).
    mode 0: IIDSegmentationLoss padding 0 (J already divided by the pixel count, losses/discreteMI.py:246-261);
    mode 1: padding > 0 (:225-243, :127-170); mode 2: IIDLoss on vectors (:90-124, :201-222)."""
    import torch
    TT = J.shape[0]
    p = J
    if mode == 1:
        p = p - p.min().detach() + 1e-8
        p = p / p.sum(dim=(1, 2), keepdim=True)
    if symmetric:
        p = (p + p.transpose(1, 2)) / 2.0
    if mode != 0:
        p = p / p.sum()
    pi = p.sum(dim=2, keepdim=True)
    pj = p.sum(dim=1, keepdim=True)
    loss = (-p * (torch.log(p + eps) - lamda * torch.log(pi + eps) - lamda * torch.log(pj + eps))).sum()
    return (loss / TT if mode == 1 else loss), p
