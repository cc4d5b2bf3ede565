"""The patch-wise IIC kernels (csrc/cy_mi.hip), the PICA and JSD / entropy-prior kernels (csrc/cy_pica.hip), their
autograd functions and losses on the GPU, against tests/golden/patch_losses.npz (the reference in f32 and f64,
tests/golden/gen_goldens_patch_losses.py) and against float64 torch on the CPU (tests/patch_losses_cases.py).

Tolerance: max(4 * the reference's own largest f32-to-f64 distance of that kind over the fixture, 1e-6), read from the
npz; how each kind is measured is in tests/patch_losses_fixture.py.  No element is left out of any comparison, and every
figure is printed before it is asserted.  Outputs of the `ops` level are written into slices of buffers filled with a
guard value, which must be intact afterwards.
"""
import sys

import pytest
import torch

import patch_losses_cases as pc
import patch_losses_fixture as fx

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, PAD = 777.25, 8
EPS = sys.float_info.epsilon  # the patch loss's default


@pytest.fixture(scope="module")
def npz(golden_dir):
    return fx.load(golden_dir)


@pytest.fixture(scope="module")
def tol(npz):
    t = fx.tolerances(npz)
    print("tolerances", t)
    return t


@pytest.fixture(scope="module")
def patch_refs(npz):
    """tag -> the f64 CPU reference of a patch case, computed on first use and shared"""
    cache = {}

    def get(tag):
        if tag not in cache:
            n, k, H, W, patch, pad = fx.PATCH_CASES[tag]
            x1, x2 = fx.inputs(npz, tag)
            cache[tag] = pc.patch_reference(x1, x2, patch, pad, fx.LAMDA, EPS)
        return cache[tag]
    return get


class Guarded:
    """a float buffer filled with the guard value; `take(n)` gives a 16-byte aligned view of n floats with PAD guard
    floats on both sides; `intact()` checks everything outside the views handed out"""

    def __init__(self, total):
        self.buf = torch.full((total,), GUARD, device=DEV)
        self.mask = torch.ones(total, dtype=torch.bool, device=DEV)
        self.at = 0

    def take(self, n):
        start = self.at + PAD
        self.at = (start + n + PAD + 3) // 4 * 4
        assert self.at <= self.buf.numel()
        self.mask[start:start + n] = False
        return self.buf[start:start + n]

    def intact(self):
        return bool((self.buf[self.mask] == GUARD).all())


def gpu_leaf(t, fmt="nchw"):
    t = t.detach().to(DEV).clone()
    if fmt == "nhwc" and t.dim() == 4:
        t = t.contiguous(memory_format=torch.channels_last)
    return t.requires_grad_(True)


def nhwc(t):
    return t.to(DEV).permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------- 1. patch-wise IIC
@pytest.mark.parametrize("fmt", ["nchw", "nhwc"])
@pytest.mark.parametrize("tag", list(fx.PATCH_CASES) + [fx.MASK_CASE])
def test_patch_loss_against_the_goldens(npz, tol, tag, fmt):
    from contrastyou.losses.discreteMI import IIDSegmentationSmallPathLoss
    n, k, H, W, patch, pad = fx.PATCH_CASES[fx.MASK_OF if tag == fx.MASK_CASE else tag]
    a, b = (gpu_leaf(p, fmt) for p in fx.inputs(npz, tag))
    mask = torch.from_numpy(npz[f"{tag}_mask"]).float().to(DEV) if tag == fx.MASK_CASE else None
    before = (a.detach().clone(), b.detach().clone())
    crit = IIDSegmentationSmallPathLoss(lamda=fx.LAMDA, padding=pad, patch_size=patch)
    loss = crit(a, b, mask)
    loss.backward()
    assert torch.equal(a.detach(), before[0]) and torch.equal(b.detach(), before[1]), "the inputs were altered"
    pc.check_value(loss, npz[f"{tag}_loss64"], tol, f"{tag} {fmt} loss")
    pc.check_grad(a.grad, npz[f"{tag}_g1_64"], tol, f"{tag} {fmt} d x_out")
    pc.check_grad(b.grad, npz[f"{tag}_g2_64"], tol, f"{tag} {fmt} d x_tf_out")
    assert crit.get_joint_matrix().shape == (k, k)
    assert crit._patch_losses.shape[0] == len(pc.origins(H, patch)) * len(pc.origins(W, patch))


@pytest.mark.parametrize("tag", list(fx.PATCH_CASES))
def test_patch_ops_in_guarded_buffers(npz, tol, patch_refs, tag):
    from cyhip import ops
    n, k, H, W, patch, pad = fx.PATCH_CASES[tag]
    ref = patch_refs(tag)
    x1, x2 = (nhwc(p) for p in fx.inputs(npz, tag))
    P, TT = ref["J"].shape[0], ref["J"].shape[1]
    nj = P * TT * k * k
    mem = Guarded(3 * nj + 1 + P + 2 * x1.numel() + 7 * (2 * PAD + 4))
    J = ops.joint_patch_fwd(x1, x2, pad, patch, pad == 0, J=mem.take(nj))
    out = (mem.take(1), mem.take(P), mem.take(nj).view(P, TT, k, k), mem.take(nj).view(P, TT, k, k))
    loss, losses, Pj, dJ = ops.iid_patch_loss(J, 0 if pad == 0 else 1, fx.LAMDA, EPS, out=out)
    g = torch.tensor([0.75], device=DEV)
    d1, d2 = ops.joint_patch_bwd(x1, x2, dJ, g, pad, patch, pad == 0, d1=mem.take(x1.numel()).view_as(x1),
                                 d2=mem.take(x1.numel()).view_as(x1))
    torch.cuda.synchronize()
    assert mem.intact(), "a guard value next to an output was overwritten"
    for q in range(P):
        pc.check_value(J[q], ref["J"][q], tol, f"{tag} J of patch {q}")
    pc.check_grad(J, ref["J"], tol, f"{tag} J")
    pc.check_value(losses, ref["losses"], tol, f"{tag} patch losses")
    pc.check_value(loss[0], ref["loss"], tol, f"{tag} mean loss")
    pc.check_value(loss[0], npz[f"{tag}_loss64"], tol, f"{tag} mean loss vs npz")
    pc.check_grad(Pj, ref["P"], tol, f"{tag} final joints")
    pc.check_grad(dJ, ref["dJ"], tol, f"{tag} dJ")
    pc.check_grad(d1.permute(0, 3, 1, 2), 0.75 * ref["g1"], tol, f"{tag} dx1")
    pc.check_grad(d2.permute(0, 3, 1, 2), 0.75 * ref["g2"], tol, f"{tag} dx2")
    # a null dx is skipped
    only2 = ops.joint_patch_bwd(x1, x2, dJ, g, pad, patch, pad == 0, need1=False)
    assert only2[0] is None and torch.equal(only2[1], d2)


@pytest.mark.parametrize("tag", ["B", "E", "C"])
def test_two_runs_are_bit_identical(npz, tag):
    from contrastyou.losses.discreteMI import IIDSegmentationSmallPathLoss
    n, k, H, W, patch, pad = fx.PATCH_CASES[tag]
    runs = []
    for _ in range(2):
        a, b = (gpu_leaf(p) for p in fx.inputs(npz, tag))
        crit = IIDSegmentationSmallPathLoss(lamda=fx.LAMDA, padding=pad, patch_size=patch)
        loss = crit(a, b)
        loss.backward()
        runs.append((loss.detach(), a.grad, b.grad, crit._patch_losses, crit._p_i_j))
    for u, v in zip(*runs):
        assert torch.equal(u, v)


def test_one_clipped_patch_is_the_single_map_loss(npz, tol):
    """case D: the map is smaller than the patch, so the patch-wise loss is IIDSegmentationLoss on the whole map: the
    same staging, the same summation order and the same loss body -- the same bits"""
    from contrastyou.losses.discreteMI import IIDSegmentationLoss, IIDSegmentationSmallPathLoss
    n, k, H, W, patch, pad = fx.PATCH_CASES["D"]
    got = []
    for crit in (IIDSegmentationSmallPathLoss(lamda=fx.LAMDA, padding=pad, patch_size=patch),
                 IIDSegmentationLoss(lamda=fx.LAMDA, padding=pad, symmetric=False, eps=EPS)):
        a, b = (gpu_leaf(p) for p in fx.inputs(npz, "D"))
        loss = crit(a, b)
        loss.backward()
        got.append((loss.detach(), a.grad, b.grad, torch.from_numpy(crit.get_joint_matrix())))
    for name, u, v in zip(("loss", "d x_out", "d x_tf_out", "joint"), *got):
        print(name, "max |difference|", float((u.double() - v.double()).abs().max()))
        assert torch.equal(u, v), name


# (shape, k, pad, normalise, forward kernel of both sides)
WHOLE_IMAGE_CASES = (
    [((1, 33, 37), k, 0, norm, "per_displacement") for k in (5, 20) for norm in (True, False)]
    + [((1, 8, 64), 64, 1, False, "per_displacement")]
    + [((1, 6, 40), k, 1, False, "staged") for k in (8, 21)])  # one row tile: one block per displacement group


@pytest.mark.parametrize("shape,k,pad,normalise,kernel", WHOLE_IMAGE_CASES,
                         ids=[f"{n}x{h}x{w}-k{k}-pad{p}-{'norm' if nm else 'raw'}-{kn}"
                              for (n, h, w), k, p, nm, kn in WHOLE_IMAGE_CASES])
def test_whole_image_joint_is_the_one_patch_joint(shape, k, pad, normalise, kernel):
    """a whole image is the window of origin (0, 0) and extent H x W: with one patch that covers the map, the patch-wise
    kernel and the whole-image kernel run the same body on the same window -- the same bits, given the same forward
    kernel, rows per tile and block count along x (asserted first, from the two plan queries)"""
    from cyhip import ops
    N, H, W = shape
    patch = max(H, W)
    whole = ops.joint_plan(N, H, W, k, pad)
    one = ops.joint_patch_plan(N, H, W, k, pad, patch, kernel)
    print("whole", whole, "\none patch", one)
    assert one["P"] == 1 and (one["eh"], one["ew"]) == (H, W)
    assert whole["fwd_kernel"] == one["fwd_kernel"] == ops.JOINT_PATCH_KERNELS[kernel]
    assert whole["R"] == one["R"]
    assert whole["nblk"] == one["nbx"]
    g = torch.Generator().manual_seed(11)
    x1, x2 = (nhwc(torch.softmax(torch.randn(N, k, H, W, generator=g) * 2, 1)) for _ in range(2))
    J = ops.joint_fwd(x1, x2, N, H, W, k, pad, normalise)
    Jp = ops.joint_patch_fwd(x1, x2, pad, patch, normalise, kernel=kernel)
    print("max |difference|", float((J.double() - Jp[0].double()).abs().max()))
    assert J.shape == Jp[0].shape and torch.equal(J, Jp[0])


@pytest.mark.parametrize("tag", ["A", "B", "C", "E"])
def test_the_fallback_forward_agrees_with_the_staged_one(npz, tol, patch_refs, tag):
    """the per-displacement kernel, which the rule takes where the staged tile exceeds the LDS cap, forced through the
    plan override `kernel`"""
    from cyhip import ops
    n, k, H, W, patch, pad = fx.PATCH_CASES[tag]
    assert ops.joint_patch_plan(n, H, W, k, pad, patch)["fwd_kernel"] == 1
    assert ops.joint_patch_plan(n, H, W, k, pad, patch, "per_displacement")["fwd_kernel"] == 0
    x1, x2 = (nhwc(p) for p in fx.inputs(npz, tag))
    staged = ops.joint_patch_fwd(x1, x2, pad, patch, pad == 0, kernel="staged")
    single = ops.joint_patch_fwd(x1, x2, pad, patch, pad == 0, kernel="per_displacement")
    ref = patch_refs(tag)["J"]
    pc.check_grad(single, ref, tol, f"{tag} per-displacement J")
    pc.check_grad(single, staged.cpu(), tol, f"{tag} per-displacement vs staged")
    for q in range(ref.shape[0]):
        pc.check_value(single[q], ref[q], tol, f"{tag} per-displacement J of patch {q}")


def test_a_block_that_walks_several_tiles(tol):
    from cyhip import ops
    n, k, H, W, patch, pad = pc.MULTI_TRIP
    plan = ops.joint_patch_plan(n, H, W, k, pad, patch)
    assert plan["fwd_kernel"] == 1 and 1 < plan["nbx"] < plan["ntile"], plan
    g = torch.Generator().manual_seed(5)
    x1, x2 = (torch.softmax(torch.randn(n, k, H, W, generator=g) * 2, 1) for _ in range(2))
    J = ops.joint_patch_fwd(nhwc(x1), nhwc(x2), pad, patch, False)
    ref = pc.patch_joints64(x1, x2, patch, pad)
    pc.check_grad(J, ref, tol, "multi-trip J")
    for q in range(ref.shape[0]):
        pc.check_value(J[q], ref[q], tol, f"multi-trip J of patch {q}")


# ---------------------------------------------------------------------------------------------- 2. PICA
def _run(crit, ps, fmt="nchw"):
    xs = [gpu_leaf(p, fmt) for p in ps]
    v = crit(*xs)
    (v if v.dim() == 0 else (v * fx.none_weights(v)).sum()).backward()
    return v.detach(), [x.grad for x in xs]


def _check(npz, tol, tag, v, grads, ref):
    """against the npz (the reference in f64) and against the f64 formula of patch_losses_cases"""
    pc.check_value(v, npz[f"{tag}_loss64"], tol, f"{tag} value vs npz")
    pc.check_value(v, ref[0], tol, f"{tag} value vs f64")
    for i, g in enumerate(grads, 1):
        assert g.shape == ref[1][i - 1].shape
        pc.check_grad(g, npz[f"{tag}_g{i}_64"], tol, f"{tag} d input {i} vs npz")
        pc.check_grad(g, ref[1][i - 1], tol, f"{tag} d input {i} vs f64")


@pytest.mark.parametrize("fmt", ["nchw", "nhwc"])
@pytest.mark.parametrize("tag", list(fx.PUISEG_CASES))
def test_puiseg_loss(npz, tol, tag, fmt):
    from contrastyou.losses.pica_loss import PUISegLoss
    shape, pad = fx.PUISEG_CASES[tag]
    ps = fx.inputs(npz, tag)
    ref = pc.reference(lambda xs: pc.puiseg64(xs[0], xs[1], fx.PUI_LAMDA, pad), ps)
    v, grads = _run(PUISegLoss(lamda=fx.PUI_LAMDA, padding=pad), ps, fmt)
    _check(npz, tol, tag, v, grads, ref)
    again = _run(PUISegLoss(lamda=fx.PUI_LAMDA, padding=pad), ps, fmt)
    assert torch.equal(v, again[0]) and all(torch.equal(a, b) for a, b in zip(grads, again[1]))


@pytest.mark.parametrize("tag", list(fx.PUI_CASES))
def test_pui_loss(npz, tol, tag):
    from contrastyou.losses.pica_loss import PUILoss
    ps = fx.inputs(npz, tag)
    ref = pc.reference(lambda xs: pc.pui64(xs[0], xs[1], fx.PUI_LAMDA), ps)
    v, grads = _run(PUILoss(lamda=fx.PUI_LAMDA), ps)
    _check(npz, tol, tag, v, grads, ref)
    again = _run(PUILoss(lamda=fx.PUI_LAMDA), ps)
    assert torch.equal(v, again[0]) and all(torch.equal(a, b) for a, b in zip(grads, again[1]))


# ---------------------------------------------------------------------------------------------- 3. JSD, entropy prior
@pytest.mark.parametrize("tag,fmt", [(t, f) for t, c in fx.JSD_CASES.items() for f in ("nchw", "nhwc")
                                     if len(c[1]) == 4 or f == "nchw"])  # rows have one memory format
def test_jsd_div(npz, tol, tag, fmt):
    from contrastyou.losses.kl import JSD_div
    m, shape, red = fx.JSD_CASES[tag]
    ps = fx.inputs(npz, tag, m)
    ref = pc.reference(lambda xs: pc.jsd64(xs, red, fx.EPS), ps)
    v, grads = _run(JSD_div(reduction=red, eps=fx.EPS), ps, fmt)
    assert v.shape == ref[0].shape
    _check(npz, tol, tag, v, grads, ref)
    again = _run(JSD_div(reduction=red, eps=fx.EPS), ps, fmt)
    assert torch.equal(v, again[0]) and all(torch.equal(a, b) for a, b in zip(grads, again[1]))


def test_jsd_div_mixed_memory_formats_and_limits(npz, tol):
    from contrastyou.losses.kl import JSD_div
    tag = "jsd3_mean"
    ps = fx.inputs(npz, tag, 3)
    xs = [gpu_leaf(ps[0], "nhwc"), gpu_leaf(ps[1], "nchw"), gpu_leaf(ps[2], "nhwc").detach()]
    v = JSD_div()(*xs)
    v.backward()
    pc.check_value(v, npz[f"{tag}_loss64"], tol, "mixed formats value")
    pc.check_grad(xs[0].grad, npz[f"{tag}_g1_64"], tol, "mixed formats d input 1")
    pc.check_grad(xs[1].grad, npz[f"{tag}_g2_64"], tol, "mixed formats d input 2")
    one = xs[0].detach()
    for bad in ((one,), (one,) * 9, (one.double(), one.double()), (torch.rand(2, 65, 3, 3, device=DEV),) * 2):
        with pytest.raises(NotImplementedError, match="2 to 8 float32 maps of up to 64 classes"):
            JSD_div()(*bad)


@pytest.mark.parametrize("tag", list(fx.PRIOR_CASES))
def test_entropy_prior(npz, tol, tag):
    from contrastyou.losses.kl import EntropyPrior
    shape, given = fx.PRIOR_CASES[tag]
    ps = fx.inputs(npz, tag, 1)
    prior = torch.from_numpy(npz[f"{tag}_prior"]) if given else None
    ref = pc.reference(lambda xs: pc.prior64(xs[0], None if prior is None else prior.double(), fx.EPS), ps)
    crit = EntropyPrior(eps=fx.EPS)
    v, grads = _run(lambda x: crit(x, None if prior is None else prior.to(DEV)), ps)
    _check(npz, tol, tag, v, grads, ref)
    with pytest.raises(AssertionError):
        crit(torch.rand(2, 6, 3, 3, device=DEV).softmax(1))
    with pytest.raises(AssertionError):
        EntropyPrior(reduction="sum")
