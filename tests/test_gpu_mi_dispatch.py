"""Parity of the information-loss kernels (csrc/cy_mi.hip) on every branch of their dispatch: grouped softmax, the
k x k joint of two maps, the displaced joints, the joint backward and the one-block loss.  The cases are those of
tests/mi_cases.py; tests/test_mi_plan_coverage.py checks on the CPU, from the launch plan, that they reach every branch.

Reference: torch on the CPU in float64, with autograd, on the same float32 inputs; nothing a kernel computed feeds it.
Three layers, each called through cyhip.ops so that a fault in one kernel is not hidden by the next: the raw joint
(an einsum, or the F.conv2d of compute_joint_2D), the loss on a given joint (mi_cases.loss_from_joint, which
test_mi_plan_coverage.py ties to oracle/next_rows.py), the adjoint of the joint with a random dJ; then IIDFn end to end
against oracle/next_rows.py.  Tolerances, on max|got - ref| <= tol * max|ref|: joints and probabilities 1e-5, loss
scalars 2e-5 * max(1, |ref|), input gradients and dJ 5e-4, grouped-softmax gradients 1e-4.

Sentinels of the forward: class k-1 of x1 and class 0 of x2 are zero except at the sentinel pixels of
mi_cases.sentinel_pixels (ends, block and tile boundaries from the plan, corners, borders), so row k-1 and column 0 of
every J[d] are sums of a few single products: they are compared against their own maximum, and before the GPU result is
read each sentinel's own contribution must be at least 10 x the tolerance of its row.

Every launch runs twice and must be bit-equal; the second run goes through the C entry point into buffers filled with
NaN, so an element no thread wrote cannot pass on what the allocator left there."""
import functools
import math

import pytest
import torch

from tests import mi_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_P, TOL_LOSS, TOL_G, TOL_SM_G = 1e-5, 2e-5, 5e-4, 1e-4


def _ops():
    from cyhip import ops
    return ops


def check(got, ref, tol, what, scale=None):
    got = got.detach().cpu().double().reshape(ref.shape)
    scale = ref.abs().max().item() if scale is None else scale
    err = (got - ref).abs().max().item() if ref.numel() else 0.0
    print(f"{what}: err {err:.3e}, tol {tol:.0e} * {scale:.3e}")
    assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol:.0e} * {scale:.3e}"  # (NaN fails: not <=)
    return err


def check_loss(got, ref, what):
    return check(got, ref.detach().reshape(()), TOL_LOSS, what, scale=max(1.0, abs(ref.item())))


def nan_like(t):
    return torch.full_like(t, float("nan"))


def rnd32(*shape, gen):
    return torch.rand(*shape, generator=gen, dtype=torch.float32) * 2 - 1


# ---------------------------------------------------------------- layer 1: the raw joint
def joint_fwd_raw(x1, x2, shape, k, pad, normalise):
    """ops.joint_fwd into a J filled with NaN"""
    ops = _ops()
    TT = (2 * pad + 1) ** 2
    J = torch.full((TT, k, k), float("nan"), device=x1.device, dtype=torch.float32)
    nbytes = ops.joint_plan(*shape, k, pad)["ws_bytes"]
    ws = ops._ws(nbytes, x1.device)
    ops._lib.call("cy_joint_fwd", x1.data_ptr(), x2.data_ptr(), J.data_ptr(), *shape, k, pad, int(normalise),
                  ws.data_ptr(), nbytes, ops._stream())
    return J


@functools.lru_cache(maxsize=1)
def joint_problem(case):
    """float32 inputs [npix, k] with their sentinel classes, the float64 raw joint, and the contribution of every
    sentinel to row k-1 (x1's sentinel class) and to column 0 (x2's)"""
    N, H, W = case.shape
    k, pad, n = case.k, case.pad, mc.npix(case.shape)
    gen = torch.Generator().manual_seed(100 * n + 10 * k + pad)
    x1, x2 = rnd32(n, k, gen=gen), rnd32(n, k, gen=gen)
    sent = mc.sentinel_pixels(case.shape, mc.plan(case)) if k > 1 else []
    if case.masked:  # IIDSegmentationLoss(mask=...): whole pixels of both maps zero (the sentinels stay)
        keep = torch.rand(n, generator=gen) > 0.3
        keep[sent] = True
        x1, x2 = x1 * keep[:, None], x2 * keep[:, None]
    if k > 1:
        x1[:, k - 1], x2[:, 0] = 0.0, 0.0
        vals = 1.0 + (torch.arange(len(sent)) % 8).float() / 8
        x1[sent, k - 1], x2[sent, 0] = vals, vals.flip(0)
    a, b = x1.double().view(N, H, W, k), x2.double().view(N, H, W, k)
    ref = mc.raw_joint(a, b, pad)
    TT = ref.shape[0]
    rows, cols = torch.zeros(len(sent), TT, k, dtype=torch.float64), torch.zeros(len(sent), TT, k, dtype=torch.float64)
    for i, q in enumerate(sent):
        img, h, w = q // (H * W), q // W % H, q % W
        for d in range(TT):
            du, dv = mc.disp(d, pad)
            if 0 <= h - du < H and 0 <= w - dv < W:  # x1's sentinel at q meets x2 at q - disp(d)
                rows[i, d] = a[img, h, w, k - 1] * b[img, h - du, w - dv]
            if 0 <= h + du < H and 0 <= w + dv < W:  # x2's sentinel at q meets x1 at q + disp(d)
                cols[i, d] = a[img, h + du, w + dv] * b[img, h, w, 0]
    return x1, x2, ref, sent, rows, cols


@pytest.mark.parametrize("case", mc.JOINT_CASES, ids=mc.case_id)
def test_joint_forward(case):
    """Worst error over the cases, relative to max|ref| (MI355X): joint 1.1e-6, sentinel row 3.0e-8, sentinel column
    4.1e-8.  The 2.1 M-pixel sum (k4-pad0-3x840x840) meets 1e-5 like the others (a float32 CPU einsum of the same sum is
    2.8e-7 off), so no case uses a float32-summation allowance."""
    ops = _ops()
    x1, x2, ref, sent, rows, cols = joint_problem(case)
    k, pad, n = case.k, case.pad, mc.npix(case.shape)
    if k > 1:  # visibility, before the GPU is looked at: losing one sentinel moves its row / column by >= 10 x tol
        row_ref, col_ref = ref[:, k - 1, :], ref[:, :, 0]
        assert (rows.sum(0) - row_ref).abs().max() <= 1e-12 * row_ref.abs().max()
        assert (cols.sum(0) - col_ref).abs().max() <= 1e-12 * col_ref.abs().max()
        assert len(sent) >= 2
        for i, q in enumerate(sent):
            assert rows[i].abs().max() >= 10 * TOL_P * row_ref.abs().max(), (q, "row")
            assert cols[i].abs().max() >= 10 * TOL_P * col_ref.abs().max(), (q, "column")
    g1, g2 = x1.to(DEV), x2.to(DEV)
    J = ops.joint_fwd(g1, g2, *case.shape, k, pad, False)
    again = joint_fwd_raw(g1, g2, case.shape, k, pad, False)
    assert torch.equal(J, again), "two runs differ"
    check(J, ref, TOL_P, "joint")
    if k > 1:
        check(J[:, k - 1, :], ref[:, k - 1, :], TOL_P, "sentinel row of x1")
        check(J[:, :, 0], ref[:, :, 0], TOL_P, "sentinel column of x2")
    if pad == 0:  # the normalised form of compute_joint_2D_with_padding_zeros
        check(ops.joint_fwd(g1, g2, *case.shape, k, 0, True), ref / n, TOL_P, "joint / npix")


# ---------------------------------------------------------------- layer 2: the loss on a given joint
def loss_joint(case):
    TT, k = case.TT, case.k
    gen = torch.Generator().manual_seed(1000 * TT + 10 * k + case.mode)
    J = torch.rand(TT, k, k, generator=gen, dtype=torch.float32) + 0.05
    if case.mode == 1:  # displaced co-occurrence sums: a different scale per displacement
        J = J * (1.0 + torch.arange(TT).float().view(TT, 1, 1)) * 10
    elif case.mode == 2:
        J = J * 37
    else:
        J = J / J.sum()
    if case.kind == "zeros":  # two classes that never co-occur
        J[:, 2, 5], J[:, 5, 2] = 0.0, 0.0
    if case.kind == "min_later":
        J[TT - 1, 1, 2] = J.min() / 4
        assert J.view(TT, -1).min(1).values.argmin().item() == TT - 1
    return J


@pytest.mark.parametrize("case", mc.LOSS_CASES, ids=mc.case_id)
def test_loss_on_a_given_joint(case):
    ops = _ops()
    J = loss_joint(case)
    eps = 1e-10 if case.mode == 2 else 1e-5
    Jg = J.to(DEV)
    for lamda in mc.LAMDAS:
        Jd = J.double().requires_grad_(True)
        loss, P = mc.loss_from_joint(Jd, case.mode, case.symmetric, lamda, eps)
        loss.backward()
        loss1, _ = mc.loss_from_joint(J.double(), case.mode, case.symmetric, 1.0, eps)
        out2, Pg, dJ = ops.iid_loss(Jg, case.mode, case.symmetric, lamda, eps, want_grad=True)
        out2b, Pb, dJb = ops.iid_loss(Jg, case.mode, case.symmetric, lamda, eps, want_grad=True)
        assert torch.equal(out2, out2b) and torch.equal(Pg, Pb) and torch.equal(dJ, dJb), "two runs differ"
        out2n, Pn, none = ops.iid_loss(Jg, case.mode, case.symmetric, lamda, eps, want_grad=False)
        assert none is None and torch.equal(out2, out2n) and torch.equal(Pg, Pn), "want_grad changes the forward"
        tag = f"lamda {lamda}"
        check_loss(out2[0], loss, f"{tag}: loss")
        check_loss(out2[1], loss1, f"{tag}: loss at lamda 1")
        check(Pg, P.detach(), TOL_P, f"{tag}: P")
        check(dJ, Jd.grad, TOL_G, f"{tag}: dJ")


# ---------------------------------------------------------------- layer 3: the adjoint of the joint
@functools.lru_cache(maxsize=1)
def bwd_problem(case):
    N, H, W = case.shape
    k, pad, n = case.k, case.pad, mc.npix(case.shape)
    TT = (2 * pad + 1) ** 2
    gen = torch.Generator().manual_seed(7 * n + 10 * k + pad)
    x1, x2, dJ = rnd32(n, k, gen=gen), rnd32(n, k, gen=gen), rnd32(TT, k, k, gen=gen)
    g = torch.tensor([case.gscale], dtype=torch.float32)
    a = x1.double().view(N, H, W, k).requires_grad_(True)
    b = x2.double().view(N, H, W, k).requires_grad_(True)
    J = mc.raw_joint(a, b, pad) * (1.0 / n if case.normalise else 1.0)
    ((J * dJ.double()).sum() * g.double()[0]).backward()
    return x1, x2, dJ, g, a.grad.reshape(n, k), b.grad.reshape(n, k)


@pytest.mark.parametrize("case", mc.BWD_CASES, ids=mc.case_id)
def test_joint_backward(case):
    ops = _ops()
    x1, x2, dJ, g, r1, r2 = bwd_problem(case)
    k, pad = case.k, case.pad
    need1, need2 = "1" in case.need, "2" in case.need
    g1, g2, gdJ, gg = x1.to(DEV), x2.to(DEV), dJ.to(DEV), g.to(DEV)
    d1, d2 = ops.joint_bwd(g1, g2, gdJ, gg, *case.shape, k, pad, case.normalise, need1, need2)
    assert (d1 is None) == (not need1) and (d2 is None) == (not need2)
    e1, e2 = (nan_like(g1) if need1 else None), (nan_like(g2) if need2 else None)
    ops._lib.call("cy_joint_bwd", g1.data_ptr(), g2.data_ptr(), gdJ.data_ptr(), gg.data_ptr(), ops._ptr(e1),
                  ops._ptr(e2), *case.shape, k, pad, int(case.normalise), ops._stream())
    for what, got, again, ref in (("dx1", d1, e1, r1), ("dx2", d2, e2, r2)):
        if got is not None:
            assert torch.equal(got, again), f"{what}: two runs differ"
            check(got, ref, TOL_G, what)  # every pixel row


# ---------------------------------------------------------------- IIDFn end to end
@pytest.mark.parametrize("case", mc.IID_CASES, ids=mc.case_id)
def test_iid_fn_against_the_oracle(case):
    from cyhip.functions import IIDFn
    from oracle import next_rows as onr
    N, H, W = case.shape
    k = case.k
    gen = torch.Generator().manual_seed(31 * k + case.pad)
    p1 = torch.softmax(torch.randn(N, H, W, k, generator=gen), -1)  # float32 probabilities, NHWC
    p2 = torch.softmax(torch.randn(N, H, W, k, generator=gen), -1)
    a, b = p1.double().requires_grad_(True), p2.double().requires_grad_(True)
    if case.mode == 2:
        assert case.symmetric
        loss, loss1, P = onr.iid_loss(a.view(N, k), b.view(N, k), lamb=case.lamda)
        eps = 1e-10
    else:
        eps = 1e-5
        an, bn = a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2)
        loss = onr.iid_segmentation_loss(an, bn, lamda=case.lamda, padding=case.pad, eps=eps, symmetric=case.symmetric)
        loss1 = onr.iid_segmentation_loss(an, bn, lamda=1.0, padding=case.pad, eps=eps, symmetric=case.symmetric)
        P = onr.joint_maps(an, bn, case.pad, case.symmetric)
    loss.backward()
    runs = []
    for _ in range(2):
        x1, x2 = p1.to(DEV).requires_grad_(True), p2.to(DEV).requires_grad_(True)
        got, got1, gP = IIDFn.apply(x1, x2, case.mode, case.pad, case.symmetric, case.lamda, eps)
        got.backward()
        runs.append((got.detach(), got1, gP, x1.grad, x2.grad))
    assert all(torch.equal(u, v) for u, v in zip(*runs)), "two runs differ"
    got, got1, gP, d1, d2 = runs[0]
    check_loss(got, loss, "loss")
    check_loss(got1, loss1, "loss at lamda 1")
    check(gP, P.detach().reshape(-1, k, k), TOL_P, "P")
    check(d1, a.grad, TOL_G, "dx1")
    check(d2, b.grad, TOL_G, "dx2")


# ---------------------------------------------------------------- grouped softmax
@functools.lru_cache(maxsize=1)
def softmax_problem(case):
    """logits on a grid of 1/64 around a row offset of +-80: logits * (1/T) is exact in float32 for both T, so what is
    left is the kernel's own arithmetic; without the max-subtraction T = 0.1 overflows on one side and divides 0 by 0
    on the other"""
    M, S, k = case.M, case.S, case.k
    gen = torch.Generator().manual_seed(1000 * M + 10 * S + k)
    off = (torch.randint(0, 2, (M, 1), generator=gen) * 2 - 1).float() * mc.LOGIT_OFFSET
    logits = off + torch.randint(-64, 65, (M, S * k), generator=gen).float() / 64
    dp = rnd32(S, M, k, gen=gen)
    ld = logits.double().requires_grad_(True)
    probs = torch.softmax((ld / case.T).view(M, S, k), -1).permute(1, 0, 2)
    (probs * dp.double()).sum().backward()
    return logits, dp, probs.detach().contiguous(), ld.grad


@pytest.mark.parametrize("case", mc.SOFTMAX_CASES, ids=mc.case_id)
def test_group_softmax(case):
    ops = _ops()
    M, S, k, T = case
    logits, dp, probs, dl = softmax_problem(case)
    gl = logits.to(DEV)
    got = ops.group_softmax_fwd(gl, S, k, T)
    again = nan_like(got)
    ops._lib.call("cy_group_softmax_fwd", gl.data_ptr(), again.data_ptr(), M, S, k, 1.0 / T, ops._stream())
    assert torch.equal(got, again), "two forward runs differ"
    check(got, probs, TOL_P, "probs")
    check(got.sum(-1), torch.ones(S, M, dtype=torch.float64), TOL_P, "rows sum to 1")
    # the backward on the reference's probabilities (rounded to float32): a fault of the forward cannot hide one here
    gp, gdp = probs.float().to(DEV), dp.to(DEV)
    gd = ops.group_softmax_bwd(gp, gdp, T)
    again = torch.full((M, S * k), float("nan"), device=DEV, dtype=torch.float32)
    ops._lib.call("cy_group_softmax_bwd", gp.data_ptr(), gdp.data_ptr(), again.data_ptr(), M, S, k, 1.0 / T,
                  ops._stream())
    assert torch.equal(gd, again), "two backward runs differ"
    check(gd, dl, TOL_SM_G, "dlogits")


def test_group_softmax_fn_refuses_in_forward():
    """S*k > 255 is refused by GroupSoftmaxFn.forward, before any launch, not in .backward()"""
    from cyhip import _lib
    from cyhip.functions import GroupSoftmaxFn
    for S, k in mc.SOFTMAX_REFUSED:
        x = torch.zeros(5, S * k, device=DEV, requires_grad=True)
        with pytest.raises(_lib.HipKernelError, match="CY_ERR_SHAPE"):
            GroupSoftmaxFn.apply(x, S, k, 1.0)
    # ten sub-heads of twenty clusters: forward and backward
    x = torch.zeros(5, 200, device=DEV, requires_grad=True)
    GroupSoftmaxFn.apply(x, 10, 20, 1.0)[0].sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and math.isclose(x.grad.abs().max().item(), 0.0, abs_tol=1e-6)
