"""The teacher kernels (csrc/cy_teacher.hip) on the GPU: Adam and axpy on flat buffers, the multi-tensor EMA and the
gather-MSE consistency term, against float64 (tests/dmt_cases.py), torch.optim.Adam's recorded float64 results
(tests/golden/dmt.npz) and, for the EMA, the bits of the per-tensor kernel.

Bounds: four times the largest distance from float64 of the reference's own f32 composition on the CPU over the same
cases (dmt_cases: `MARGIN`), a loss floored at 1.2e-6.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

import dmt_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 777.25


@pytest.fixture(scope="module")
def npz(golden_dir):
    return dc.load(golden_dir)


def guarded(t: torch.Tensor, sliced: bool):
    """(view on the GPU holding t, its buffer): 4 guard floats in front -- 5 for a base that is only 4-byte aligned --
    and 4 behind"""
    lead = 5 if sliced else 4
    buf = torch.full((t.numel() + lead + 4,), GUARD, device=DEV)
    view = buf[lead:lead + t.numel()]
    view.copy_(t.reshape(-1))
    assert view.data_ptr() % 16 == (4 if sliced else 0)
    return view, buf, lead


def guards_intact(buf, lead, n) -> bool:
    return bool((buf[:lead] == GUARD).all()) and bool((buf[lead + n:] == GUARD).all())


# ---------------------------------------------------------------- Adam
def adam_id(c):
    step, wd, case, zero = c
    return f"s{step}-wd{wd:g}-n{case.n}{'-slice' if case.sliced else ''}{'-zero' if zero else ''}"


@functools.lru_cache(maxsize=None)
def adam_yardstick():
    """torch.optim.Adam in f32 on the CPU against float64, the largest over the cases, per output"""
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for step, wd, case, zero in dc.adam_cases():
        p, g, m, v = dc.adam_inputs(step, case.n, zero)
        ref = dc.adam64(p, g, m, v, step, wd)
        got = dc.adam_torch(p, g, m, v, step, wd, torch.float32)
        for k, a, b in zip(worst, got, ref):
            worst[k] = max(worst[k], dc.rel_max(a, b))
    print("Adam yardstick:", {k: f"{e:.3g}" for k, e in worst.items()})
    return worst


def run_adam(step, wd, case, zero):
    from cyhip import ops
    ins = dc.adam_inputs(step, case.n, zero)
    placed = [guarded(t, case.sliced) for t in ins]
    (p, g, m, v) = (x[0] for x in placed)
    ops.adam_step(p, g, m, v, dc.ADAM["lr"], dc.ADAM["beta1"], dc.ADAM["beta2"], dc.ADAM["eps"], wd, step)
    torch.cuda.synchronize()
    for view, buf, lead in placed:
        assert guards_intact(buf, lead, case.n)
    assert torch.equal(g.cpu(), ins[1])  # the gradient is read only
    return ins, (p.cpu(), m.cpu(), v.cpu())


@pytest.mark.parametrize("c", dc.adam_cases(), ids=adam_id)
def test_adam(c, npz):
    step, wd, case, zero = c
    ins, got = run_adam(step, wd, case, zero)
    ref = dc.adam64(*ins, step, wd)
    yard = adam_yardstick()
    for k, a, b in zip(("p", "m", "v"), got, ref):
        e, lim = dc.rel_max(a, b), dc.bound(yard[k])
        print(f"adam {adam_id(c)} {k}: {e:.3g} (<= {lim:.3g})")
        assert bool(torch.isfinite(a).all()) and e <= lim, (k, e, lim)
        key = f"adam_s{step}_wd{wd:g}_z{int(zero)}_{k}"
        if case == dc.FlatCase(257, False):   # torch.optim.Adam's own float64 result, as recorded
            e = dc.rel_max(a, torch.from_numpy(npz[key]))
            assert e <= lim, (key, e, lim)
    if zero and wd == 0.0 and step == 1:   # zero moments, zero gradient: nothing moves
        assert torch.equal(got[0], ins[0])
    again = run_adam(step, wd, case, zero)[1]
    assert all(torch.equal(a, b) for a, b in zip(got, again))


# ---------------------------------------------------------------- axpy
@functools.lru_cache(maxsize=None)
def axpy_yardstick():
    worst = 0.0
    for n in (1, 255, 256, 257):
        y, x = dc.axpy_inputs(n)
        for a in dc.AXPY_ALPHAS:
            worst = max(worst, dc.rel_max(y.clone().add_(x, alpha=a), y.double() + float(np.float32(a)) * x.double()))
    print(f"axpy yardstick: {worst:.3g}")
    return worst


@pytest.mark.parametrize("case", dc.FLAT_CASES, ids=lambda c: f"n{c.n}{'-slice' if c.sliced else ''}")
def test_axpy(case):
    from cyhip import ops
    y0, x0 = dc.axpy_inputs(case.n)
    lim = dc.bound(axpy_yardstick())
    for a in dc.AXPY_ALPHAS:
        outs = []
        for _ in range(2):
            (y, ybuf, lead), (x, xbuf, _) = guarded(y0, case.sliced), guarded(x0, case.sliced)
            ops.axpy(y, x, a)
            torch.cuda.synchronize()
            assert guards_intact(ybuf, lead, case.n) and guards_intact(xbuf, lead, case.n)
            assert torch.equal(x.cpu(), x0)
            outs.append(y.cpu())
        e = dc.rel_max(outs[0], y0.double() + float(np.float32(a)) * x0.double())
        print(f"axpy n{case.n} a{a}: {e:.3g} (<= {lim:.3g})")
        assert e <= lim and torch.equal(outs[0], outs[1])
    # the method-2 pair: there and back is the reference's arithmetic (two roundings), not a copy
    (y, _, _), (x, _, _) = guarded(y0, case.sliced), guarded(x0, case.sliced)
    ops.axpy(y, x, -1e-3)
    ops.axpy(y, x, 1e-3)
    back = y.cpu()
    ref = (y0.double() - float(np.float32(1e-3)) * x0.double()) + float(np.float32(1e-3)) * x0.double()
    assert dc.rel_max(back, ref) <= 2 * lim


# ---------------------------------------------------------------- multi-tensor EMA
@pytest.mark.parametrize("sizes", dc.ema_size_lists(), ids=lambda s: f"{len(s)}x{max(s)}")
@pytest.mark.parametrize("alpha,wd", dc.EMA_SETS)
def test_ema_multi_equals_the_per_tensor_kernel(sizes, alpha, wd):
    from cyhip import ops
    pairs = dc.ema_inputs(sizes)
    # one arena for all tensors, four guard floats between neighbours; odd offsets: bases of every alignment
    def arena():
        ts, ss, bufs = [], [], []
        for i, (t, s) in enumerate(pairs):
            tv, tb, lead = guarded(t, i % 2 == 1)
            ts.append(tv), ss.append(s.to(DEV)), bufs.append((tb, lead, t.numel()))
        return ts, ss, bufs
    ts, ss, bufs = arena()
    table = ops.ema_table(list(zip(ts, ss)), DEV)
    assert table.shape == (len(sizes), 3) and table.dtype == torch.int64
    ops.ema_update_multi(table, alpha, wd)
    torch.cuda.synchronize()
    for tb, lead, n in bufs:
        assert guards_intact(tb, lead, n)
    ts1, ss1, _ = arena()
    for t, s in zip(ts1, ss1):
        ops.ema_update(t, s, alpha, wd)
    torch.cuda.synchronize()
    af, wf = float(np.float32(alpha)), float(np.float32(wd))
    for i, (a, b) in enumerate(zip(ts, ts1)):
        assert torch.equal(a, b), (i, sizes[i])          # bit for bit
        ref = (af * pairs[i][0].double() + (1 - af) * pairs[i][1].double()) * (1 - wf)
        assert dc.rel_max(a, ref) <= 1e-6, (i, sizes[i])
    assert all(torch.equal(s.cpu(), p[1]) for s, p in zip(ss, pairs))   # the students are read only
    # a second launch over the same table moves the teachers again, and to the same bits as the per-tensor kernel
    ops.ema_update_multi(table, alpha, wd)
    for t, s in zip(ts1, ss1):
        ops.ema_update(t, s, alpha, wd)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ts, ts1))


def test_ema_table_limits():
    from cyhip import ops
    x = torch.zeros(4, device=DEV)
    with pytest.raises(ValueError, match="1..4096"):
        ops.ema_table([], DEV)
    with pytest.raises(ValueError, match="1..4096"):
        ops.ema_table([(x, x)] * 4097, DEV)
    with pytest.raises(AssertionError):
        ops.ema_table([(x, x[:3])], DEV)


# ---------------------------------------------------------------- gather-MSE
@functools.lru_cache(maxsize=None)
def gather_ref(tag):
    return dc.gather_reference(dc.GATHER_BY_TAG[tag])


@functools.lru_cache(maxsize=None)
def gather_bounds():
    """(yardstick, bound) for loss, grad2, gradmax over the cases"""
    refs = [gather_ref(c.tag) for c in dc.GATHER_CASES]
    out = []
    for i in range(3):
        e = max(r[2][i] for r in refs)
        out.append((e, dc.bound(e, loss=(i == 0))))
    print("gather-MSE (yardstick, bound): loss %.3g %.3g  grad2 %.3g %.3g  gradmax %.3g %.3g"
          % tuple(v for pair in out for v in pair))
    return out


def place(z, sliced):
    """logits [N,K,H,W] on the GPU with NHWC memory; `sliced`: rows that start one float into a larger buffer"""
    N, K, H, W = z.shape
    lead = 5 if sliced else 4
    buf = torch.full((z.numel() + lead + 4,), GUARD, device=DEV)
    t = buf[lead:lead + z.numel()].view(N, H, W, K).permute(0, 3, 1, 2)
    t.copy_(z)
    assert t.data_ptr() % 16 == (4 if sliced else 0)
    return t, buf, lead


@functools.lru_cache(maxsize=None)
def run_gather(tag):
    """two runs of SoftmaxGatherMSEFn forward + backward -> [(loss, dstudent) x 2] on the CPU"""
    from cyhip.functions import SoftmaxGatherMSEFn
    case = dc.GATHER_BY_TAG[tag]
    t, s = dc.gather_inputs(case)
    m = dc.gather_map(case).to(DEV).view(case.N, case.H, case.W)
    runs = []
    for _ in range(2):
        (td, tbuf, lead), (sd, sbuf, _) = place(t, case.sliced), place(s, case.sliced)
        sd.requires_grad_(True)
        loss = SoftmaxGatherMSEFn.apply(td, m, sd)
        (loss * 1.0).backward()
        torch.cuda.synchronize()
        assert guards_intact(tbuf, lead, t.numel()) and guards_intact(sbuf, lead, s.numel())
        assert torch.equal(td.cpu(), t) and torch.equal(sd.detach().cpu(), s)
        assert sd.grad.shape == s.shape and not td.requires_grad
        runs.append((loss.detach().cpu(), sd.grad.cpu().contiguous()))
    return runs


@pytest.mark.parametrize("case", dc.GATHER_CASES, ids=lambda c: c.tag)
def test_gathermse(case):
    v64, g64, _ = gather_ref(case.tag)
    (loss, grad), (loss2, grad2) = run_gather(case.tag)
    lims = gather_bounds()
    e = [dc.rel_scalar(loss, v64), *dc.rel_grad(grad, g64)]
    print(f"gather-MSE {case.tag}: loss {e[0]:.3g} (<= {lims[0][1]:.3g})  grad2 {e[1]:.3g} (<= {lims[1][1]:.3g})  "
          f"gradmax {e[2]:.3g} (<= {lims[2][1]:.3g})")
    assert np.isfinite(float(loss)) and bool(torch.isfinite(grad).all())
    assert all(x <= lim for x, (_, lim) in zip(e, lims)), (case.tag, e, lims)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)   # no atomics: the same bits run to run


def test_gathermse_semantics():
    """an all-outside map is the MSE against zero; an identity map is SoftmaxMSEFn on the same logits; the upstream
    gradient scales the student's; a map value past the image counts as outside"""
    from cyhip.functions import SoftmaxGatherMSEFn, SoftmaxMSEFn
    case = dc.GATHER_BY_TAG["k4_rand"]
    t, s = (x.to(DEV) for x in dc.gather_inputs(case))
    HW = case.H * case.W
    outside = torch.full((case.N, case.H, case.W), -1, dtype=torch.int32, device=DEV)
    got = SoftmaxGatherMSEFn.apply(t, outside, s)
    ref = s.double().softmax(1).pow(2).mean()
    assert dc.rel_scalar(got, ref) <= gather_bounds()[0][1]
    past = torch.full_like(outside, HW)
    assert torch.equal(SoftmaxGatherMSEFn.apply(t, past, s), got)
    ident = torch.arange(HW, dtype=torch.int32, device=DEV).repeat(case.N).view(case.N, case.H, case.W)
    a = SoftmaxGatherMSEFn.apply(t, ident, s)
    b = SoftmaxMSEFn.apply(t, s)
    assert dc.rel_scalar(a, b.double()) <= gather_bounds()[0][1]
    m = dc.gather_map(case).to(DEV).view(case.N, case.H, case.W)
    s1, s2 = s.clone().requires_grad_(True), s.clone().requires_grad_(True)
    SoftmaxGatherMSEFn.apply(t, m, s1).backward()
    (SoftmaxGatherMSEFn.apply(t, m, s2) * 0.25).backward()
    assert dc.rel_grad(s2.grad, 0.25 * s1.grad.double())[1] <= 1e-6


def test_source_map_through_the_affine_kernel():
    """the hook's way to the map: an image of pixel index + 1 through the step's nearest-neighbour kernel; the map
    then reproduces that kernel's warp of any tensor, bit for bit"""
    from cyhip import ops
    from semi_seg.augment import AffineAugment
    N, H, W = 2, 17, 9
    aug = AffineAugment(scale=(0.8, 1.3), rotation=(-45, 45), translation=(-0.1, 0.1), mirror_p=0.9, gamma=(0.5, 2))
    warp = lambda x: aug(x, mode="feature", seed=11)  # noqa: E731
    smap = ops.source_map_from_warped(warp(ops.source_index_image(N, H, W, DEV)))
    assert smap.dtype == torch.int32 and smap.shape == (N, H, W)
    assert int(smap.min()) >= -1 and int(smap.max()) < H * W and bool((smap == -1).any())
    x = torch.randn(N, 5, H, W, device=DEV)
    assert torch.equal(warp(x).contiguous(), dc.warp_by_map(x, smap.view(N, -1)))
