"""The kernels of csrc/cy_pica.hip (PUILoss, PUISegLoss, JSD_div, EntropyPrior) past every launch cap, at their maxima
and on the branches the goldens do not reach, against the f64 formulas of tests/patch_losses_cases.py on the CPU.  The
cases and what each reaches: tests/pica_stream_cases.py; that they reach it: tests/test_pica_stream_coverage.py.

Tolerance: max(4 * e_ref, 1e-6) per kind, e_ref the larger of the fixture's stored e_ref of that kind and the case's own
f32-to-f64 distance of the formula on the CPU, which is computed here and printed.  No element is left out of any
comparison, and every figure is printed before it is asserted.
"""
import pytest
import torch

import patch_losses_cases as pc
import patch_losses_fixture as fx
import pica_stream_cases as ps

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def stored(golden_dir):
    return ps.fixture_e_ref(fx.load(golden_dir))


@pytest.fixture(scope="module")
def refs():
    """key -> (inputs, f64 reference, own distances), computed on first use and shared"""
    cache = {}

    def get(key, make_inputs, formula):
        if key not in cache:
            inputs = make_inputs()
            fn = formula(inputs)
            r64 = pc.reference(fn, inputs[0])
            own = ps.own_distances(ps.reference32(fn, inputs[0]), r64)
            print(f"{key}: own f32-to-f64 distance: value {own[0]:.2e}, gradients {own[1]}")
            cache[key] = (inputs, r64, own)
        return cache[key]
    return get


def leaf(t, fmt, need=True):
    t = t.detach().to(DEV).clone()
    if fmt == "nhwc":
        t = t.contiguous(memory_format=torch.channels_last)
    return t.requires_grad_(need)


def run(crit, ps_, fmt, needs):
    xs = [leaf(p, fmt, n) for p, n in zip(ps_, needs)]
    v = crit(*xs)
    (v if v.dim() == 0 else (v * fx.none_weights(v)).sum()).backward()
    return v.detach(), [x.grad for x in xs]


def check(what, stored, v, grads, needs, r64, own):
    """the value, and every gradient: a requested one against the formula, the others None"""
    assert v.shape == r64[0].shape, (what, v.shape, r64[0].shape)
    assert bool(torch.isfinite(v).all()), what
    pc.check_value(v, r64[0], ps.tolerances(stored, own[0], (0.0, 0.0)), f"{what} value")
    for i, (g, need) in enumerate(zip(grads, needs)):
        if not need:
            assert g is None, f"{what}: a gradient on input {i} that was not asked for"
            continue
        assert g is not None and bool(torch.isfinite(g).all()), (what, i)
        pc.check_grad(g, r64[1][i], ps.tolerances(stored, own[0], own[1][i]), f"{what} d input {i}")


def same(a, b):
    return torch.equal(a[0], b[0]) and all((u is None and w is None) or torch.equal(u, w) for u, w in zip(a[1], b[1]))


# ---------------------------------------------------------------------------------------------- JSD_div
def _jsd(c, refs):
    from contrastyou.losses.kl import JSD_div
    (xs,), r64, own = refs(f"jsd {c.name}", lambda: (ps.jsd_inputs(c),), lambda _: ps.jsd_formula(c))
    needs = [c.needs is None or i in c.needs for i in range(c.m)]
    return JSD_div(reduction=c.reduction, eps=ps.EPS), xs, needs, r64, own


@pytest.mark.parametrize("c", ps.JSD_CASES, ids=lambda c: c.name)
def test_jsd_div(stored, refs, c):
    crit, xs, needs, r64, own = _jsd(c, refs)
    before = [x.clone() for x in xs]
    v, grads = run(crit, xs, "nchw" if c.fmt == "rows" else c.fmt, needs)
    assert all(torch.equal(a, b) for a, b in zip(xs, before))
    check(f"JSD {c.name}", stored, v, grads, needs, r64, own)
    if c.kind == "zeros":
        k, g0 = ps.ZERO_CLASS, grads[0].cpu()
        assert bool((g0[:, k, ps.ZERO_BOTH] == 0).all()), "both maps and the mean exactly 0: a gradient of exactly 0"


# ---------------------------------------------------------------------------------------------- EntropyPrior
def _prior(c, refs):
    from contrastyou.losses.kl import EntropyPrior
    def make():
        x, prior = ps.prior_inputs(c)
        return [x], prior

    (xs, prior), r64, own = refs(f"prior {c.name}", make, lambda inp: ps.prior_formula(inp[1]))
    crit = EntropyPrior(eps=ps.EPS)
    pg = None if prior is None else prior.to(DEV)
    return (lambda x: crit(x, pg)), xs, r64, own


@pytest.mark.parametrize("c", ps.PRIOR_CASES, ids=lambda c: c.name)
def test_entropy_prior(stored, refs, c):
    crit, xs, r64, own = _prior(c, refs)
    v, grads = run(crit, xs, "nchw", [True])
    check(f"EntropyPrior {c.name}", stored, v, grads, [True], r64, own)


# ---------------------------------------------------------------------------------------------- PUILoss
def _pui(c, refs):
    from contrastyou.losses.pica_loss import PUILoss
    (xs,), r64, own = refs(f"pui {c.name}", lambda: (ps.pui_inputs(c),), lambda _: ps.pui_formula)
    return PUILoss(lamda=ps.PUI_LAMDA), xs, r64, own


@pytest.mark.parametrize("c", [c for c in ps.PUI_CASES if c.column is None], ids=lambda c: c.name)
def test_pui_loss(stored, refs, c):
    crit, xs, r64, own = _pui(c, refs)
    v, grads = run(crit, xs, "nchw", [True, True])
    check(f"PUI {c.name}", stored, v, grads, [True, True], r64, own)
    # one side only: the other launch of rows_axpb_kernel is not made
    for needs in ([True, False], [False, True]):
        v1, g1 = run(crit, xs, "nchw", needs)
        check(f"PUI {c.name} needs {needs}", stored, v1, g1, needs, r64, own)


@pytest.mark.parametrize("c", [c for c in ps.PUI_CASES if c.column is not None], ids=lambda c: c.name)
def test_pui_loss_clamped_column(stored, refs, c):
    """dy of the clamped column is of order 1e10, the others of order 1e-2: the clamped column and the other columns
    are compared apart, each against its own norm and maximum"""
    crit, xs, r64, own = _pui(c, refs)
    v, (dx, dy) = run(crit, xs, "nchw", [True, True])
    k = ps.CLAMPED_COLUMN
    others = [j for j in range(c.K) if j != k]
    xs32 = ps.reference32(ps.pui_formula, xs)
    pc.check_value(v, r64[0], ps.tolerances(stored, own[0], (0.0, 0.0)), f"PUI {c.name} value")
    pc.check_grad(dx, r64[1][0], ps.tolerances(stored, own[0], own[1][0]), f"PUI {c.name} dx")
    for cols, tag in (([k], "clamped column"), (others, "other columns")):
        e = fx.rel_grad(xs32[1][1][:, cols], r64[1][1][:, cols])
        print(f"PUI {c.name} dy, {tag}: own f32-to-f64 distance {e}")
        pc.check_grad(dy[:, cols], r64[1][1][:, cols], ps.tolerances(stored, own[0], e), f"PUI {c.name} dy, {tag}")


# ---------------------------------------------------------------------------------------------- PUISegLoss
def _seg(c, refs):
    from contrastyou.losses.pica_loss import PUISegLoss
    (xs,), r64, own = refs(f"puiseg {c.name}", lambda: (ps.seg_inputs(c),), lambda _: ps.seg_formula(c))
    return PUISegLoss(lamda=c.lamda, padding=c.pad), xs, r64, own


@pytest.mark.parametrize("c,fmt,needs", [(c, f, n) for c in ps.SEG_CASES for f, n in c.runs],
                         ids=lambda v: v.name if isinstance(v, ps.Seg) else v if isinstance(v, str) else
                         {ps.BOTH: "both", ps.X1_ONLY: "x1", ps.X2_ONLY: "x2"}[v])
def test_puiseg_loss(stored, refs, c, fmt, needs):
    crit, xs, r64, own = _seg(c, refs)
    v, grads = run(crit, xs, fmt, needs)
    check(f"PUISeg {c.name} {fmt}", stored, v, grads, needs, r64, own)


def test_puiseg_dx2_does_not_see_lamda(refs):
    """the two cases share their input; dx2 has no balance part and dJ does not depend on lamda: the same bits"""
    c0, c2 = ps.by_name(ps.SEG_CASES, "lam0"), ps.by_name(ps.SEG_CASES, "lam2")
    crit0, xs, _, _ = _seg(c0, refs)
    crit2, xs2, _, _ = _seg(c2, refs)
    assert all(torch.equal(a, b) for a, b in zip(xs, xs2))
    _, g0 = run(crit0, xs, "nchw", ps.BOTH)
    _, g2 = run(crit2, xs, "nchw", ps.BOTH)
    assert torch.equal(g0[1], g2[1])
    assert not torch.equal(g0[0], g2[0])


# ---------------------------------------------------------------------------------------------- determinism
def test_two_runs_past_the_cap_give_the_same_bits(refs):
    c = ps.by_name(ps.JSD_CASES, ps.SAME_BITS["jsd"])
    crit, xs, needs, _, _ = _jsd(c, refs)
    assert same(run(crit, xs, c.fmt, needs), run(crit, xs, c.fmt, needs)), "JSD_div"
    crit, xs, _, _ = _prior(ps.by_name(ps.PRIOR_CASES, ps.SAME_BITS["prior"]), refs)
    assert same(run(crit, xs, "nchw", [True]), run(crit, xs, "nchw", [True])), "EntropyPrior"
    crit, xs, _, _ = _pui(ps.by_name(ps.PUI_CASES, ps.SAME_BITS["pui"]), refs)
    assert same(run(crit, xs, "nchw", ps.BOTH), run(crit, xs, "nchw", ps.BOTH)), "PUILoss"
    crit, xs, _, _ = _seg(ps.by_name(ps.SEG_CASES, ps.SAME_BITS["seg"]), refs)
    assert same(run(crit, xs, "nchw", ps.BOTH), run(crit, xs, "nchw", ps.BOTH)), "PUISegLoss"
