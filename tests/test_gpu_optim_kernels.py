"""The flat-buffer optimizer kernels (csrc/cy_optim.hip) on the GPU: cy_sgd_step and cy_adamw_step against the float64
restatements of torch.optim's single-tensor update (tests/optim_cases.py), on every access form and past every cap.

Bounds: four times the largest distance from float64 of torch.optim's own f32 update on the CPU over the same cases, per
output, floored at 2^-23 (optim_cases: `bound`).  Every figure is printed before it is asserted."""
import pytest
import torch

import optim_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 777.25


def guarded(t: torch.Tensor, sliced: bool):
    """(view on the GPU holding t, its buffer, the guard floats in front): 4 guard floats in front -- 5 for a base that
    is only 4-byte aligned -- and 4 behind"""
    lead = 5 if sliced else 4
    buf = torch.full((t.numel() + lead + 4,), GUARD, device=DEV)
    view = buf[lead:lead + t.numel()]
    view.copy_(t.reshape(-1))
    assert view.data_ptr() % 16 == (4 if sliced else 0)
    return view, buf, lead


def guards_intact(buf, lead, n) -> bool:
    return bool((buf[:lead] == GUARD).all()) and bool((buf[lead + n:] == GUARD).all())


def place(ins, sliced):
    return [None if t is None else guarded(t, sliced) for t in ins]


def finish(placed, ins, n):
    """after the launch: guards, the read-only gradient; -> the outputs on the CPU (None where there is no buffer)"""
    torch.cuda.synchronize()
    for x in placed:
        assert x is None or guards_intact(x[1], x[2], n)
    assert torch.equal(placed[1][0].cpu(), ins[1])   # the gradient is read only
    return tuple(None if x is None else x[0].cpu() for i, x in enumerate(placed) if i != 1)


def run_sgd(c: oc.Case):
    from cyhip import ops
    ins = oc.sgd_inputs(c)
    placed = place(ins, c.flat.sliced)
    p, g, buf = (None if x is None else x[0] for x in placed)
    cfg = c.cfg
    ops.sgd_step(p, g, buf, cfg.lr, cfg.momentum, cfg.dampening, cfg.wd, cfg.nesterov, c.step == 1)
    return ins, finish(placed, ins, c.flat.n)


def run_adamw(c: oc.Case):
    from cyhip import ops
    ins = oc.adamw_inputs(c)
    placed = place(ins, c.flat.sliced)
    p, g, m, v, vmax = (None if x is None else x[0] for x in placed)
    cfg = c.cfg
    ops.adamw_step(p, g, m, v, vmax, cfg.lr, cfg.beta1, cfg.beta2, cfg.eps, cfg.wd, cfg.decoupled, c.step)
    return ins, finish(placed, ins, c.flat.n)


def check(kind, c, outputs, got, ref, yard):
    for k, a, b in zip(outputs, got, ref):
        assert (a is None) == (b is None), k
        if b is None:
            continue
        e, lim = oc.rel_max(a, b), oc.bound(yard[k])
        print(f"{kind} {oc.case_id(c)} {k}: {e:.3g} (<= {lim:.3g})")
        assert bool(torch.isfinite(a).all()) and e <= lim, (k, e, lim)


@pytest.mark.parametrize("c", oc.sgd_cases(), ids=oc.case_id)
def test_sgd(c):
    ins, got = run_sgd(c)
    check("sgd", c, oc.SGD_OUTPUTS, got, oc.sgd64(*ins, c.cfg, c.step == 1), oc.sgd_yardstick())
    if c.zero and c.cfg.wd == 0.0 and c.step == 1:   # zero state, zero gradient, no decay: nothing moves
        assert torch.equal(got[0], ins[0]) and (got[1] is None or not bool(got[1].any()))
    again = run_sgd(c)[1]
    assert all(a is None or torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("c", oc.adamw_cases(), ids=oc.case_id)
def test_adamw(c):
    ins, got = run_adamw(c)
    check("adamw", c, oc.ADAMW_OUTPUTS, got, oc.adamw64(*ins, c.cfg, c.step), oc.adamw_yardstick())
    again = run_adamw(c)[1]
    assert all(a is None or torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("amsgrad", (False, True))
@pytest.mark.parametrize("decoupled", (False, True))
def test_zero_gradient_zero_state_no_decay_moves_nothing(decoupled, amsgrad):
    cfg = oc.Adamw("still", 1e-3, 0.9, 0.999, 1e-8, 0.0, decoupled, amsgrad)
    for flat in (oc.AT_257, oc.FlatCase(257, True)):
        ins, got = run_adamw(oc.Case(cfg, 1, flat, True))
        assert torch.equal(got[0], ins[0])
        assert all(a is None or not bool(a.any()) for a in got[1:])


@pytest.mark.parametrize("flat", oc.FLAT_CASES, ids=lambda f: f"n{f.n}{'-slice' if f.sliced else ''}")
def test_adam_without_amsgrad_is_the_adam_kernel_bit_for_bit(flat):
    """cy_adamw_step(decoupled = 0, no maximum buffer) and FusedAdam(amsgrad=False)'s launch give the bits of
    ops.adam_step"""
    from contrastyou.optim import FusedAdam
    from cyhip import ops
    cfg = oc.Adamw("adam", 1e-3, 0.9, 0.999, 1e-8, 1e-5, False, False)
    c = oc.Case(cfg, 10, flat, False)
    ins = oc.adamw_inputs(c)[:4]
    outs = []
    for how in ("adam_step", "adamw_step", "FusedAdam"):
        p, g, m, v = (guarded(t, flat.sliced)[0] for t in ins)
        if how == "adam_step":
            ops.adam_step(p, g, m, v, cfg.lr, cfg.beta1, cfg.beta2, cfg.eps, cfg.wd, c.step)
        elif how == "adamw_step":
            ops.adamw_step(p, g, m, v, None, cfg.lr, cfg.beta1, cfg.beta2, cfg.eps, cfg.wd, False, c.step)
        else:
            opt = FusedAdam([torch.nn.Parameter(torch.zeros(1, device=DEV))], lr=cfg.lr, betas=(cfg.beta1, cfg.beta2),
                            eps=cfg.eps, weight_decay=cfg.wd)
            flat_bufs = type("Flat", (), {"data": p, "grad": g})
            opt._launch(opt.param_groups[0], flat_bufs, dict(exp_avg=m, exp_avg_sq=v), 0, flat.n, c.step)
        outs.append([t.cpu() for t in (p, m, v)])
    for other in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], other))
