"""Host-side contract of the flat-buffer SGD / Adam / AdamW (no kernel runs, no GPU): the float64 restatements of
tests/optim_cases.py against torch.optim in float64, the launch rule's coverage by the cases, the C ABI's argument checks
with their exact statuses, and the optimizer classes: torch's constructor signatures and errors, the names
contrastyou.optim exports, the checkpoint schema and FusedRAdam's new base."""
import ctypes as C
import inspect

import pytest
import torch
from torch import nn

import optim_cases as oc

OK, ARG = 0, -1
P = 4096  # stands for a 16-byte aligned device pointer: every call below is refused before anything is launched or read


@pytest.fixture(scope="module")
def lib():
    from cyhip import _lib
    return _lib.load()


# ---- 1. the restatements are torch.optim --------------------------------------------------------------------------------
def test_restatements_equal_torch_in_float64():
    for c in oc.sgd_cases():
        ins = oc.sgd_inputs(c)
        got, ref = oc.sgd64(*ins, c.cfg, c.step == 1), oc.sgd_torch(*ins, c.cfg, c.step == 1, torch.float64)
        assert (got[1] is None) == (ref[1] is None) == (c.cfg.momentum == 0)
        for a, b in zip(got, ref):
            assert a is None or oc.rel_max(a, b) <= 1e-14, oc.case_id(c)
    for c in oc.adamw_cases():
        ins = oc.adamw_inputs(c)
        got, ref = oc.adamw64(*ins, c.cfg, c.step), oc.adamw_torch(*ins, c.cfg, c.step, torch.float64)
        assert (got[3] is None) == (ref[3] is None) == (not c.cfg.amsgrad)
        for a, b in zip(got, ref):
            assert a is None or oc.rel_max(a, b) <= 1e-14, oc.case_id(c)


def test_yardsticks_are_not_zero():
    for k, e in {**oc.sgd_yardstick(), **{"adamw " + k: v for k, v in oc.adamw_yardstick().items()}}.items():
        assert 1e-8 < e < 1e-6, (k, e)


def test_the_cases_are_what_the_docstring_lists():
    for cases, configs in ((oc.sgd_cases(), oc.SGD_CONFIGS), (oc.adamw_cases(), oc.ADAMW_CONFIGS)):
        at257 = {(c.cfg.tag, c.step) for c in cases if c.flat == oc.AT_257 and not c.zero}
        assert at257 == {(cfg.tag, st) for cfg in configs for st in oc.STEPS}
        assert {c.flat for c in cases if c.step == 10} == set(oc.FLAT_CASES)
        assert {(c.cfg.tag, c.step) for c in cases if c.zero} == {(cfg.tag, st) for cfg in configs for st in (1, 10)}
    assert [c.n for c in oc.FLAT_CASES] == [1, 255, 256, 257, 2048 * 256 * 4 + 1, 2048 * 256 * 4 + 257, 257,
                                            2048 * 256 + 257]
    assert [c.sliced for c in oc.FLAT_CASES] == [False] * 6 + [True] * 2


# ---- 2. the launch rule against the cases -------------------------------------------------------------------------------
def test_plans_and_their_coverage(lib):
    from cyhip import ops
    seen = set()
    for form in ("sgd", "adamw"):
        for case in oc.FLAT_CASES:
            align = 4 if case.sliced else 16
            pl = ops.optim_plan(form, case.n, align=align)
            vec = 4 if (not case.sliced and case.n >= 4) else 1
            groups = case.n // vec
            grid = min(oc.FLAT_GRID_CAP, -(-groups // 256))
            assert pl == dict(vec=vec, grid=grid, trips=-(-groups // (grid * 256)), tail=case.n % 4 if vec == 4 else 0)
            adam = ops.teacher_plan("adam", case.n, align=align)  # the rule cy_teacher_plan gives Adam
            assert (pl["vec"], pl["grid"], pl["trips"]) == (adam["vec"], adam["fwd_grid"], adam["fwd_trips"])
            seen.add((form, vec, pl["trips"] > 1, pl["tail"] > 0))
    for form in ("sgd", "adamw"):
        assert (form, 4, True, True) in seen      # vector form, second trip of its cap, with a scalar tail
        assert (form, 4, False, False) in seen    # vector form without a tail (256)
        assert (form, 4, False, True) in seen
        assert (form, 1, True, False) in seen     # one float at a time, second trip of its cap
        assert (form, 1, False, False) in seen
    assert ops.optim_plan("sgd", 8, align=8)["vec"] == 1 and ops.optim_plan("sgd", 8, align=32)["vec"] == 4
    assert ops.optim_plan("adamw", 3, align=16) == dict(vec=1, grid=1, trips=1, tail=0)


def test_plan_refusals(lib):
    from cyhip import _lib, ops
    assert (_lib.CY_OPTIM_SGD, _lib.CY_OPTIM_ADAMW) == (0, 1)
    assert _lib.ABI_VERSION == 19 == lib.cy_abi_version()
    plan = _lib.OptimPlan()
    assert lib.cy_optim_plan(0, 8, 16, None) == ARG
    for form in (-1, 2):
        assert lib.cy_optim_plan(form, 8, 16, plan) == ARG
    for form in (0, 1):
        assert lib.cy_optim_plan(form, 8, 16, plan) == OK
        for n, align in ((0, 16), (-3, 16), (8, 2), (8, 0), (8, 6)):
            assert lib.cy_optim_plan(form, n, align, plan) == ARG, (form, n, align)
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_ARG"):
        ops.optim_plan("sgd", 0)


# ---- 3. refusals of the launches, each with its exact status -------------------------------------------------------------
def _sgd(lib, p=P, g=P, b=P, n=8, momentum=0.9):
    return lib.cy_sgd_step(p, g, b, n, 0.1, momentum, 0.0, 0.0, 0, 0, None)


def _adamw(lib, p=P, g=P, m=P, v=P, x=P, n=8, step=1, decoupled=1):
    return lib.cy_adamw_step(p, g, m, v, x, n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, decoupled, step, None)


def test_sgd_refusals(lib):
    for kw in (dict(p=None), dict(g=None), dict(n=0), dict(n=-3), dict(p=P + 2), dict(g=P + 1), dict(b=P + 2),
               dict(b=None),                      # momentum != 0 without a buffer
               dict(momentum=0.0),                # a buffer without momentum
               dict(p=None, b=None, momentum=0.0), dict(n=0, b=None, momentum=0.0),
               dict(g=P + 2, b=None, momentum=0.0)):
        assert _sgd(lib, **kw) == ARG, kw


def test_adamw_refusals(lib):
    for dec in (0, 1):
        for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=0), dict(n=-3), dict(step=0),
                   dict(step=-1), dict(p=P + 2), dict(v=P + 1), dict(x=P + 2), dict(x=None, m=P + 1),
                   dict(x=None, step=0), dict(x=None, n=0)):
            assert _adamw(lib, decoupled=dec, **kw) == ARG, (dec, kw)


def test_wrappers_refuse_cpu_tensors():
    from cyhip import ops
    x = torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sgd_step(x, x, None, 0.1, 0.0, 0.0, 0.0, False, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sgd_step(x, x, x, 0.1, 0.9, 0.0, 0.0, False, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.adamw_step(x, x, x, x, None, 1e-3, 0.9, 0.999, 1e-8, 1e-2, True, 1)


# ---- 4. the classes ---------------------------------------------------------------------------------------------------
def _classes():
    from contrastyou import optim
    return ((optim.FusedSGD, torch.optim.SGD), (optim.FusedAdam, torch.optim.Adam), (optim.FusedAdamW, torch.optim.AdamW))


def test_exports_and_bases():
    from contrastyou import optim
    from contrastyou.optim.flat_optimizer import FlatOptimizer, FlatParams
    from contrastyou.optim.fused_radam import FlatParams as SamePlace, FusedRAdam
    assert optim.SGD is optim.FusedSGD and optim.Adam is optim.FusedAdam and optim.AdamW is optim.FusedAdamW
    assert optim.RAdam is FusedRAdam and SamePlace is FlatParams
    assert FlatOptimizer in FusedRAdam.__mro__ and FusedRAdam.__module__ == "contrastyou.optim.fused_radam"
    for ours, _ in _classes():
        assert issubclass(ours, FlatOptimizer) and issubclass(ours, torch.optim.Optimizer)
    assert FusedRAdam.BUCKET_ELEMS == 16 << 20
    from cyhip import ops
    for name in ("sgd_step", "adamw_step", "optim_plan"):
        assert callable(getattr(ops, name)), name


def test_constructor_signatures_follow_torch():
    for ours, theirs in _classes():
        mine = inspect.signature(ours.__init__).parameters
        ref = inspect.signature(theirs.__init__).parameters
        positional = [n for n, p in ref.items() if p.kind is p.POSITIONAL_OR_KEYWORD]
        assert [n for n, p in mine.items() if p.kind is p.POSITIONAL_OR_KEYWORD] == positional, ours
        for n in positional[2:]:
            assert mine[n].default == ref[n].default, (ours, n)
        for n, p in ref.items():   # every keyword torch takes is taken, with torch's default
            if p.kind is p.KEYWORD_ONLY:
                assert mine[n].kind is p.KEYWORD_ONLY and mine[n].default == p.default, (ours, n)
        assert {"process_group", "data_parallel"} <= set(mine)


BAD_ARGS = {
    "SGD": (dict(lr=-1.0), dict(momentum=-0.5), dict(weight_decay=-1e-4), dict(nesterov=True),
            dict(nesterov=True, momentum=0.9, dampening=0.1)),
    "Adam": (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.0)), dict(betas=(-0.1, 0.9)),
             dict(weight_decay=-1e-4)),
}


def test_constructor_errors_are_torchs():
    for ours, theirs in _classes():
        for kw in BAD_ARGS["SGD" if theirs is torch.optim.SGD else "Adam"]:
            with pytest.raises(ValueError) as ref:
                theirs([nn.Parameter(torch.zeros(2))], **kw)
            with pytest.raises(ValueError) as got:
                ours([nn.Parameter(torch.zeros(2))], **kw)
            assert str(got.value) == str(ref.value), (ours, kw)


def test_flags_that_change_the_step_raise():
    for ours, theirs in _classes():
        flags = ("maximize", "differentiable", "fused") + (() if theirs is torch.optim.SGD else ("capturable",))
        for flag in flags:
            with pytest.raises(NotImplementedError, match=flag):
                ours([nn.Parameter(torch.zeros(2))], **{flag: True})
        for kw in (dict(foreach=True), dict(foreach=False), dict(foreach=None, fused=None, maximize=False),
                   dict(fused=False, differentiable=False)):
            ours([nn.Parameter(torch.zeros(2))], **kw)


def test_defaults_and_groups():
    from contrastyou import optim
    a, b = nn.Parameter(torch.zeros(3)), nn.Parameter(torch.zeros(2))
    opt = optim.SGD([{"params": [a], "lr": 0.5, "momentum": 0.9}, {"params": [b], "weight_decay": 1e-3}], lr=0.1)
    g0, g1 = opt.param_groups
    assert (g0["lr"], g0["momentum"], g0["weight_decay"], g0["nesterov"]) == (0.5, 0.9, 0, False)
    assert (g1["lr"], g1["momentum"], g1["weight_decay"], g1["dampening"]) == (0.1, 0, 1e-3, 0)
    assert optim.AdamW([a]).param_groups[0]["weight_decay"] == 1e-2 and optim.Adam([a]).param_groups[0]["weight_decay"] == 0
    assert optim.AdamW([a]).param_groups[0]["decoupled_weight_decay"] is True
    assert optim.Adam([a]).param_groups[0]["decoupled_weight_decay"] is False
    assert optim.Adam(params=[a], lr=1e-4, weight_decay=1e-5).param_groups[0]["lr"] == 1e-4   # the trainer's call form
    assert not opt._dp and opt._flat == [None, None]
    opt.add_param_group({"params": [nn.Parameter(torch.zeros(1))]})
    assert opt._flat == [None, None, None]


def test_state_dict_schema_on_cpu_buffers():
    """the flat buffers are built at the first zero_grad(), on the parameters' device: the schema, the parameters
    re-pointed into one buffer per group, and a load that waits for the flat buffers"""
    from contrastyou import optim
    torch.manual_seed(0)
    expect = {optim.SGD: (dict(momentum=0.9), ["momentum_buffer"]), optim.Adam: (dict(), ["exp_avg", "exp_avg_sq"]),
              optim.AdamW: (dict(amsgrad=True), ["exp_avg", "exp_avg_sq", "max_exp_avg_sq"])}
    for cls, (kw, names) in expect.items():
        net, head = nn.Linear(5, 3), nn.Linear(3, 2)
        opt = cls([{"params": list(net.parameters())}, {"params": list(head.parameters()), "lr": 0.5}], lr=0.1, **kw)
        opt.zero_grad()
        assert net.weight.data_ptr() == opt._flat[0].data.data_ptr()
        assert net.bias.data_ptr() == opt._flat[0].data.data_ptr() + 4 * 15
        assert net.bias.grad.data_ptr() == opt._flat[0].grad.data_ptr() + 4 * 15
        sd = opt.state_dict()
        assert set(sd) == {"param_groups", "flat"} and set(sd["flat"]) == {0, 1}
        assert list(sd["flat"][0]) == ["step", "steps", *names]
        assert sd["flat"][0]["step"] == 0 and sd["flat"][0]["steps"] == [0, 0]
        assert all(sd["flat"][0][k].shape == (18,) and sd["flat"][1][k].shape == (8,) for k in names)
        assert "params" not in sd["param_groups"][0] and sd["param_groups"][1]["lr"] == 0.5
        # a checkpoint loaded before the flat buffers exist is handed back as loaded, and applied when they are built
        sd["flat"][0] = dict(sd["flat"][0], step=7, steps=[7, 6], **{k: torch.full((18,), 0.25) for k in names})
        sd["param_groups"][0]["lr"] = 0.01
        fresh = cls([{"params": list(nn.Linear(5, 3).parameters())}, {"params": list(nn.Linear(3, 2).parameters())}],
                    lr=0.1, **kw)
        fresh.load_state_dict(sd)
        assert fresh.param_groups[0]["lr"] == 0.01 and fresh.state_dict()["flat"] is sd["flat"]
        fresh.zero_grad()
        st = fresh._flat_state[0]
        assert (st["step"], st["steps"]) == (7, [7, 6]) and all(bool((st[k] == 0.25).all()) for k in names)
    plain = optim.SGD([nn.Parameter(torch.zeros(4))], lr=0.1)
    plain.zero_grad()
    assert list(plain.state_dict()["flat"][0]) == ["step", "steps"]     # no momentum, no buffer


def test_step_has_no_cpu_path():
    from contrastyou import optim
    for cls in (optim.SGD, optim.Adam, optim.AdamW):
        lin = nn.Linear(3, 2)
        opt = cls(lin.parameters(), lr=0.1)
        opt.zero_grad()
        lin(torch.ones(1, 3)).sum().backward()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            opt.step()
