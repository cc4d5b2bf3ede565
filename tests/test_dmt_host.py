"""Host-side contract of the differentiable mean teacher (no kernel runs, no GPU): the exports, the C ABI's argument
checks with their exact statuses, the workspace formula, the launch rule's coverage -- every kernel variant and a second
trip of every capped loop `ops.teacher_plan` can report is reached by a case of tests/dmt_cases.py, which
tests/test_gpu_dmt_kernels.py runs --, the hook's signature against the reference's recorded one, what raises, and
FlatTeacher's constant number of launches."""
import ctypes as C
import inspect
from pathlib import Path

import pytest
import torch
from torch import nn

import dmt_cases as dc

OK, ARG, SHAPE, WORKSPACE = 0, -1, -2, -5
P = 4096  # stands for a 16-byte aligned device pointer: every call below is refused before anything is launched or read
ENTRIES = ("cy_teacher_plan", "cy_adam_step", "cy_axpy", "cy_ema_update_multi", "cy_softmax_gathermse_ws_bytes",
           "cy_softmax_gathermse_fwd", "cy_softmax_gathermse_bwd")


@pytest.fixture(scope="module")
def lib():
    from cyhip import _lib
    return _lib.load()


# ---- 1. exports --------------------------------------------------------------------------------------------------------
def test_exports(lib):
    from cyhip import _lib, functions, ops
    from contrastyou.optim import FlatTeacher
    from semi_seg.hooks import DifferentiableMeanTeacherTrainerHook
    assert set(ENTRIES) <= set(_lib.exported_names())
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert _lib.ABI_VERSION == 19 == lib.cy_abi_version()
    for name in ("adam_step", "axpy", "ema_update_multi", "ema_table", "softmax_gathermse_fwd", "softmax_gathermse_bwd",
                 "teacher_plan", "source_index_image", "source_map_from_warped"):
        assert callable(getattr(ops, name)), name
    assert issubclass(functions.SoftmaxGatherMSEFn, torch.autograd.Function)
    assert FlatTeacher is not None and DifferentiableMeanTeacherTrainerHook is not None
    assert (_lib.CY_TEACHER_ADAM, _lib.CY_TEACHER_AXPY, _lib.CY_TEACHER_EMA_MULTI, _lib.CY_TEACHER_GATHERMSE) == \
        (0, 1, 2, 3)


# ---- 2. refusals, each with its exact status ----------------------------------------------------------------------------
def _adam(lib, p=P, g=P, m=P, v=P, n=8, step=1):
    return lib.cy_adam_step(p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, None)


def test_adam_and_axpy_refusals(lib):
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=0), dict(n=-3), dict(step=0),
               dict(step=-1), dict(p=P + 2), dict(v=P + 1)):
        assert _adam(lib, **kw) == ARG, kw
    assert lib.cy_axpy(None, P, 8, 1.0, None) == ARG
    assert lib.cy_axpy(P, None, 8, 1.0, None) == ARG
    assert lib.cy_axpy(P, P, 0, 1.0, None) == ARG
    assert lib.cy_axpy(P, P + 2, 8, 1.0, None) == ARG


def test_ema_multi_refusals(lib):
    assert lib.cy_ema_update_multi(None, 1, 0.5, 0.0, None) == ARG
    assert lib.cy_ema_update_multi(P + 4, 1, 0.5, 0.0, None) == ARG  # the int64 table is 8-byte aligned
    for count in (0, -1, dc.EMA_MULTI_MAX + 1):
        assert lib.cy_ema_update_multi(P, count, 0.5, 0.0, None) == SHAPE, count


def _gfwd(lib, t=P, m=P, s=P, loss=P, N=2, HW=9, K=4, ws=P, nbytes=1 << 20):
    return lib.cy_softmax_gathermse_fwd(t, m, s, loss, N, HW, K, ws, nbytes, None)


def _gbwd(lib, t=P, m=P, s=P, g=P, d=P, N=2, HW=9, K=4):
    return lib.cy_softmax_gathermse_bwd(t, m, s, g, d, N, HW, K, None)


def test_gathermse_refusals(lib):
    for kw in (dict(t=None), dict(m=None), dict(s=None), dict(loss=None), dict(ws=None), dict(N=0), dict(HW=0),
               dict(t=P + 2), dict(m=P + 2), dict(s=P + 1)):
        assert _gfwd(lib, **kw) == ARG, kw
    for kw in (dict(t=None), dict(m=None), dict(s=None), dict(g=None), dict(d=None), dict(N=0), dict(HW=-1),
               dict(d=P + 1), dict(g=P + 2)):
        assert _gbwd(lib, **kw) == ARG, kw
    for K in (0, 1, 17, 64):
        assert _gfwd(lib, K=K) == SHAPE, K
        assert _gbwd(lib, K=K) == SHAPE, K
    need = lib.cy_softmax_gathermse_ws_bytes(2, 9)
    assert _gfwd(lib, nbytes=need - 1) == WORKSPACE
    assert _gfwd(lib, nbytes=0) == WORKSPACE


def test_plan_refusals(lib):
    from cyhip import _lib
    plan = _lib.TeacherPlan()
    assert lib.cy_teacher_plan(0, 8, 0, 16, None) == ARG
    assert lib.cy_teacher_plan(4, 8, 0, 16, plan) == ARG
    assert lib.cy_teacher_plan(-1, 8, 0, 16, plan) == ARG
    for form in range(4):
        assert lib.cy_teacher_plan(form, 0, 4, 16, plan) == ARG
        assert lib.cy_teacher_plan(form, 8, 4, 2, plan) == ARG
        assert lib.cy_teacher_plan(form, 8, 4, 0, plan) == ARG
    assert lib.cy_teacher_plan(2, dc.EMA_MULTI_MAX + 1, 0, 16, plan) == SHAPE
    assert lib.cy_teacher_plan(2, dc.EMA_MULTI_MAX, 0, 16, plan) == OK
    for K in (1, 17):
        assert lib.cy_teacher_plan(3, 8, K, 16, plan) == SHAPE
    for align in (4, 8):  # K == 4 on a base short of 16 bytes is the run-time form, as its neighbours are
        assert lib.cy_teacher_plan(3, 8, 4, align, plan) == OK and (plan.variant, plan.vec) == (0, 1)


def test_wrappers_refuse_cpu_tensors():
    from cyhip import ops
    from cyhip.functions import SoftmaxGatherMSEFn
    x = torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.adam_step(x, x, x, x, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.axpy(x, x, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ema_table([(x, x)], "cpu")
    z = torch.zeros(1, 3, 2, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SoftmaxGatherMSEFn.apply(z, torch.zeros(1, 2, 2, dtype=torch.int32), z)
    with pytest.raises(AssertionError, match="2\\^24"):
        ops.source_index_image(1, 4096, 4096, "cpu")


# ---- 3. workspace -------------------------------------------------------------------------------------------------------
def test_workspace_formula(lib):
    for N, HW in ((1, 1), (2, 153), (1, 256), (1, 257), (2, 131201), (4, 1 << 20)):
        assert lib.cy_softmax_gathermse_ws_bytes(N, HW) == 8 * min(dc.LOSS_BLOCK_CAP, -(-N * HW // 256)), (N, HW)
    assert lib.cy_softmax_gathermse_ws_bytes(0, 5) == 0 and lib.cy_softmax_gathermse_ws_bytes(2, 0) == 0


# ---- 4. the launch rule against the cases -------------------------------------------------------------------------------
def test_flat_plans_and_their_coverage():
    from cyhip import ops
    seen = set()
    for form in ("adam", "axpy"):
        for case in dc.FLAT_CASES:
            pl = ops.teacher_plan(form, case.n, align=4 if case.sliced else 16)
            vec = 4 if (not case.sliced and case.n >= 4) else 1
            groups = case.n // vec
            grid = min(dc.FLAT_GRID_CAP, -(-groups // 256))
            assert (pl["vec"], pl["fwd_grid"], pl["fwd_trips"]) == (vec, grid, -(-groups // (grid * 256))), case
            assert (pl["variant"], pl["bwd_grid"], pl["bwd_trips"], pl["rows"]) == (0, 0, 0, 0)
            seen.add((form, vec, pl["fwd_trips"] > 1, vec == 4 and case.n % 4 != 0))
    for form in ("adam", "axpy"):
        assert (form, 4, True, True) in seen      # vector form, second trip, with a scalar tail
        assert (form, 4, False, False) in seen    # vector form without a tail (256)
        assert (form, 1, True, False) in seen     # scalar form, second trip
        assert (form, 1, False, False) in seen
    assert dc.VEC_TRIP == dc.FLAT_GRID_CAP * 1024 and dc.SCALAR_TRIP == dc.FLAT_GRID_CAP * 256
    # every Adam case of the GPU file is one of these sizes
    assert {c for _, _, c, _ in dc.adam_cases()} <= set(dc.FLAT_CASES)


def test_ema_multi_plan_and_its_coverage():
    from cyhip import ops
    for count in (1, 2, 44, 128):
        pl = ops.teacher_plan("ema_multi", count)
        assert (pl["fwd_grid"], pl["rows"], pl["vec"]) == (dc.EMA_ROW_BLOCKS, count, 1)
        assert pl["fwd_trips"] == dc.EMA_ROW_BLOCKS * 256
    assert ops.teacher_plan("ema_multi", 1024)["fwd_grid"] == 8
    assert ops.teacher_plan("ema_multi", dc.EMA_MULTI_MAX)["fwd_grid"] == 2
    per_trip = dc.EMA_ROW_BLOCKS * 256
    for sizes in dc.ema_size_lists():
        assert len(sizes) in dc.EMA_COUNTS
    flat = [n for sizes in dc.ema_size_lists() for n in sizes]
    assert set(flat) == set(dc.EMA_SIZES)
    assert max(flat) > per_trip > 512          # a second trip, and tensors that leave most blocks idle
    assert any(len(s) == 44 and max(s) > per_trip for s in dc.ema_size_lists())


def test_gather_plan_and_its_coverage():
    from cyhip import ops
    seen = set()
    for case in dc.GATHER_CASES:
        npix = case.N * case.H * case.W
        pl = ops.teacher_plan("gathermse", npix, K=case.K, align=4 if case.sliced else 16)
        variant = case.K if (case.K in (2, 4, 8) and not case.sliced) else 0
        grid = min(dc.LOSS_BLOCK_CAP, -(-npix // 256))
        assert pl["variant"] == variant and pl["vec"] == {2: 2, 4: 4, 8: 4, 0: 1}[variant], case
        assert (pl["fwd_grid"], pl["bwd_grid"]) == (grid, 2 * grid), case
        assert pl["fwd_trips"] == -(-npix // (grid * 256)) and pl["bwd_trips"] == -(-npix // (2 * grid * 256)), case
        seen.add((variant, pl["fwd_trips"], pl["bwd_trips"]))
    assert {v for v, _, _ in seen} == {0, 2, 4, 8}
    assert any(f >= 2 for _, f, _ in seen)                      # past the forward's block cap
    assert any(b >= 2 for _, _, b in seen)                      # past the backward's
    assert (0, 1, 1) in seen and {c.K for c in dc.GATHER_CASES if c.sliced} == {2, 4, 8}
    assert {c.K for c in dc.GATHER_CASES} == {2, 3, 4, 5, 8, 13, 16}
    assert {c.map for c in dc.GATHER_CASES} >= {"identity", "outside", "random"}
    assert {(c.H, c.W) for c in dc.GATHER_CASES} >= {(17, 9), (1, 1)}
    assert all(c.N == 2 for c in dc.GATHER_CASES)
    assert dc.GATHER_BY_TAG["k2_past_cap"].N * dc.GATHER_BY_TAG["k2_past_cap"].W >= dc.LOSS_BLOCK_CAP * 256 + 257
    big = dc.GATHER_BY_TAG["k2_past_bwd_cap"]
    assert big.N * big.W >= 2 * dc.LOSS_BLOCK_CAP * 256 + 257
    assert ops.teacher_plan("gathermse", big.N * big.W, K=2)["bwd_trips"] == 2


def test_float64_restatement_agrees_with_torch_adam(golden_dir):
    """dmt_cases.adam64 is torch.optim.Adam: against torch's own float64 run, now and as recorded"""
    npz = dc.load(golden_dir)
    for step, wd, case, zero in dc.adam_cases():
        if case != dc.FlatCase(257, False):
            continue
        p, g, m, v = dc.adam_inputs(step, case.n, zero)
        mine = dc.adam64(p, g, m, v, step, wd)
        now = dc.adam_torch(p, g, m, v, step, wd, torch.float64)
        for name, a, b in zip(("p", "m", "v"), mine, now):
            rec = torch.from_numpy(npz[f"adam_s{step}_wd{wd:g}_z{int(zero)}_{name}"])
            assert dc.rel_max(a, b) < 1e-14 and dc.rel_max(a, rec) < 1e-14, (step, wd, zero, name)


# ---- 5. the hook's face --------------------------------------------------------------------------------------------------
def _names(fn):
    return [("**" + n if p.kind is p.VAR_KEYWORD else n) for n, p in inspect.signature(fn).parameters.items()
            if n != "self"]


def test_signature_is_the_references(golden_dir):
    from semi_seg.hooks import DifferentiableMeanTeacherTrainerHook as Hook
    line = (Path(golden_dir) / "dmt_signatures.txt").read_text().strip()
    name, names = line.split(": ")
    assert name == "DifferentiableMeanTeacherTrainerHook"
    assert _names(Hook.__init__) == names.split()
    sig = inspect.signature(Hook.__init__).parameters
    assert all(p.kind is p.KEYWORD_ONLY for n, p in sig.items() if n != "self")
    assert (sig["alpha"].default, sig["weight_decay"].default, sig["meta_weight"].default) == (0.999, 1e-5, 1e-3)
    assert sig["meta_criterion"].default is inspect.Parameter.empty
    assert sig["method_name"].default is inspect.Parameter.empty


def _hook(method, criterion="ce", name="dmt_host"):
    from semi_seg.hooks import DifferentiableMeanTeacherTrainerHook as Hook
    return Hook(name=name, model=dc.StandIn(), weight=0.3, meta_criterion=criterion, method_name=method)


def test_method3_and_unknown_methods_raise():
    with pytest.raises(NotImplementedError, match=r"mt_update.*required.*dmt\.py:356-360"):
        _hook("method3")
    for method in ("method5", "", "MT"):
        with pytest.raises(NotImplementedError):
            _hook(method)
    with pytest.raises(AssertionError):
        _hook("mt", criterion="mse")


def test_the_factory_and_the_trainer_still_raise():
    from semi_seg.hooks import create_differentiable_mt_hook
    from semi_seg.trainers import trainer_zoo
    with pytest.raises(NotImplementedError):
        trainer_zoo["dmt"]()
    with pytest.raises(NotImplementedError):
        create_differentiable_mt_hook(model=nn.Identity(), weight=0.1, meta_criterion="ce", method_name="mt")


def test_hook_face_on_the_host():
    from contrastyou.hooks.base import EpocherHook, TrainerHook
    from contrastyou.losses.dice_loss import DiceLoss
    from contrastyou.losses.kl import KL_div
    from semi_seg.hooks import EMAUpdater
    from semi_seg.hooks import dmt
    for method, cls, meters in (("mt", dmt.MTEpocherHook, ["loss"]),
                                ("method1", dmt.DifferentiableMeanTeacherEpocherHook1, ["consistency_loss", "teacher_loss"]),
                                ("method2", dmt.DifferentiableMeanTeacherEpocherHook2, ["consistency_loss", "teacher_loss"]),
                                ("method4", dmt.DifferentiableMeanTeacherEpocherHook4, ["consistency_loss", "teacher_loss"])):
        hook = _hook(method, "dice" if method == "method2" else "ce")
        assert isinstance(hook, TrainerHook) and hook.learnable_modules == [] and list(hook.parameters()) == []
        assert isinstance(hook._meta_criterion, DiceLoss if method == "method2" else KL_div)
        assert isinstance(hook._updater, EMAUpdater) and hook._updater._update_bn
        keys = sorted(hook.state_dict()["module_state"])
        assert [k for k in keys if k.startswith("_teacher_model.")] == \
            sorted("_teacher_model." + k for k in dc.StandIn().state_dict())
        assert not any("exp_avg" in k for k in keys) and hook.state_dict()["other_state"] == {}
        ep_hook = hook()
        assert type(ep_hook) is cls and isinstance(ep_hook, EpocherHook)
        ep_hook.meters = dc.Meters()
        ep_hook.configure_meters_given_epocher(ep_hook.meters)
        assert sorted(ep_hook.meters) == meters
        assert hook.teacher_model.training and ep_hook.teacher_model is hook.teacher_model


# ---- 6. FlatTeacher: a constant number of launches -------------------------------------------------------------------------
class _Many(nn.Module):
    """`layers` x (conv weight + bias, BatchNorm weight + bias + two statistics + counter)"""

    def __init__(self, layers: int):
        super().__init__()
        self.convs = nn.ModuleList(nn.Conv2d(2, 2, 1) for _ in range(layers))
        self.bns = nn.ModuleList(nn.BatchNorm2d(2) for _ in range(layers))


def _count_calls(monkeypatch, layers: int, flat_student: bool):
    from contrastyou.optim import FlatParams, FlatTeacher
    from cyhip import ops
    from semi_seg.hooks import EMAUpdater
    calls = []

    def wrap(name, result=None):
        def fn(*a, **k):
            calls.append(name)
            return result(*a, **k) if result else None
        monkeypatch.setattr(ops, name, fn)

    for name in ("adam_step", "axpy", "ema_update", "ema_update_multi"):
        wrap(name)
    wrap("ema_table", lambda pairs, device: torch.zeros(len(pairs), 3, dtype=torch.int64))
    torch.manual_seed(layers)
    teacher_model, student = _Many(layers), _Many(layers)
    if flat_student:
        FlatParams(list(student.parameters()))
    teacher = FlatTeacher(teacher_model)
    assert len(teacher.flat.params) == 4 * layers and len(teacher._float_bufs) == 2 * layers
    updater = EMAUpdater(update_bn=True)
    before = {k: v.clone() for k, v in teacher_model.state_dict().items()}
    for _ in range(2):
        teacher.zero_grad()
        teacher.snapshot()
        teacher.perturb(-1e-3)
        teacher.perturb(1e-3)
        with torch.no_grad():
            for p in teacher_model.parameters():
                p.add_(1.0)
            for b in teacher_model.buffers():
                b.add_(1)
        teacher.restore()
        teacher.adam_step(1e-3, 1e-5)
        teacher.ema_from(student, updater)
    assert updater._global_step == 2 and teacher.adam_steps == 2
    for k, v in teacher_model.state_dict().items():      # restore() put every parameter, statistic and counter back
        assert torch.equal(v, before[k]), k
    lo = teacher.flat.data.data_ptr()
    assert all(lo <= p.data_ptr() < lo + 4 * teacher.flat.numel for p in teacher_model.parameters())
    assert all(p.grad.data_ptr() == teacher.flat.grad.data_ptr() + 4 * off
               for p, off in zip(teacher_model.parameters(), teacher.flat.offsets))
    return calls


@pytest.mark.parametrize("flat_student", [False, True])
def test_flat_teacher_issues_a_constant_number_of_calls(monkeypatch, flat_student):
    small = _count_calls(monkeypatch, 3, flat_student)
    large = _count_calls(monkeypatch, 18, flat_student)   # 72 parameter tensors, 36 running statistics
    assert small == large
    per_step = ["axpy", "axpy", "adam_step"] + (["ema_update"] if flat_student else ["ema_update_multi"]) + \
        ["ema_update_multi"]
    tables = ["ema_table"] if flat_student else ["ema_table", "ema_table"]   # built once, cached on the second step
    assert sorted(large) == sorted(per_step * 2 + tables)
    assert large[:3] == ["axpy", "axpy", "adam_step"]
