"""Host-side contract of the MixUp / ICT family (no kernel runs, no GPU): the draw against the reference's recorded one,
the f64 restatement of the formulas against the reference's recorded f64 values, the Python names and signatures
against tests/golden/mixup_signatures.txt (both written by tests/golden/gen_goldens_mixup.py), the class hierarchy, the
C ABI's argument checks, and the launch rule's coverage: every kernel variant and every capped loop `ops.mix_plan` can
report is reached by a case of tests/mixup_cases.py, which tests/test_gpu_mixup.py runs."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import mixup_cases as mc
import mixup_fixture as fx

OK, ARG, SHAPE, WORKSPACE = 0, -1, -2, -5
P = 4096  # stands for a 16-byte aligned device pointer: every call below is refused before anything is launched or read


@pytest.fixture(scope="module")
def npz(golden_dir):
    return fx.load(golden_dir)


@pytest.fixture(scope="module")
def lib():
    from cyhip import _lib
    return _lib.load()


# ---- 1. the draw ------------------------------------------------------------------------------------------------------
def test_draw_reproduces_the_recorded_one_bit_for_bit(npz):
    from contrastyou.utils.utils import fix_all_seed_within_context
    from semi_seg.hooks.utils import mixup_draw
    for seed in mc.SEEDS:
        for batch in mc.BATCHES:
            for alpha in mc.ALPHAS:
                with fix_all_seed_within_context(seed):
                    lam, index = mixup_draw(batch, alpha)
                ref_lam, ref_index = fx.recorded_draw(npz, seed, batch, alpha)
                assert isinstance(lam, float) and not index.is_cuda and index.dtype == torch.int64
                assert np.float64(lam).tobytes() == np.float64(ref_lam).tobytes(), (seed, batch, alpha)
                assert tuple(index.tolist()) == ref_index, (seed, batch, alpha)
    assert mixup_draw(4, 0)[0] == 1.0  # alpha <= 0: no beta draw
    # what the cases call "a recorded draw"
    assert fx.recorded_draw(npz, 3, 6, 1.0)[1] == (4, 0, 3, 2, 1, 5)
    assert 0.4 < fx.weights_of(npz, mc.DRAW_A1)[0] < 0.5 and 0 < fx.weights_of(npz, mc.DRAW_A02)[0] < 1e-5


def test_draw_leaves_the_generators_as_they_were():
    from contrastyou.utils.utils import fix_all_seed_within_context
    from semi_seg.hooks.utils import mixup_draw
    before = (np.random.get_state()[1].copy(), torch.random.get_rng_state().clone())
    with fix_all_seed_within_context(7):
        mixup_draw(6, 0.2)
    assert (np.random.get_state()[1] == before[0]).all() and torch.equal(torch.random.get_rng_state(), before[1])


# ---- 2. the restatement -----------------------------------------------------------------------------------------------
GOLDEN = [c for c in mc.LOSS_CASES if c.golden]


@pytest.mark.parametrize("case", GOLDEN, ids=lambda c: c.tag)
def test_restatement_agrees_with_the_recorded_f64(npz, case):
    s, t, y, index, (w_self, w_other) = fx.case_inputs(npz, case)
    # the stored inputs are what the case module builds
    assert (npz[f"{case.tag}_s_i8d8"] == mc.logits_i8(case, "s")).all()
    assert (npz[f"{case.tag}_t_i8d8"] == mc.logits_i8(case, "t")).all()
    assert (npz[f"{case.tag}_y"] == mc.labels(case)).all()
    v, g = fx.grad_of(fx.mixkl64, s, y, index, w_self, w_other)
    assert fx.rel_scalar(v, npz[f"{case.tag}_kl64"]) <= 1e-12
    # (the recorded gradients are f64 rounded to f32 for the file's size: 2^-24 relative per element)
    assert max(fx.rel_grad(g, npz[f"{case.tag}_gkl64"])) <= 2.0 ** -24
    v, g = fx.grad_of(fx.mixmse64, s, t, index, w_self, w_other)
    assert fx.rel_scalar(v, npz[f"{case.tag}_mse64"]) <= 1e-12
    assert max(fx.rel_grad(g, npz[f"{case.tag}_gmse64"])) <= 2.0 ** -24


def test_restatement_gradients_against_autograd_through_the_one_hot_form(npz):
    """to 1e-12, in f64 end to end: the two-label closed form against KL_div's expression on the mixed one-hot"""
    for case in GOLDEN:
        s, _, y, index, (w_self, w_other) = fx.case_inputs(npz, case)
        ws, wo = np.float32(w_self), np.float32(w_other)
        oh = torch.nn.functional.one_hot(y, case.K).movedim(-1, 1).float()
        target = (float(ws) * oh + float(wo) * oh[index]).double()  # f32, as the reference forms it

        def onehot_form(z):
            p = torch.softmax(z, 1)
            return (-target * torch.log((p + fx.EPS) / (target + fx.EPS))).sum(1).mean()

        v1, g1 = fx.grad_of(onehot_form, s)
        v2, g2 = fx.grad_of(fx.mixkl64, s, y, index, w_self, w_other)
        assert fx.rel_scalar(v2, v1) <= 1e-12 and max(fx.rel_grad(g2, g1)) <= 1e-12, case.tag


def test_restatement_edge_semantics(npz):
    case = mc.LOSS_BY_TAG["k5_5x7_oob"]
    s, _, y, index, _ = fx.case_inputs(npz, case)
    assert int((y == case.K).sum()) > 0 and int(y.max()) == case.K
    # a weight of exactly 0 adds exactly 0: (1, 0) is the plain KL against the own label, whatever the index
    inside = y.clamp(max=case.K - 1)
    plain = -torch.log(torch.softmax(s.double(), 1).gather(1, inside.unsqueeze(1)) + fx.EPS).mean() \
        + np.log(1.0 + fx.EPS)
    assert abs(float(fx.mixkl64(s, inside, index, 1.0, 0.0)) - float(plain)) <= 1e-12 * float(plain)
    # a label equal to K selects no class: finite, and larger than with the label moved inside
    v = fx.mixkl64(s, y, index, 0.5, 0.5)
    assert torch.isfinite(v) and float(v) > float(fx.mixkl64(s, inside, index, 0.5, 0.5))
    assert fx.tolerances(npz).keys() == set(fx.KINDS)
    assert all(1e-6 <= t < 1e-5 for t in fx.tolerances(npz).values())


# ---- 3. names and signatures ------------------------------------------------------------------------------------------
def _names(fn):
    out = []
    for name, p in inspect.signature(fn).parameters.items():
        if name != "self":
            out.append("**" + name if p.kind is p.VAR_KEYWORD else name)
    return " ".join(out)


def test_signatures_equal_the_references(golden_dir):
    from semi_seg.epochers import MixupEpocher
    from semi_seg.hooks import ICTMeanTeacherTrainerHook, MixUpTrainHook
    from semi_seg.hooks.utils import mixup_data
    from semi_seg.trainers import MixUpTrainer
    want = dict(line.split(": ", 1) for line in (golden_dir / "mixup_signatures.txt").read_text().splitlines())
    got = {"mixup_data": _names(mixup_data), "MixUpTrainHook": _names(MixUpTrainHook.__init__),
           "ICTMeanTeacherTrainerHook": _names(ICTMeanTeacherTrainerHook.__init__),
           "MixupEpocher._batch_update": _names(MixupEpocher._batch_update),
           "MixUpTrainer": _names(MixUpTrainer.__init__)}
    assert got == want
    sig = inspect.signature(mixup_data)
    assert sig.parameters["alpha"].default == 1.0 and sig.parameters["device"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(ICTMeanTeacherTrainerHook.__init__)
    assert [sig.parameters[k].default for k in ("alpha", "weight_decay", "update_bn")] == [0.999, 1e-5, False]
    assert inspect.signature(MixUpTrainHook.__init__).parameters["enable_bn"].default is True


# ---- 4. the class hierarchy ---------------------------------------------------------------------------------------------
def test_class_hierarchy():
    import semi_seg.epochers as epochers
    import semi_seg.hooks as hooks
    import semi_seg.trainers as trainers
    from semi_seg.hooks.mt import _ICTMeanTeacherEpocherHook, _MeanTeacherEpocherHook
    assert issubclass(hooks.ICTMeanTeacherTrainerHook, hooks.MeanTeacherTrainerHook)
    assert issubclass(_ICTMeanTeacherEpocherHook, _MeanTeacherEpocherHook)
    assert _ICTMeanTeacherEpocherHook.MIX_ALPHA == 0.2
    assert issubclass(trainers.MixUpTrainer, trainers.SemiTrainer) and trainers.MixUpTrainer.activate_hooks is True
    assert trainers.MixUpTrainer.train_epocher.fget(None) is epochers.MixupEpocher
    assert issubclass(epochers.MixupEpocher, epochers.SemiSupervisedEpocher)
    from contrastyou.hooks.base import TrainerHook
    assert issubclass(hooks.MixUpTrainHook, TrainerHook)
    # the zoo entry and the factories stay pinned (other tests hold them to NotImplementedError)
    assert trainers.trainer_zoo["mixup"] is not trainers.MixUpTrainer


def test_functions_refuse_cpu_tensors():
    from cyhip import ops
    from cyhip.functions import MixSoftmaxMSEFn, MixupKLFn
    z, y, idx = torch.zeros(2, 3, 4, 4), torch.zeros(2, 4, 4, dtype=torch.int64), torch.tensor([1, 0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MixupKLFn.apply(z, y, idx, 0.5, 0.5, 1e-16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MixSoftmaxMSEFn.apply(z, z, idx, 0.5, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mix_images(z, idx, 0.5, 0.5)
    for bad in (torch.tensor([0, 2]), torch.tensor([-1, 0]), torch.tensor([0, 1, 0])):
        with pytest.raises(ValueError):
            ops.mix_index(bad, 2, "cpu")
    with pytest.raises(TypeError):
        ops.mix_index(torch.tensor([0.0, 1.0]), 2, "cpu")
    assert ops.mix_weights(0.25) == (0.25, 0.75)


# ---- 5. argument checks of the C ABI ----------------------------------------------------------------------------------
ENTRIES = {
    "cy_mix_plan": (C.c_int, 6), "cy_mix_images": (C.c_int, 8),
    "cy_softmax_mixkl_ws_bytes": (C.c_size_t, 2), "cy_softmax_mixkl_fwd": (C.c_int, 13),
    "cy_softmax_mixkl_bwd": (C.c_int, 12), "cy_softmax_mixmse_ws_bytes": (C.c_size_t, 2),
    "cy_softmax_mixmse_fwd": (C.c_int, 12), "cy_softmax_mixmse_bwd": (C.c_int, 11),
}


def test_entries_are_declared_exported_and_typed(lib):
    from cyhip import _lib
    assert lib.cy_abi_version() == 19 == _lib.ABI_VERSION
    for name, (res, nargs) in ENTRIES.items():
        assert name in _lib.exported_names(), name
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs, (name, fn.restype, fn.argtypes)
    assert lib.cy_mix_images.argtypes == [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_long,
                                          C.c_void_p]
    assert (_lib.CY_MIX_IMAGES, _lib.CY_MIX_KL, _lib.CY_MIX_MSE) == (0, 1, 2)
    assert tuple(f for f, _ in _lib.MixPlan._fields_) == ("vec", "kt", "fwd_grid", "fwd_trips", "bwd_grid", "bwd_trips",
                                                          "rows")
    assert len(_lib._STRUCTS) == 27 and _lib._STRUCTS["cy_mix_plan_t"] is _lib.MixPlan  # the plan is a header struct
    assert lib.cy_mix_plan.argtypes[-1] is C.POINTER(_lib.MixPlan)


def _kl(lib, which, N=2, HW=10, K=3, null=None, ws_bytes=1 << 20):
    if which == "fwd":
        ptrs = {"logits": P, "target": P, "index": P, "loss": P, "ws": P}
        if null:
            ptrs[null] = None
        return lib.cy_softmax_mixkl_fwd(ptrs["logits"], ptrs["target"], ptrs["index"], 0.5, 0.5, ptrs["loss"], N, HW, K,
                                        1e-16, ptrs["ws"], ws_bytes, None)
    ptrs = {"logits": P, "target": P, "index": P, "gscale": P, "dlogits": P}
    if null:
        ptrs[null] = None
    return lib.cy_softmax_mixkl_bwd(ptrs["logits"], ptrs["target"], ptrs["index"], 0.5, 0.5, ptrs["gscale"],
                                    ptrs["dlogits"], N, HW, K, 1e-16, None)


def _mse(lib, which, N=2, HW=10, K=3, null=None, ws_bytes=1 << 20):
    if which == "fwd":
        ptrs = {"student": P, "teacher": P, "index": P, "loss": P, "ws": P}
        if null:
            ptrs[null] = None
        return lib.cy_softmax_mixmse_fwd(ptrs["student"], ptrs["teacher"], ptrs["index"], 0.5, 0.5, ptrs["loss"], N, HW,
                                         K, ptrs["ws"], ws_bytes, None)
    ptrs = {"student": P, "teacher": P, "index": P, "gscale": P, "dstudent": P}
    if null:
        ptrs[null] = None
    return lib.cy_softmax_mixmse_bwd(ptrs["student"], ptrs["teacher"], ptrs["index"], 0.5, 0.5, ptrs["gscale"],
                                     ptrs["dstudent"], N, HW, K, None)


@pytest.mark.parametrize("call,fwd_ptrs,bwd_ptrs", [
    (_kl, ("logits", "target", "index", "loss", "ws"), ("logits", "target", "index", "gscale", "dlogits")),
    (_mse, ("student", "teacher", "index", "loss", "ws"), ("student", "teacher", "index", "gscale", "dstudent"))],
    ids=["mixkl", "mixmse"])
def test_losses_reject_with_their_status_before_any_launch(lib, call, fwd_ptrs, bwd_ptrs):
    for null in fwd_ptrs:
        assert call(lib, "fwd", null=null) == ARG, null
    for null in bwd_ptrs:
        assert call(lib, "bwd", null=null) == ARG, null
    for which in ("fwd", "bwd"):
        for N, HW in ((0, 10), (-1, 10), (2, 0), (2, -3)):
            assert call(lib, which, N=N, HW=HW) == ARG, (which, N, HW)
        for K in (1, 0, 17, 64):
            assert call(lib, which, K=K) == SHAPE, (which, K)
    query = lib.cy_softmax_mixkl_ws_bytes if call is _kl else lib.cy_softmax_mixmse_ws_bytes
    for N, HW in ((2, 10), (2, 363 * 363), (6, 361)):
        need = query(N, HW)
        assert need == 8 * min(1024, -(-N * HW // 256))
        assert call(lib, "fwd", N=N, HW=HW, ws_bytes=need - 1) == WORKSPACE
    assert query(0, 10) == 0 and query(2, 0) == 0


def test_images_and_plan_reject_with_their_status(lib):
    img = lib.cy_mix_images
    assert img(None, P, 0.5, 0.5, 2 * P, 2, 4, None) == ARG
    assert img(P, None, 0.5, 0.5, 2 * P, 2, 4, None) == ARG
    assert img(P, P, 0.5, 0.5, None, 2, 4, None) == ARG
    assert img(P, P, 0.5, 0.5, P, 2, 4, None) == ARG  # out must not be x
    assert img(P, P, 0.5, 0.5, 2 * P, 0, 4, None) == ARG and img(P, P, 0.5, 0.5, 2 * P, 2, 0, None) == ARG
    assert img(P + 2, P, 0.5, 0.5, 2 * P, 2, 4, None) == ARG  # not a float's alignment
    from cyhip import _lib
    plan = _lib.MixPlan()
    assert lib.cy_mix_plan(1, 2, 10, 3, 16, None) == ARG
    assert lib.cy_mix_plan(3, 2, 10, 3, 16, plan) == ARG and lib.cy_mix_plan(-1, 2, 10, 3, 16, plan) == ARG
    for form in (0, 1, 2):
        assert lib.cy_mix_plan(form, 0, 10, 3, 16, plan) == ARG and lib.cy_mix_plan(form, 2, 0, 3, 16, plan) == ARG
        assert lib.cy_mix_plan(form, 2, 10, 3, 0, plan) == ARG and lib.cy_mix_plan(form, 2, 10, 3, 2, plan) == ARG
    for form in (1, 2):
        for K in (1, 17):
            assert lib.cy_mix_plan(form, 2, 10, K, 16, plan) == SHAPE
        assert lib.cy_mix_plan(form, 2, 10, 4, 4, plan) == ARG  # K == 4 rows are always read 16 bytes at a time
    assert lib.cy_mix_plan(0, 2, 10, 99, 16, plan) == OK  # images ignore K


# ---- 6. the launch rule and its coverage ----------------------------------------------------------------------------
def test_plan_formulas():
    from cyhip import ops
    for N, HW, K in ((2, 1, 2), (4, 35, 3), (6, 361, 5), (2, 363 * 363, 2), (4, 363 * 363, 2), (3, 70000, 16)):
        for form in ("mixkl", "mixmse"):
            p = ops.mix_plan(form, N, HW, K)
            npix = N * HW
            assert p["fwd_grid"] == min(1024, -(-npix // 256)) and p["bwd_grid"] == 2 * p["fwd_grid"]
            assert p["fwd_trips"] == -(-npix // (256 * p["fwd_grid"]))
            assert p["bwd_trips"] == -(-npix // (256 * p["bwd_grid"]))
            assert p["kt"] == (K if K in (2, 4, 8) else 0) and p["vec"] == {2: 2, 4: 4, 8: 4}.get(K, 1)
            assert p["rows"] == 0
    assert ops.mix_plan("mixkl", 2, 10, 2, align=4)["kt"] == 0 and ops.mix_plan("mixmse", 2, 10, 8, align=8)["kt"] == 0
    assert ops.mix_plan("mixkl", 2, 10, 2, align=8)["kt"] == 2
    for N, E, align in ((2, 1, 16), (4, 35, 16), (4, 1444, 16), (2, 1444, 4), (3, 1048580, 16), (2, 349527, 16),
                        (2000, 64, 16)):
        p = ops.mix_plan("images", N, E, align=align)
        vec = 4 if E % 4 == 0 and align % 16 == 0 else 1
        rows = min(N, 1024)
        cols = min(-(-(E // vec) // 256), 2048 // rows)
        assert (p["vec"], p["rows"], p["fwd_grid"]) == (vec, rows, rows * cols)
        assert p["fwd_trips"] == -(-(E // vec) // (256 * cols)) * -(-N // rows)
        assert p["fwd_grid"] <= 2048 and (p["bwd_grid"], p["bwd_trips"], p["kt"]) == (0, 0, 0)


def test_every_variant_and_every_capped_loop_has_a_parity_case():
    from cyhip import ops
    for form in ("mixkl", "mixmse"):
        plans = {c.tag: ops.mix_plan(form, c.N, c.H * c.W, c.K) for c in mc.LOSS_CASES}
        assert {p["kt"] for p in plans.values()} == {0, 2, 4, 8}  # every kernel the plan can select
        assert {c.K for c in mc.LOSS_CASES if plans[c.tag]["kt"] == 0} >= {3, 5, 16}
        assert plans["k2_363_swap"]["fwd_trips"] == 2 and plans["k2_363_swap"]["bwd_trips"] == 1
        assert plans["k2_363_repeat"]["fwd_trips"] == 3 and plans["k2_363_repeat"]["bwd_trips"] == 2
        assert any(p["fwd_grid"] > 1 and p["fwd_trips"] == 1 for p in plans.values())  # more than one block
        assert any(p["fwd_grid"] == 1 for p in plans.values())
        # (a compiled K on a base that is only 4-byte aligned takes the run-time kernel: test_gpu_mixup runs K = 2
        # and K = 8 on such a base)
    plans = {c.tag: ops.mix_plan("images", c.N, c.E, align=16 if c.base == "aligned" else 4) for c in mc.IMAGE_CASES}
    assert {p["vec"] for p in plans.values()} == {1, 4}
    assert plans["e1444"]["vec"] == 4 and plans["e1444_slice"]["vec"] == 1 and plans["e1083"]["vec"] == 1
    for tag, vec in (("vec_past_cap", 4), ("scalar_past_cap", 1)):  # the capped loop, in both forms
        assert plans[tag]["vec"] == vec and plans[tag]["fwd_trips"] == 2, (tag, plans[tag])
    assert all(p["fwd_trips"] == 1 for t, p in plans.items() if not t.endswith("past_cap"))
    assert {c.E for c in mc.IMAGE_CASES} >= {1, 35, 4 * 19 * 19, 3 * 19 * 19}
