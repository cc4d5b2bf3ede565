"""Host-side contract of the DAE prior and the orthogonal-prototype regulariser (no kernel runs, no GPU): the classes,
their parameter lists and state-dict keys against the reference's recorded ones (tests/golden/prior.npz, written by
tests/golden/gen_goldens_prior.py), the float64 restatement against the reference's recorded f32 values, the C ABI's
argument checks, and the launch rule's coverage: every kernel variant, chunk count and capped loop `ops.prior_plan` can
report is reached by a case of tests/prior_cases.py, which tests/test_gpu_prior.py runs."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import prior_cases as pc

OK, ARG, SHAPE, WORKSPACE = 0, -1, -2, -5
P = 4096  # stands for a 16-byte aligned device pointer: every call below is refused before anything is launched or read


@pytest.fixture(scope="module")
def npz(golden_dir):
    return pc.load(golden_dir)


@pytest.fixture(scope="module")
def lib():
    from cyhip import _lib
    return _lib.load()


def _names(fn):
    out = []
    for name, p in inspect.signature(fn).parameters.items():
        if name != "self":
            out.append("**" + name if p.kind is p.VAR_KEYWORD else "*" + name if p.kind is p.VAR_POSITIONAL else name)
    return out


# ---- 1. classes, parameter lists, state dicts ---------------------------------------------------------------------------
def test_classes_have_the_references_parameter_lists():
    from contrastyou.hooks.base import EpocherHook, TrainerHook
    from semi_seg.hooks import AuxiliaryLayer, DenoisingAutoEncoderTrainerHook, OrthogonalTrainerHook
    from semi_seg.hooks.autoencoder import DenoisingAutoEncoderEpocherHook
    from semi_seg.hooks.orthogonal import _OrthogonalEpocherHook, normalize, pairwise_matrix
    assert _names(AuxiliaryLayer.__init__) == ["in_features", "out_features", "activation"]
    sig = inspect.signature(AuxiliaryLayer.__init__)
    assert (sig.parameters["out_features"].default, sig.parameters["activation"].default) == (1, "sigmoid")
    assert all(p.kind is p.KEYWORD_ONLY for n, p in sig.parameters.items() if n != "self")
    assert _names(DenoisingAutoEncoderTrainerHook.__init__) == ["hook_name", "num_classes", "weight", "**kwargs"]
    sig = inspect.signature(DenoisingAutoEncoderTrainerHook.__init__)
    assert (sig.parameters["hook_name"].default, sig.parameters["weight"].default) == ("deAE", 0.0)
    assert _names(DenoisingAutoEncoderEpocherHook.__init__) == ["name", "extra_layer", "weight"]
    assert inspect.signature(DenoisingAutoEncoderEpocherHook.__init__).parameters["name"].default == "deAE"
    assert _names(DenoisingAutoEncoderEpocherHook._call_implementation) == \
        ["unlabeled_image_tf", "unlabeled_tf_logits", "**kwargs"]
    assert _names(OrthogonalTrainerHook.__init__) == ["hook_name", "prototypes", "weight"]
    assert inspect.signature(OrthogonalTrainerHook.__init__).parameters["weight"].default == 0.0
    assert _names(_OrthogonalEpocherHook.__init__) == ["name", "prototypes", "weight"]
    assert _names(_OrthogonalEpocherHook._call_implementation) == ["**kwargs"]
    assert issubclass(DenoisingAutoEncoderTrainerHook, TrainerHook) and issubclass(OrthogonalTrainerHook, TrainerHook)
    assert issubclass(DenoisingAutoEncoderEpocherHook, EpocherHook) and issubclass(_OrthogonalEpocherHook, EpocherHook)
    # the two plain torch helpers
    a = torch.arange(6.0).view(2, 3)
    assert torch.equal(pairwise_matrix(a, a), a @ a.t())
    assert torch.allclose(normalize(a + 1).norm(dim=1), torch.ones(2))
    with pytest.raises(AssertionError):
        pairwise_matrix(a, a.t())
    with pytest.raises(AssertionError):
        AuxiliaryLayer(in_features=4, activation="relu")


def test_auxiliary_layer_initialises_as_the_reference_does(npz):
    from semi_seg.hooks import AuxiliaryLayer
    for K, seed in pc.AUX_INIT:
        torch.manual_seed(seed)
        layer = AuxiliaryLayer(in_features=K)
        sd = layer.state_dict()
        assert sorted(sd) == ["fc.bias", "fc.weight"]
        assert sd["fc.weight"].shape == (1, K, 1, 1) and sd["fc.bias"].shape == (1,)
        assert np.array_equal(sd["fc.weight"].numpy(), npz[f"aux_k{K}_weight"]), K
        assert np.array_equal(sd["fc.bias"].numpy(), npz[f"aux_k{K}_bias"]), K
    assert isinstance(AuxiliaryLayer(in_features=3, activation="tanh").activation, torch.nn.Tanh)


class _Meters(dict):
    def register_meter(self, name, meter):
        self[name] = meter

    def focus_on(self, name):
        from contextlib import nullcontext
        return nullcontext()


class _Epocher:
    def __init__(self):
        self.meters = _Meters()


def test_hooks_modules_meters_and_the_name_quirk():
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.meters import AverageValueMeter
    from semi_seg.hooks import AuxiliaryLayer, DenoisingAutoEncoderTrainerHook, OrthogonalTrainerHook
    from semi_seg.hooks.autoencoder import DenoisingAutoEncoderEpocherHook
    type(TrainerHook).names.clear()
    try:
        hook = DenoisingAutoEncoderTrainerHook(hook_name="my_prior", num_classes=4, weight=0.25, ignored="x")
        assert hook.learnable_modules == [hook.aux_layer] and isinstance(hook.aux_layer, AuxiliaryLayer)
        assert [tuple(p.shape) for p in hook.parameters()] == [(1, 4, 1, 1), (1,)]
        assert sorted(hook.state_dict()["module_state"]) == ["aux_layer.fc.bias", "aux_layer.fc.weight"]  # checkpointed
        ep_hook = hook()
        assert ep_hook.name == "deAE" and ep_hook._weight == 0.25 and ep_hook.layer is hook.aux_layer
        ep = _Epocher()
        ep_hook.epocher = ep
        assert list(ep.meters) == ["ls"] and isinstance(ep.meters["ls"], AverageValueMeter)
        with pytest.raises(ValueError, match="out_features must be 1"):
            DenoisingAutoEncoderEpocherHook(extra_layer=AuxiliaryLayer(in_features=4, out_features=2), weight=1.0)

        proto = torch.nn.Parameter(torch.randn(4, 16, 1, 1))
        hook = OrthogonalTrainerHook(hook_name="orth", prototypes=proto, weight=0.5)
        assert hook.learnable_modules == [] and list(hook.parameters()) == []
        ep_hook = hook()
        assert ep_hook.name == "orth" and ep_hook._prototypes is proto and ep_hook._weight == 0.5
        ep = _Epocher()
        ep_hook.epocher = ep
        assert list(ep.meters) == ["loss"] and isinstance(ep.meters["loss"], AverageValueMeter)
    finally:
        type(TrainerHook).names.clear()


def test_the_two_factories_still_raise():
    from semi_seg.hooks import create_dae_hook, create_orthogonal_hook
    with pytest.raises(NotImplementedError):
        create_dae_hook(weight=0.1, num_classes=4)
    with pytest.raises(NotImplementedError):
        create_orthogonal_hook(weight=0.1, model=torch.nn.Identity())


def test_functions_refuse_cpu_tensors_and_bad_arguments():
    from cyhip.functions import DAELossFn, OrthoLossFn
    z, w, b, img = torch.zeros(1, 3, 2, 2), torch.zeros(1, 3, 1, 1), torch.zeros(1), torch.zeros(1, 1, 2, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DAELossFn.apply(z, w, b, img, "sigmoid")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OrthoLossFn.apply(torch.zeros(3, 4))


# ---- 2. the restatement against the reference's recorded values ---------------------------------------------------------
def test_restatement_agrees_with_the_recorded_hooks(npz):
    """f64 against the reference's f32: 1e-5 holds them together and tells every formula apart from a wrong one"""
    for h in pc.HOOK_DAE:
        tag, K = h["tag"], h["K"]
        z = torch.from_numpy(npz[f"{tag}_z_i8d8"].astype(np.float32) / 8)
        w, b = torch.from_numpy(npz[f"aux_k{K}_weight"]), torch.from_numpy(npz[f"aux_k{K}_bias"])
        img = torch.from_numpy(npz[f"{tag}_image"])
        assert z.shape == (h["N"], K, h["H"], h["W"]) and img.shape == (h["N"], h["Cimg"], h["H"], h["W"])
        v, g = pc.grads_of(lambda a, c, d, e: h["weight"] * pc.dae64(a, c, d, e, "sigmoid"), z, w, b, img, wrt=(0, 1, 2))
        assert pc.rel_scalar(npz[f"{tag}_value"], v) <= 1e-5
        assert pc.rel_scalar(npz[f"{tag}_meter"][0], v / h["weight"]) <= 1e-5
        for name, g64 in zip(("logits", "weight", "bias"), g):
            assert max(pc.rel_grad(torch.from_numpy(npz[f"{tag}_g_{name}"]), g64)) <= 1e-5, (tag, name)
    for h in pc.HOOK_ORTHO:
        tag = h["tag"]
        p = torch.from_numpy(npz[f"{tag}_v"])
        assert p.shape == (h["K"], h["C"], 1, 1)
        v, g = pc.grads_of(lambda a: h["weight"] * pc.ortho64(a), p, wrt=(0,))
        assert pc.rel_scalar(npz[f"{tag}_value"], v) <= 1e-5
        assert max(pc.rel_grad(torch.from_numpy(npz[f"{tag}_g_v"]), g[0])) <= 1e-5, tag


def test_restatement_tells_a_wrong_formula_apart():
    case = pc.DAE_BY_TAG["k3_70_c3"]
    z, w, b, img = pc.dae_inputs(case)
    v = float(pc.dae64(z, w, b, img, case.act))
    assert abs(float(pc.dae64(z, w, b, img, "sigmoid")) - v) > 1e-3 * v                # the other activation
    assert abs(float(pc.dae64(z, w, b, img[:, :1], case.act)) - v) > 1e-3 * v          # one image channel only
    assert float(pc.dae_inputs(pc.DAE_BY_TAG["k4_70_sat"])[0].abs().max()) <= 6.0      # logits stay on the int8 grid
    zz, ww, bb, _ = pc.dae_inputs(pc.DAE_BY_TAG["k4_70_sat"])
    pre = bb.double() + torch.einsum("nkhw,k->nhw", zz.double(), ww.double())
    assert 29.9 < float(pre.abs().max()) < 30.1
    zero = pc.ortho_inputs(pc.ORTHO_BY_TAG["k4_c16_zero"])
    assert float(zero[1].abs().max()) == 0.0 and torch.isfinite(pc.ortho64(zero))
    assert float(pc.ortho64(torch.eye(4))) == 0.0 and abs(float(pc.ortho64(torch.ones(2, 3))) - 0.5) < 1e-15


# ---- 3. the C ABI -----------------------------------------------------------------------------------------------------
ENTRIES = {"cy_prior_plan": (C.c_int, 6), "cy_dae_ws_bytes": (C.c_size_t, 3), "cy_dae_fwd": (C.c_int, 13),
           "cy_dae_bwd": (C.c_int, 16), "cy_ortho_fwd": (C.c_int, 5), "cy_ortho_bwd": (C.c_int, 6)}


def test_entries_are_declared_exported_and_typed(lib):
    from cyhip import _lib, ops
    assert lib.cy_abi_version() == 19 == _lib.ABI_VERSION
    for name, (res, nargs) in ENTRIES.items():
        assert name in _lib.exported_names(), name
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs, (name, fn.restype, fn.argtypes)
    assert (_lib.CY_PRIOR_DAE, _lib.CY_PRIOR_ORTHO, _lib.CY_PRIOR_ACT_SIGMOID, _lib.CY_PRIOR_ACT_TANH) == (0, 1, 0, 1)
    assert ops.PRIOR_ACTS == {"sigmoid": 0, "tanh": 1}
    assert tuple(f for f, _ in _lib.PriorPlan._fields_) == ("variant", "vec", "fwd_grid", "fwd_trips", "bwd_grid",
                                                            "bwd_trips", "k_chunks", "fwd_lds", "bwd_lds", "aux")
    assert len(_lib._STRUCTS) == 27 and _lib._STRUCTS["cy_prior_plan_t"] is _lib.PriorPlan  # the plan is a header struct
    assert lib.cy_prior_plan.argtypes[-1] is C.POINTER(_lib.PriorPlan)


def _dae(lib, which, N=2, HW=35, K=3, Cimg=1, act=0, null=None, ws_bytes=1 << 20):
    if which == "fwd":
        ptrs = {"logits": P, "w": P, "b": P, "image": P, "loss": P, "ws": P}
        if null:
            ptrs[null] = None
        return lib.cy_dae_fwd(ptrs["logits"], ptrs["w"], ptrs["b"], ptrs["image"], ptrs["loss"], N, HW, K, Cimg, act,
                              ptrs["ws"], ws_bytes, None)
    ptrs = {"logits": P, "w": P, "b": P, "image": P, "gscale": P, "dlogits": P, "dw": P, "db": P, "ws": P}
    if null:
        ptrs[null] = None
    return lib.cy_dae_bwd(ptrs["logits"], ptrs["w"], ptrs["b"], ptrs["image"], ptrs["gscale"], ptrs["dlogits"],
                          ptrs["dw"], ptrs["db"], N, HW, K, Cimg, act, ptrs["ws"], ws_bytes, None)


def test_dae_rejects_with_its_status_before_any_launch(lib):
    for null in ("logits", "w", "b", "image", "loss", "ws"):
        assert _dae(lib, "fwd", null=null) == ARG, null
    for null in ("logits", "w", "b", "image", "gscale", "dlogits", "dw", "db", "ws"):
        assert _dae(lib, "bwd", null=null) == ARG, null
    for which in ("fwd", "bwd"):
        for N, HW in ((0, 10), (-1, 10), (2, 0), (2, -3)):
            assert _dae(lib, which, N=N, HW=HW) == ARG, (which, N, HW)
        for K in (1, 65, 0, -2):
            assert _dae(lib, which, K=K) == SHAPE, (which, K)
        for Cimg in (0, 5):
            assert _dae(lib, which, Cimg=Cimg) == SHAPE, (which, Cimg)
        for act in (2, -1):
            assert _dae(lib, which, act=act) == SHAPE, (which, act)
        for K in (2, 64):
            for Cimg in (1, 4):
                for act in (0, 1):  # the edges of the ranges are inside: only the workspace is then wrong
                    assert _dae(lib, which, K=K, Cimg=Cimg, act=act, ws_bytes=0) == WORKSPACE
    for N, HW, K in ((2, 35, 3), (1, 513 * 512, 2), (6, 361, 64)):
        blocks = min(1024, -(-N * HW // 256))
        assert lib.cy_dae_ws_bytes(N * HW, K, 0) == 8 * blocks
        assert lib.cy_dae_ws_bytes(N * HW, K, 1) == 8 * blocks * (K + 1)
        assert _dae(lib, "fwd", N=N, HW=HW, K=K, ws_bytes=8 * blocks - 1) == WORKSPACE
        assert _dae(lib, "bwd", N=N, HW=HW, K=K, ws_bytes=8 * blocks * (K + 1) - 1) == WORKSPACE
    assert lib.cy_dae_ws_bytes(0, 3, 0) == 0 and lib.cy_dae_ws_bytes(0, 3, 1) == 0
    # a base that is not a float's alignment
    assert lib.cy_dae_fwd(P + 2, P, P, P, P, 2, 35, 3, 1, 0, P, 1 << 20, None) == ARG


def test_ortho_and_plan_reject_with_their_status(lib):
    assert lib.cy_ortho_fwd(None, P, 4, 16, None) == ARG and lib.cy_ortho_fwd(P, None, 4, 16, None) == ARG
    for null in range(3):
        ptrs = [P, P, P]
        ptrs[null] = None
        assert lib.cy_ortho_bwd(*ptrs, 4, 16, None) == ARG
    for K, Cc in ((1, 16), (65, 16), (0, 16)):
        assert lib.cy_ortho_fwd(P, P, K, Cc, None) == SHAPE and lib.cy_ortho_bwd(P, P, P, K, Cc, None) == SHAPE
    # K * C = 16385 = 5 * 3277, one past the limit, and the next products past it at the ends of K's range
    assert 5 * 3277 == 16385
    for K, Cc in ((5, 3277), (64, 257), (2, 8193)):
        assert lib.cy_ortho_fwd(P, P, K, Cc, None) == SHAPE and lib.cy_ortho_bwd(P, P, P, K, Cc, None) == SHAPE
    assert lib.cy_ortho_fwd(P, P, 4, 0, None) == ARG and lib.cy_ortho_bwd(P, P, P, 4, -1, None) == ARG
    assert lib.cy_ortho_fwd(P + 2, P, 4, 16, None) == ARG
    from cyhip import _lib
    plan = _lib.PriorPlan()
    assert lib.cy_prior_plan(0, 70, 3, 1, 16, None) == ARG
    assert lib.cy_prior_plan(2, 70, 3, 1, 16, plan) == ARG and lib.cy_prior_plan(-1, 70, 3, 1, 16, plan) == ARG
    assert lib.cy_prior_plan(0, 0, 3, 1, 16, plan) == ARG and lib.cy_prior_plan(0, 70, 3, 1, 2, plan) == ARG
    assert lib.cy_prior_plan(0, 70, 3, 1, 0, plan) == ARG
    for K in (1, 65):
        assert lib.cy_prior_plan(0, 70, K, 1, 16, plan) == SHAPE and lib.cy_prior_plan(1, 0, K, 16, 16, plan) == SHAPE
    for Cimg in (0, 5):
        assert lib.cy_prior_plan(0, 70, 3, Cimg, 16, plan) == SHAPE
    assert lib.cy_prior_plan(1, 0, 64, 257, 16, plan) == SHAPE and lib.cy_prior_plan(1, 0, 64, 256, 16, plan) == OK
    assert lib.cy_prior_plan(1, 0, 4, 0, 16, plan) == ARG
    assert lib.cy_prior_plan(0, 70, 2, 1, 16, plan) == OK and lib.cy_prior_plan(0, 70, 64, 4, 4, plan) == OK


# ---- 4. the launch rule and its coverage ------------------------------------------------------------------------------
def test_plan_formulas_for_every_form():
    from cyhip import _lib, ops
    for npix, K in ((1, 2), (70, 3), (257, 64), (513 * 512, 2), (3 * 1024 * 256 + 1, 17)):
        for align in (16, 8, 4):
            p = ops.prior_plan("dae", K, 1, npix, align=align)
            blocks = min(1024, -(-npix // 256))
            assert p["fwd_grid"] == p["bwd_grid"] == blocks
            assert p["fwd_trips"] == p["bwd_trips"] == -(-npix // (256 * blocks))
            assert p["aux"] == 256 // K * K and (p["fwd_lds"], p["bwd_lds"]) == (2304, 3328)
            assert p["variant"] in (0, 2, 4, 8) and (p["variant"] == 0 or p["variant"] == K)
            assert p["k_chunks"] == (1 if p["variant"] else -(-K // 16))
            if align == 4:
                assert (p["variant"], p["vec"]) == (0, 1)
            if p["vec"] == 4:
                assert K % 4 == 0 and align == 16
            if p["vec"] == 2:
                assert K == 2 and align % 8 == 0
    for K, Cc in ((2, 1), (4, 16), (64, 16), (64, 64), (64, 256), (3, 5461), (17, 65)):
        p = ops.prior_plan("ortho", K, Cc)
        wave = p["variant"]
        assert wave in (0, 1) and p["fwd_grid"] == p["bwd_grid"] == 1 and p["k_chunks"] == 0 and p["vec"] == 1
        assert p["fwd_trips"] == (-(-K * K // 4) if wave else -(-K * K // 256)) and p["bwd_trips"] == -(-K * Cc // 256)
        assert p["aux"] == (Cc if wave else Cc | 1)
        assert p["fwd_lds"] == 4 * K * p["aux"] and p["bwd_lds"] == p["fwd_lds"] + 4 * K * K
        assert p["bwd_lds"] <= 80 * 1024
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_SHAPE"):
        ops.prior_plan("ortho", 64, 257)
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_SHAPE"):
        ops.prior_plan("dae", 65, 1, 70)


def _dae_plan(case):
    from cyhip import ops
    return ops.prior_plan("dae", case.K, case.Cimg, case.N * case.H * case.W, align=4 if case.layout == "slice" else 16)


def test_every_variant_chunk_count_and_capped_loop_has_a_parity_case():
    """reads the plan: which K takes which variant is the launch rule's business, not this test's"""
    from cyhip import ops
    plans = {c.tag: _dae_plan(c) for c in pc.DAE_CASES}
    # every (variant, vec) the rule can return for any K, any alignment
    possible = {(p["variant"], p["vec"]) for K in range(2, 65) for align in (4, 8, 16)
                for p in [ops.prior_plan("dae", K, 1, 70, align=align)]}
    assert {(p["variant"], p["vec"]) for p in plans.values()} == possible
    possible_chunks = {ops.prior_plan("dae", K, 1, 70, align=a)["k_chunks"] for K in range(2, 65) for a in (4, 16)}
    assert {p["k_chunks"] for p in plans.values()} == possible_chunks and len(possible_chunks) >= 4
    # the flat sweep of the backward with idle threads (256 is no multiple of K) and without
    assert {p["aux"] == 256 for p in plans.values()} == {True, False}
    assert {c.act for c in pc.DAE_CASES} == {"sigmoid", "tanh"}
    assert {c.Cimg for c in pc.DAE_CASES} == {1, 2, 3, 4}
    assert {c.layout for c in pc.DAE_CASES} == {"nchw", "cl", "slice"}
    npix = {c.tag: c.N * c.H * c.W for c in pc.DAE_CASES}
    assert 1 in npix.values()                                                         # a one-pixel problem
    assert any(n % 256 not in (0, 1) and plans[t]["fwd_grid"] == 1 for t, n in npix.items())  # a partial only block
    assert any(n % 256 == 1 and plans[t]["fwd_grid"] > 1 for t, n in npix.items())    # a one-pixel last block
    assert any(c.N > 1 and plans[c.tag]["fwd_grid"] == 1 for c in pc.DAE_CASES)       # two images in one block
    past = plans["k2_past_cap"]
    assert past["fwd_trips"] >= 2 and past["bwd_trips"] >= 2 and npix["k2_past_cap"] % 256 == 0
    assert npix["k2_past_cap"] == 256 * (past["fwd_grid"] + 2)  # the second trip is a partial one: two blocks of 1024
    assert all(p["fwd_trips"] == 1 and p["bwd_trips"] == 1 for t, p in plans.items() if t != "k2_past_cap")
    assert any(c.reach >= 30 for c in pc.DAE_CASES)

    plans = {c.tag: ops.prior_plan("ortho", c.K, c.C) for c in pc.ORTHO_CASES}
    assert {p["variant"] for p in plans.values()} == {0, 1}
    for wave in (0, 1):  # at least two trips of the Gram loop and of the sweeps, and a single one, in each form
        mine = [p for p in plans.values() if p["variant"] == wave]
        assert any(p["fwd_trips"] >= 2 for p in mine) and any(p["bwd_trips"] >= 2 for p in mine), wave
    assert any(p["fwd_trips"] == 1 and p["bwd_trips"] == 1 for p in plans.values())
    assert {c.rank for c in pc.ORTHO_CASES} == {2, 4} and any(c.zero for c in pc.ORTHO_CASES)
    assert {(c.K, c.C) for c in pc.ORTHO_CASES} >= {(2, 1), (4, 16), (12, 16), (64, 16), (64, 256), (3, 5461)}
    assert max(p["bwd_lds"] for p in plans.values()) == 80 * 1024  # the largest LDS request the rule can make


def test_bounds_come_from_the_references_own_error():
    """the rule, on the two smallest cases (the GPU tests evaluate it over all of them)"""
    refs = [pc.dae_reference(pc.DAE_BY_TAG[t]) for t in ("k3_70_c3", "k4_70_cl")]
    b = pc.bounds(refs)
    assert set(b) == set(pc.KINDS)
    for kind, (e_ref, bound) in b.items():
        assert 0 <= e_ref < 1e-5 and bound >= 4 * e_ref
        assert bound == (max(4 * e_ref, 1.2e-6) if kind == "loss" else 4 * e_ref)
    v64, g64, e = pc.ortho_reference(pc.ORTHO_BY_TAG["k4_c16_zero"])
    assert g64 is None and torch.isfinite(v64) and e[1:] == [0.0, 0.0]
