"""Host-side checks of the entropy-minimisation, pseudo-label and UA-MT baselines (no GPU): the new entry points of
csrc/cy_pixel_reg.hip refuse bad arguments before any launch, every hook factory the reference's hook_creator.py
imports exists, the seven methods that are not built raise NotImplementedError, the factories take the reference's yaml
keys, and the UA-MT threshold arithmetic.  No kernel runs here."""
import ctypes
import inspect
import math

import pytest

ARG, WS = -1, -5
ENTRIES = ("softmax_entropy", "softmax_selfmse", "uamt_mse")


@pytest.fixture(scope="module")
def lib():
    from cyhip import _lib
    return _lib.load()


def _calls(lib, p, npix, K, big):
    """every new launching entry with host pointers `p` (no launch may ever see them) -> [(name, status)]"""
    return [
        ("entropy_fwd", lib.cy_softmax_entropy_fwd(p, p, npix, K, 1e-16, p, big, None)),
        ("entropy_bwd", lib.cy_softmax_entropy_bwd(p, p, p, npix, K, 1e-16, None)),
        ("selfmse_fwd", lib.cy_softmax_selfmse_fwd(p, p, npix, K, p, big, None)),
        ("selfmse_bwd", lib.cy_softmax_selfmse_bwd(p, p, p, npix, K, None)),
        ("uamt_fwd", lib.cy_uamt_mse_fwd(p, p, p, npix, K, 1.0, 0, p, big, None)),
        ("uamt_bwd", lib.cy_uamt_mse_bwd(p, p, p, p, p, npix, K, 1.0, 0, None)),
    ]


def test_library_exports_the_new_entries(lib):
    from cyhip import _lib
    assert lib.cy_abi_version() == _lib.ABI_VERSION
    for e in ENTRIES:
        for suffix in ("ws_bytes", "fwd", "bwd"):
            name = f"cy_{e}_{suffix}"
            assert hasattr(lib, name) and name in _lib.exported_names(), name


def test_new_entry_points_check_arguments_before_launching(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    big = 1 << 20
    for K in (1, 17, 0, -4):
        for name, rc in _calls(lib, p, 286, K, big):
            assert rc == ARG, (name, K, rc)
    for npix in (0, -1):
        for name, rc in _calls(lib, p, npix, 4, big):
            assert rc == ARG, (name, npix, rc)
    # every pointer in turn NULL
    assert lib.cy_softmax_entropy_fwd(None, p, 286, 4, 1e-16, p, big, None) == ARG
    assert lib.cy_softmax_entropy_fwd(p, None, 286, 4, 1e-16, p, big, None) == ARG
    assert lib.cy_softmax_entropy_fwd(p, p, 286, 4, 1e-16, None, big, None) == ARG
    assert lib.cy_softmax_entropy_bwd(None, p, p, 286, 4, 1e-16, None) == ARG
    assert lib.cy_softmax_entropy_bwd(p, None, p, 286, 4, 1e-16, None) == ARG
    assert lib.cy_softmax_entropy_bwd(p, p, None, 286, 4, 1e-16, None) == ARG
    assert lib.cy_softmax_selfmse_fwd(None, p, 286, 4, p, big, None) == ARG
    assert lib.cy_softmax_selfmse_fwd(p, None, 286, 4, p, big, None) == ARG
    assert lib.cy_softmax_selfmse_fwd(p, p, 286, 4, None, big, None) == ARG
    assert lib.cy_softmax_selfmse_bwd(None, p, p, 286, 4, None) == ARG
    assert lib.cy_softmax_selfmse_bwd(p, None, p, 286, 4, None) == ARG
    assert lib.cy_softmax_selfmse_bwd(p, p, None, 286, 4, None) == ARG
    for i in (0, 1, 2, 5):
        args = [p, p, p, 286, 4, 1.0, 0, p, big, None]
        args[i if i < 3 else 7] = None
        assert lib.cy_uamt_mse_fwd(*args) == ARG, i
    for i in range(5):
        args = [p, p, p, p, p, 286, 4, 1.0, 0, None]
        args[i] = None
        assert lib.cy_uamt_mse_bwd(*args) == ARG, i
    # a short workspace
    assert lib.cy_softmax_entropy_fwd(p, p, 286, 4, 1e-16, p, 15, None) == WS
    assert lib.cy_softmax_selfmse_fwd(p, p, 286, 4, p, 15, None) == WS
    assert lib.cy_uamt_mse_fwd(p, p, p, 286, 4, 1.0, 0, p, 31, None) == WS


def test_wrapper_raises_on_a_refused_call():
    from cyhip import _lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_ARG"):
        _lib.call("cy_softmax_entropy_fwd", p, p, 286, 17, 1e-16, p, 1 << 20, None)


@pytest.mark.parametrize("npix", [1, 255, 256, 257, 286, 270000, 16 * 224 * 224, 1 << 31])
def test_workspace_sizes(lib, npix):
    """one f64 partial per block of 256 pixels, at most 1024 blocks (the head's loss kernels' grid); two for UA-MT"""
    blocks = min(max((npix + 255) // 256, 1), 1024)
    assert lib.cy_softmax_entropy_ws_bytes(npix) == blocks * 8
    assert lib.cy_softmax_selfmse_ws_bytes(npix) == blocks * 8
    assert lib.cy_uamt_mse_ws_bytes(npix) == blocks * 16
    assert lib.cy_softmax_mse_ws_bytes(npix) == blocks * 8  # the shared cy_blocks(npix, 256, LOSS_GRID_CAP)


def test_every_factory_of_the_reference_hook_creator_is_importable(golden_dir):
    import semi_seg.hooks as hooks
    names = (golden_dir / "hook_factory_names.txt").read_text().split()
    assert len(names) == 18 and "create_uamt_hook" in names and "create_infonce_hooks" in names
    missing = [n for n in names if not callable(getattr(hooks, n, None))]
    assert not missing, missing


STUBS = {
    "create_differentiable_mt_hook": dict(model=None, weight=1.0, alpha=0.999, weight_decay=1e-6, meta_weight=0,
                                          meta_criterion="ce", method_name="method1"),
    "create_orthogonal_hook": dict(weight=0.001, model=None),
    "create_imsat_hook": dict(weight=0.1),
    "create_intermediate_imsat_hook": dict(feature_name="Conv5", weight=0.1, num_clusters=10, cons_weight=0.1,
                                           model=None),
    "create_mixup_hook": dict(weight=0.1, enable_bn=True),
    "create_ict_hook": dict(weight=0.1, alpha=0.999, weight_decay=1e-6, update_bn=False, model=None),
    "create_dae_hook": dict(weight=0.1, num_classes=4),
}


@pytest.mark.parametrize("name", sorted(STUBS))
def test_methods_that_are_not_built_say_so(name):
    import semi_seg.hooks as hooks
    fn = getattr(hooks, name)
    params = inspect.signature(fn).parameters
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params.values()), name
    assert set(STUBS[name]) == set(params), (name, list(params))
    with pytest.raises(NotImplementedError, match=name):
        fn(**STUBS[name])
    with pytest.raises(TypeError):
        fn(**STUBS[name], no_such_keyword=1)


def test_factories_take_the_reference_yaml_keys():
    """config/hooks/mt.yaml, uamt.yaml, entmin.yaml, pseudolabel.yaml, iid.yaml: signatures only, no model forward"""
    import semi_seg.hooks as hooks
    yaml_keys = dict(weight=10, alpha=0.99, weight_decay=0.000001, update_bn=False, num_teachers=1, hard_clip=False)
    for name in ("create_mt_hook", "create_uamt_hook"):
        sig = inspect.signature(getattr(hooks, name))
        assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in sig.parameters.values()), name
        sig.bind(model=object(), **yaml_keys)
        assert set(sig.parameters) == {"model", *yaml_keys}, name
    inspect.signature(hooks.create_ent_min_hook).bind(weight=1)
    assert inspect.signature(hooks.create_ent_min_hook).parameters["weight"].default == 0.001
    inspect.signature(hooks.create_pseudo_label_hook).bind(weight=0.1)
    with pytest.raises(TypeError):
        inspect.signature(hooks.create_pseudo_label_hook).bind()
    inspect.signature(hooks.create_iid_seg_hook).bind(weight=0.1, mi_lambda=1.0)


def test_hook_classes_and_names():
    from contrastyou.hooks.base import TrainerHook
    from semi_seg.hooks import (EntropyMinTrainerHook, MeanTeacherTrainerHook, PseudoLabelTrainerHook,
                                UAMeanTeacherTrainerHook, create_ent_min_hook, create_iid_seg_hook,
                                create_pseudo_label_hook, mt_in_hooks)
    from semi_seg.hooks.entmin import _EntropyEpocherHook
    from semi_seg.hooks.pseudolabel import _PLEpocherHook
    assert issubclass(UAMeanTeacherTrainerHook, MeanTeacherTrainerHook)  # what mt_in_hooks looks for
    type(TrainerHook).names.clear()
    ent, pl, iid = create_ent_min_hook(weight=1), create_pseudo_label_hook(weight=0.1), create_iid_seg_hook(weight=0.1)
    assert isinstance(ent, EntropyMinTrainerHook) and isinstance(pl, PseudoLabelTrainerHook)
    assert (ent._hook_name, pl._hook_name, iid._hook_name) == ("entropy", "plab", "iid")
    assert isinstance(ent(), _EntropyEpocherHook) and isinstance(pl(), _PLEpocherHook)
    assert list(ent.parameters()) == [] and not mt_in_hooks(ent, pl)
    type(TrainerHook).names.clear()


def test_more_than_one_teacher_is_refused():
    import torch
    from contrastyou.hooks.base import TrainerHook
    from semi_seg.hooks import create_mt_hook, create_uamt_hook, mt_in_hooks
    type(TrainerHook).names.clear()
    net = torch.nn.Conv2d(1, 2, 1)
    for make in (create_mt_hook, create_uamt_hook):
        with pytest.raises(RuntimeError, match="one Teacher"):
            make(model=net, weight=1.0, num_teachers=2)
        type(TrainerHook).names.clear()
    hook = create_uamt_hook(model=net, weight=1.0, num_teachers=1, hard_clip=True)
    assert mt_in_hooks(hook) and hook.teacher_model is not net
    assert all(not p.requires_grad for p in hook.teacher_model.parameters())
    type(TrainerHook).names.clear()


@pytest.mark.parametrize("epoch,factor", [(0, 0.75), (40, 0.85), (100, 1.0)])
def test_uamt_threshold(epoch, factor):
    """thr = (3/4 + 1/4 * cur_epoch / max_epoch) * ln C for C = 4, max_epoch = 100: f64 on the host"""
    from semi_seg.hooks.mt import uamt_threshold
    thr = uamt_threshold(4, epoch, 100)
    assert isinstance(thr, float)
    assert abs(thr - factor * math.log(4)) <= 4 * 2.0 ** -53 * math.log(4)
    assert thr == 3 / 4 * math.log(4) + 1 / 4 * math.log(4) * float(epoch / 100)  # the reference's expression


def test_entropy_from_logits_falls_back_to_the_formula_off_the_mean():
    """reduction "sum" / "none" are the torch formula (runs on the CPU); "mean" is the kernel path: no CPU fallback"""
    import torch
    from contrastyou.losses.kl import Entropy
    z = torch.randn(2, 4, 5, 7)
    for red in ("sum", "none"):
        assert torch.equal(Entropy(reduction=red).from_logits(z), Entropy(reduction=red)(z.softmax(1)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Entropy().from_logits(z)
