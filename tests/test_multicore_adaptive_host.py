"""CPU-side checks of the adaptive over-segmented criteria (contrastyou/losses/multicore_loss.py): the class surface,
the probability-space members on hand values, and the argument checks and workspace rules of the cy_softmax_mix_* /
cy_mix_dice_counts entries (csrc/cy_mix_loss.hip), made without a launch as tests/test_multicore_host.py does."""
import ctypes
import inspect
import math
import re
from pathlib import Path

import pytest
import torch

OK, ERR_ARG, ERR_SHAPE, ERR_WORKSPACE = 0, -1, -2, -5
ENTRIES = ("cy_softmax_mix_kl_ws_bytes", "cy_softmax_mix_kl_fwd", "cy_softmax_mix_kl_bwd_ws_bytes",
           "cy_softmax_mix_kl_bwd", "cy_mix_dice_counts")
EPS = 1e-16


def test_class_surface():
    from contrastyou.losses import multicore_loss as ml
    from contrastyou.losses.discreteMI import IIDLoss
    from contrastyou.losses.kl import Entropy, KL_div

    def params(cls):
        return [(n, p.kind) for n, p in inspect.signature(cls.__init__).parameters.items()]

    P = inspect.Parameter
    assert params(ml.AdaptiveOverSegmentedLoss) == [
        ("self", P.POSITIONAL_OR_KEYWORD), ("input_num_classes", P.POSITIONAL_OR_KEYWORD),
        ("output_num_classes", P.POSITIONAL_OR_KEYWORD), ("device", P.POSITIONAL_OR_KEYWORD),
        ("entropy_decay", P.POSITIONAL_OR_KEYWORD)]
    assert inspect.signature(ml.AdaptiveOverSegmentedLoss.__init__).parameters["entropy_decay"].default == 1e-3
    assert params(ml.StricterAdaptiveOverSegmentedLoss) == [
        ("self", P.POSITIONAL_OR_KEYWORD), ("input_num_classes", P.POSITIONAL_OR_KEYWORD),
        ("output_num_classes", P.POSITIONAL_OR_KEYWORD), ("device", P.POSITIONAL_OR_KEYWORD), ("kwargs", P.VAR_KEYWORD)]
    assert params(ml.StricterAdaptiveOverSegmentedLossWithMI) == [
        ("self", P.POSITIONAL_OR_KEYWORD), ("input_num_classes", P.POSITIONAL_OR_KEYWORD),
        ("output_num_classes", P.POSITIONAL_OR_KEYWORD), ("device", P.POSITIONAL_OR_KEYWORD),
        ("mi_weight", P.KEYWORD_ONLY), ("kwargs", P.VAR_KEYWORD)]

    a = ml.AdaptiveOverSegmentedLoss(8, 4, "cpu")
    s = ml.StricterAdaptiveOverSegmentedLoss(8, 4, "cpu", anything=1)
    m = ml.StricterAdaptiveOverSegmentedLossWithMI(8, 4, "cpu", mi_weight=0.1)
    for crit, shape in ((a, (8, 4)), (s, (4, 4)), (m, (4, 4))):
        assert isinstance(crit, ml.GeneralOverSegmentedLoss) and isinstance(crit.kl, KL_div)
        assert list(crit.state_dict()) == ["_translate_matrix"]
        assert [n for n, _ in crit.named_parameters()] == ["_translate_matrix"]
        assert tuple(crit._translate_matrix.shape) == shape and crit._translate_matrix.requires_grad
        assert list(inspect.signature(crit.forward).parameters) == ["predict_simplex", "onehot_target"]
        assert list(inspect.signature(crit.reduced_simplex).parameters) == ["predict_simplex"]
        for name in ("mix", "kl_from_logits", "from_logits"):
            assert callable(getattr(crit, name)), name
        mix = crit.mix()
        assert tuple(mix.shape) == (8, 4) and mix.requires_grad
        assert torch.allclose(mix.sum(1), torch.ones(8))
        assert crit.fusable(8) and not crit.fusable(12)
    assert isinstance(a.entropy, Entropy) and a._entropy_decay == 1e-3
    assert float(a._translate_matrix.detach().std()) > 0.3                 # randn
    assert torch.equal(s._translate_matrix, torch.zeros(4, 4))    # zeros under the fixed diagonal
    assert torch.equal(s._diagonal_matrix, 30 * torch.eye(4)) and not isinstance(s._diagonal_matrix, torch.nn.Parameter)
    assert tuple(s.translate_matrix.shape) == (8, 4) and torch.equal(s.translate_matrix[:4], 30 * torch.eye(4))
    assert s.needs_optimize and m.needs_optimize
    assert isinstance(m._mi, IIDLoss) and m._mi_weight == 0.1
    # K = C: nothing to learn, the mix has no autograd history, so its gradient is never asked for
    s44 = ml.StricterAdaptiveOverSegmentedLoss(4, 4, "cpu")
    assert not s44.needs_optimize and s44._translate_matrix.numel() == 0
    assert list(s44.state_dict()) == ["_translate_matrix"]
    assert not s44.mix().requires_grad
    m44 = ml.StricterAdaptiveOverSegmentedLossWithMI(4, 4, "cpu", mi_weight=0.1)
    assert not m44.needs_optimize and m44.extra_terms() is None
    with pytest.raises(AssertionError):
        ml.StricterAdaptiveOverSegmentedLoss(3, 4, "cpu")
    assert not ml.AdaptiveOverSegmentedLoss(80, 5, "cpu").fusable(80)    # wider than the kernels
    assert not ml.AdaptiveOverSegmentedLoss(40, 20, "cpu").fusable(40)   # more classes than the kernels
    # GradientReverse / scale_grad as in the reference: identity forward, gradient times the (global) scale
    x = torch.tensor([1.0, -2.0], requires_grad=True)
    y = ml.scale_grad(x, 0.5)
    assert torch.equal(y, x) and ml.GradientReverse.scale == 0.5
    y.sum().backward()
    assert torch.equal(x.grad, torch.tensor([0.5, 0.5]))
    ml.scale_grad(x, 1.0)
    # the package exports them too
    import contrastyou.losses as L
    for name in ("AdaptiveOverSegmentedLoss", "StricterAdaptiveOverSegmentedLoss",
                 "StricterAdaptiveOverSegmentedLossWithMI", "GradientReverse", "scale_grad"):
        assert getattr(L, name) is getattr(ml, name)


def test_probability_space_members_on_hand_values():
    """plain torch ops on the CPU"""
    from contrastyou.losses.multicore_loss import AdaptiveOverSegmentedLoss, StricterAdaptiveOverSegmentedLoss
    ln2, ln3 = math.log(2.0), math.log(3.0)
    a = AdaptiveOverSegmentedLoss(3, 2, "cpu", entropy_decay=0.5)
    with torch.no_grad():
        # softmax rows: [2/3, 1/3], [1/2, 1/2], [1/4, 3/4]
        a._translate_matrix.copy_(torch.tensor([[ln2, 0.0], [0.0, 0.0], [0.0, ln3]]))
    M = torch.tensor([[2 / 3, 1 / 3], [0.5, 0.5], [0.25, 0.75]])
    assert torch.allclose(a.mix(), M, atol=1e-7)
    p = torch.tensor([[0.2, 0.3, 0.5], [0.6, 0.4, 0.0]]).t().reshape(1, 3, 1, 2)  # two pixels
    red = a.reduced_simplex(p)
    want = torch.tensor([[0.2 * 2 / 3 + 0.15 + 0.125, 0.4 + 0.2], [0.2 / 3 + 0.15 + 0.375, 0.2 + 0.2]]).view(1, 2, 1, 2)
    assert red.shape == (1, 2, 1, 2) and torch.allclose(red, want, atol=1e-6)
    onehot = torch.tensor([[0, 1], [1, 0]]).view(1, 2, 1, 2)  # pixel 0 -> class 1, pixel 1 -> class 0
    kl = -(math.log(float(want[0, 1, 0, 0])) + math.log(0.6)) / 2
    ent = -sum(float((r * r.log()).sum()) for r in M) / 3
    loss = a(p, onehot)
    assert abs(float(loss) - (kl + 0.5 * ent)) < 1e-6
    loss.backward()
    assert a._translate_matrix.grad is not None and float(a._translate_matrix.grad.abs().sum()) > 0

    s = StricterAdaptiveOverSegmentedLoss(3, 2, "cpu")
    with torch.no_grad():
        s._translate_matrix.copy_(torch.tensor([[0.0, ln3]]))
    Ms = s.mix()
    assert torch.allclose(Ms, torch.tensor([[1.0, 0.0], [0.0, 1.0], [0.25, 0.75]]), atol=1e-6)
    red = s.reduced_simplex(p)
    want = torch.tensor([[0.2 + 0.125, 0.6], [0.3 + 0.375, 0.4]]).view(1, 2, 1, 2)
    assert torch.allclose(red, want, atol=1e-6)
    assert abs(float(s(p, onehot)) + (math.log(0.675) + math.log(0.6)) / 2) < 1e-6


def test_the_five_entries_exist_in_header_and_binding():
    from cyhip import _lib
    header = (Path(__file__).resolve().parents[1] / "include" / "contrastyou_hip.h").read_text()
    declared = set(re.findall(r"\b(cy_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared, name
        assert name in _lib._SIGS, name
        assert hasattr(lib, name), name
    assert lib.cy_abi_version() == _lib.ABI_VERSION


def _host_buffer():
    """a host address: the entries below return before they would touch it"""
    buf = ctypes.create_string_buffer(4096)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_argument_errors_are_reported_not_launched():
    from cyhip import _lib
    lib = _lib.load()
    keep, p = _host_buffer()
    big = 1 << 24

    def fwd(*, logits=p, target=p, mix=p, loss=p, npix=572, K=32, C=4, ws=p, ws_bytes=big):
        return lib.cy_softmax_mix_kl_fwd(logits, target, mix, loss, npix, K, C, EPS, ws, ws_bytes, None)

    def bwd(*, logits=p, target=p, mix=p, gscale=p, dlogits=p, dmix=p, npix=572, K=32, C=4, ws=p, ws_bytes=big):
        return lib.cy_softmax_mix_kl_bwd(logits, target, mix, gscale, dlogits, dmix, npix, K, C, EPS, ws, ws_bytes,
                                         None)

    def dice(*, logits=p, target=p, mix=p, counts=p, N=2, HW=286, K=32, C=4):
        return lib.cy_mix_dice_counts(logits, target, mix, counts, N, HW, K, C, None)

    # each pointer NULL in turn, a count < 1 -> CY_ERR_ARG
    for name in ("logits", "target", "mix", "loss", "ws"):
        assert fwd(**{name: None}) == ERR_ARG, name
    for name in ("logits", "target", "mix", "gscale", "dlogits", "ws"):
        assert bwd(**{name: None}) == ERR_ARG, name
    for name in ("logits", "target", "mix", "counts"):
        assert dice(**{name: None}) == ERR_ARG, name
    for n in (0, -1):
        assert fwd(npix=n) == ERR_ARG and bwd(npix=n) == ERR_ARG and bwd(npix=n, dmix=None, ws=None) == ERR_ARG
        assert dice(N=n) == ERR_ARG and dice(HW=n) == ERR_ARG
    # K or C out of range -> CY_ERR_SHAPE (also without dmix)
    for K, C in ((0, 4), (65, 4), (32, 0), (32, 17), (65, 17)):
        assert fwd(K=K, C=C) == ERR_SHAPE, (K, C)
        assert bwd(K=K, C=C) == ERR_SHAPE, (K, C)
        assert bwd(K=K, C=C, dmix=None, ws=None, ws_bytes=0) == ERR_SHAPE, (K, C)
        assert dice(K=K, C=C) == ERR_SHAPE, (K, C)
    # a workspace one byte short -> CY_ERR_WORKSPACE
    for K, C in ((4, 4), (16, 4), (16, 16), (21, 3), (32, 4), (64, 16)):
        need = lib.cy_softmax_mix_kl_ws_bytes(572, K)
        assert need > 0 and fwd(K=K, C=C, ws_bytes=need - 1) == ERR_WORKSPACE, (K, C)
        need = lib.cy_softmax_mix_kl_bwd_ws_bytes(572, K, C)
        assert need > 0 and bwd(K=K, C=C, ws_bytes=need - 1) == ERR_WORKSPACE, (K, C)
    # a NULL pointer is reported before a bad shape, a bad shape before a short workspace
    assert fwd(mix=None, K=65) == ERR_ARG and fwd(K=65, ws_bytes=0) == ERR_SHAPE
    assert bwd(mix=None, C=17) == ERR_ARG and bwd(C=17, ws_bytes=0) == ERR_SHAPE
    with pytest.raises(_lib.HipKernelError):
        _lib.call("cy_softmax_mix_kl_fwd", p, p, p, p, 572, 65, 4, EPS, p, big, None)
    del keep


def test_dmix_null_needs_no_workspace_but_still_checks_the_rest():
    """`dmix` NULL is accepted: then neither `ws` nor `ws_bytes` is looked at.  No call here may reach a launch, so the
    accepted form is shown through the checks that come after the pointer check."""
    from cyhip import _lib
    lib = _lib.load()
    keep, p = _host_buffer()
    # with dmix, a NULL or short workspace is an error ...
    assert lib.cy_softmax_mix_kl_bwd(p, p, p, p, p, p, 572, 32, 4, EPS, None, 0, None) == ERR_ARG
    assert lib.cy_softmax_mix_kl_bwd(p, p, p, p, p, p, 572, 32, 4, EPS, p, 0, None) == ERR_WORKSPACE
    # ... without it the same call gets past both checks: the next one (the shape) is what answers
    assert lib.cy_softmax_mix_kl_bwd(p, p, p, p, p, None, 572, 65, 4, EPS, None, 0, None) == ERR_SHAPE
    assert lib.cy_softmax_mix_kl_bwd(p, p, p, p, p, None, 572, 32, 17, EPS, None, 0, None) == ERR_SHAPE
    del keep


def test_workspace_sizes_follow_the_header():
    """forward: as cy_softmax_group_kl_ws_bytes.  backward: 4 * K * C * min(1024, ceil(npix / 16)); 0 for a count < 1"""
    from cyhip import _lib
    lib = _lib.load()
    for npix in (1, 15, 16, 17, 255, 256, 257, 572, 16384, 16385, 18432, 262144, 262145, 802816):
        for K in (1, 4, 15, 16, 17, 20, 21, 32, 40, 64):
            assert lib.cy_softmax_mix_kl_ws_bytes(npix, K) == lib.cy_softmax_group_kl_ws_bytes(npix, K), (npix, K)
            for C in (1, 2, 4, 5, 16):
                want = 4 * K * C * min(1024, -(-npix // 16))
                assert lib.cy_softmax_mix_kl_bwd_ws_bytes(npix, K, C) == want, (npix, K, C)
    assert lib.cy_softmax_mix_kl_bwd_ws_bytes(0, 32, 4) == 0
    assert lib.cy_softmax_mix_kl_bwd_ws_bytes(572, 0, 4) == 0
    assert lib.cy_softmax_mix_kl_bwd_ws_bytes(572, 32, 0) == 0


def test_add_logits_refuses_groups_together_with_mix():
    from contrastyou.meters import UniversalDice
    meter = UniversalDice(4)
    z, t = torch.zeros(1, 8, 2, 2), torch.zeros(1, 2, 2, dtype=torch.long)
    with pytest.raises(AssertionError, match="exclude each other"):
        meter.add_logits(z, t, groups=4, mix=torch.full((8, 4), 0.25))
    assert meter._pending == [] and meter._n == 0


def test_num_classes_of_an_adaptive_criterion():
    from contrastyou.losses.multicore_loss import AdaptiveOverSegmentedLoss
    from semi_seg.epochers.features.multicore_epocher import _MultiCoreMixin

    class Ep(_MultiCoreMixin):
        def __init__(self, config):
            self._sup_criterion = AdaptiveOverSegmentedLoss(32, 4, "cpu")
            self._trainer = None if config is None else type("T", (), {"_config": config})()

    assert Ep(None).num_classes == 4
    assert Ep({"Arch": {"true_num_classes": 4}}).num_classes == 4
    with pytest.raises(AssertionError):
        Ep({"Arch": {"true_num_classes": 5}}).num_classes
