"""CPU-side checks of the cross-correlation family: the reference's import paths exist, the hook factory dispatches
as semi_seg/hooks/creator.py:196-239 does, the projector's parameters carry the reference's names, and the new C
entry points (ABI v15) refuse bad arguments before any launch.  No kernel runs here."""
import ctypes

import numpy as np
import pytest
import torch

HOOK_PARAMS = {"cc": dict(weight=1.0, kernel_size=5, diff_power=0.75),
               "mi": dict(weight=0.1, lamda=1.0, padding=0),
               "rr": dict(weight=0.1, alpha=0.5)}


@pytest.fixture()
def net():
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    type(TrainerHook).names.clear()
    return UNet(input_dim=1, num_classes=4, max_channel=128)


def test_reference_import_paths_exist():
    from contrastyou.losses.cross_correlation import CCLoss  # noqa: F401
    from contrastyou.projectors import CrossCorrelationProjector  # noqa: F401
    from semi_seg.hooks import create_cross_correlation_hooks2  # noqa: F401
    from semi_seg.hooks.cc import CrossCorrelationOnLogitsHook  # noqa: F401
    from semi_seg.hooks.ccblock import (ProjectorGeneralHook, _ConsistencyHook, _CrossCorrelationHook,  # noqa: F401
                                        _MIHook, _RedundancyReduction, _TinyHook)


@pytest.mark.parametrize("head_type", ["linear", "mlp"])
def test_factory_on_a_feature_map(net, golden_dir, head_type):
    from contrastyou.hooks.base import CombineTrainerHook
    from contrastyou.projectors import CrossCorrelationProjector
    from semi_seg.hooks import create_cross_correlation_hooks2, feature_until_from_hooks
    from semi_seg.hooks.ccblock import ProjectorGeneralHook, _CrossCorrelationHook, _MIHook, _RedundancyReduction
    hook = create_cross_correlation_hooks2(model=net, feature_name="Up_conv2", num_clusters=10, head_type=head_type,
                                           num_subheads=2, save=True, hook_params=HOOK_PARAMS)
    assert isinstance(hook, CombineTrainerHook) and len(hook._hooks) == 1
    member = hook._hooks[0]
    assert isinstance(member, ProjectorGeneralHook) and member._hook_name == "cc_Up_conv2"
    (projector,) = member.learnable_modules
    assert isinstance(projector, CrossCorrelationProjector)
    names = sorted(projector.state_dict())
    assert names == list(np.load(golden_dir / "cc.npz")[f"names_{head_type}_2"])
    assert len(list(hook.parameters())) == len(names)
    assert [type(h) for h in member._dist_hooks] == [_MIHook, _CrossCorrelationHook, _RedundancyReduction]
    assert member._feature_hooks == []
    assert feature_until_from_hooks(hook, model=net) == "Up_conv2"
    if head_type == "mlp":  # hidden_dim = 64 (creator.py:204)
        assert projector._headers[0][0].weight.shape == (64, net.get_channel_dim("Up_conv2"), 1, 1)
    assert member().name == "cc_Up_conv2"  # an epocher hook is handed out once tiny hooks are registered
    assert member.saver is None and member.matrix_saver is None  # save=True is accepted; the dumps are not built


def test_factory_on_the_logits(net):
    from semi_seg.hooks import create_cross_correlation_hooks2
    from semi_seg.hooks.cc import CrossCorrelationOnLogitsHook, _CrossCorrelationLogitEpocherHook
    hook = create_cross_correlation_hooks2(model=net, feature_name="Deconv_1x1", num_clusters=10, head_type="linear",
                                           num_subheads=2, hook_params=HOOK_PARAMS)
    member = hook._hooks[0]
    assert isinstance(member, CrossCorrelationOnLogitsHook)
    assert member._feature_name == "Deconv_1x1" and member._diff_power == 0.75
    assert list(hook.parameters()) == []
    ep = member()
    assert isinstance(ep, _CrossCorrelationLogitEpocherHook) and ep.cc_weight == 1.0 and ep.mi_weight == 0.1


def test_general_hook_without_tiny_hooks_raises(net):
    from semi_seg.hooks.ccblock import ProjectorGeneralHook
    hook = ProjectorGeneralHook(name="empty", model=net, feature_name="Up_conv2", save=False,
                                projector_params=dict(num_clusters=5, head_type="linear", normalize=False))
    with pytest.raises(RuntimeError, match="hooks not registered"):
        hook()


@pytest.mark.parametrize("key,params", [("imsat", dict(weight=0.1)), ("compact", dict(weight=0.1))])
def test_hooks_outside_the_build_are_named(net, key, params):
    from semi_seg.hooks import create_cross_correlation_hooks2
    with pytest.raises(NotImplementedError, match="IMSAT|CenterCompactness"):
        create_cross_correlation_hooks2(model=net, feature_name="Up_conv2", num_clusters=10, head_type="linear",
                                        num_subheads=1, hook_params={key: params})


def test_ccloss_windows_and_channels():
    from contrastyou.losses.cross_correlation import CCLoss
    from semi_seg.hooks.ccblock import _CrossCorrelationHook
    for win in ((4, 4), (3, 5), (17, 17)):
        with pytest.raises(NotImplementedError, match=str(win[0])):
            CCLoss(win=win)
    with pytest.raises(NotImplementedError, match="4"):
        _CrossCorrelationHook(weight=1.0, kernel_size=4)
    crit = CCLoss(win=(5, 5))
    assert crit.eps == 1e-5 and crit.win == (5, 5) and crit.win_size == 25
    assert list(crit.state_dict()) == ["_sum_filt"] and crit._sum_filt.shape == (1, 1, 5, 5)
    with pytest.raises(RuntimeError, match="single-channel"):
        crit(torch.rand(1, 2, 8, 8), torch.rand(1, 2, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(torch.rand(1, 1, 8, 8), torch.rand(1, 1, 8, 8))


def test_weight_zero_short_cut():
    from semi_seg.hooks.ccblock import _ConsistencyHook, _MIHook, _RedundancyReduction
    p = torch.rand(2, 4, 6, 6).softmax(1)
    for tiny in (_MIHook(weight=0, lamda=1.0), _RedundancyReduction(weight=0, alpha=0.5), _ConsistencyHook(weight=0)):
        out = tiny(input1=p, input2=p, cur_epoch=0)
        assert out.item() == 0 and out.dtype == p.dtype
    kl = _ConsistencyHook(weight=2.0)(input1=p, input2=p.roll(1, 1), cur_epoch=0)  # KL_div is plain torch: runs here
    assert kl.item() > 0


NEW_SYMBOLS = ["cy_cc_edge_map", "cy_cc_edge_map_ws_bytes", "cy_entropy_map_fwd", "cy_entropy_map_bwd",
               "cy_entropy_map_ws_bytes", "cy_ccloss_fwd", "cy_ccloss_bwd", "cy_ccloss_ws_bytes"]


def test_library_exports_abi_15():
    from cyhip import _lib
    lib = _lib.load()
    assert lib.cy_abi_version() == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.exported_names(), name


def test_new_entry_points_check_arguments_before_launching():
    """NULL -> CY_ERR_ARG, window 4 / 17, K = 129, C = 5 -> CY_ERR_SHAPE, short workspace -> CY_ERR_WORKSPACE; the
    pointers handed over are host memory, which no launch may ever see (safe without a GPU)"""
    from cyhip import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ARG, SHAPE, WS = -1, -2, -5
    big = 1 << 20
    assert lib.cy_cc_edge_map(None, p, 1, 8, 8, 1, 0.75, p, big, None) == ARG
    assert lib.cy_cc_edge_map(p, None, 1, 8, 8, 1, 0.75, p, big, None) == ARG
    assert lib.cy_cc_edge_map(p, p, 1, 8, 8, 1, 0.75, None, big, None) == ARG
    assert lib.cy_cc_edge_map(p, p, 0, 8, 8, 1, 0.75, p, big, None) == ARG
    assert lib.cy_cc_edge_map(p, p, 1, 8, 8, 5, 0.75, p, big, None) == SHAPE
    assert lib.cy_cc_edge_map(p, p, 1, 8, 8, 0, 0.75, p, big, None) == SHAPE
    assert lib.cy_cc_edge_map(p, p, 1, 8, 8, 1, 0.75, p, 4, None) == WS
    assert lib.cy_entropy_map_fwd(None, p, p, 1, 64, 5, 1, p, big, None) == ARG
    assert lib.cy_entropy_map_fwd(p, p, None, 1, 64, 5, 1, p, big, None) == ARG
    assert lib.cy_entropy_map_fwd(p, p, p, 1, 64, 129, 1, p, big, None) == SHAPE
    assert lib.cy_entropy_map_fwd(p, p, p, 1, 64, 0, 1, p, big, None) == SHAPE
    assert lib.cy_entropy_map_fwd(p, p, p, 1, 64, 5, 1, p, 4, None) == WS
    assert lib.cy_entropy_map_bwd(p, p, None, p, 1, 64, 5, None) == ARG
    assert lib.cy_entropy_map_bwd(p, p, p, p, 1, 64, 129, None) == SHAPE
    assert lib.cy_ccloss_fwd(None, p, p, 1, 8, 8, 5, 1e-5, p, big, None) == ARG
    assert lib.cy_ccloss_fwd(p, p, None, 1, 8, 8, 5, 1e-5, p, big, None) == ARG
    assert lib.cy_ccloss_fwd(p, p, p, 1, 8, 8, 5, 1e-5, None, big, None) == ARG
    for win in (4, 17, 1, 0, -3):
        assert lib.cy_ccloss_fwd(p, p, p, 1, 8, 8, win, 1e-5, p, big, None) == SHAPE, win
        assert lib.cy_ccloss_bwd(p, p, p, p, p, 1, 8, 8, win, 1e-5, None) == SHAPE, win
    assert lib.cy_ccloss_fwd(p, p, p, 1, 8, 8, 5, 1e-5, p, 4, None) == WS
    assert lib.cy_ccloss_bwd(p, p, None, p, p, 1, 8, 8, 5, 1e-5, None) == ARG
    assert lib.cy_ccloss_bwd(p, p, p, None, None, 1, 8, 8, 5, 1e-5, None) == ARG
    assert lib.cy_ccloss_ws_bytes(16, 224, 224) == 16 * 7 * 7 * 8
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_SHAPE"):
        _lib.call("cy_ccloss_fwd", p, p, p, 1, 8, 8, 4, 1e-5, p, big, None)
