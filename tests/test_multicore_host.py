"""CPU-side checks of the multi-prototype ("multicore") additions: the class surface of
contrastyou/losses/multicore_loss.py, the trainer and epochers importing, the detection of the contiguous equal
partition the fused kernels take, and the argument checks of the new C-ABI entries (csrc/cy_group_loss.hip), made
without a launch as tests/test_abi.py does."""
import ctypes
import inspect

import pytest

from multicore_fixture import groups_of

OK, ERR_ARG, ERR_SHAPE, ERR_WORKSPACE = 0, -1, -2, -5


def test_class_surface():
    from contrastyou.losses import multicore_loss as ml
    from contrastyou.losses.kl import KL_div
    assert list(inspect.signature(ml.MultiCoreKL.__init__).parameters) == ["self", "groups"]
    groups = groups_of(4, 8)
    crit = ml.MultiCoreKL(groups=groups)
    assert isinstance(crit, ml.GeneralOverSegmentedLoss)
    assert crit.groups == groups
    assert isinstance(crit.kl, KL_div)
    assert callable(crit.reduced_simplex) and callable(crit.from_logits)
    assert list(inspect.signature(crit.forward).parameters) == ["predict_simplex", "onehot_target"]
    assert getattr(ml.GeneralOverSegmentedLoss.reduced_simplex, "__isabstractmethod__", False)
    from contrastyou.losses import GeneralOverSegmentedLoss, MultiCoreKL  # the package exports them too
    assert MultiCoreKL is ml.MultiCoreKL and GeneralOverSegmentedLoss is ml.GeneralOverSegmentedLoss


def test_reduced_simplex_and_forward_on_the_cpu():
    """the probability-space members are plain torch ops"""
    import torch
    from contrastyou.losses.multicore_loss import MultiCoreKL
    crit = MultiCoreKL(groups=[[0, 3], [1, 2, 4]])
    p = torch.tensor([[0.1, 0.2, 0.3, 0.15, 0.25]]).view(1, 5, 1, 1)
    red = crit.reduced_simplex(p)
    assert torch.allclose(red.flatten(), torch.tensor([0.25, 0.75]))
    onehot = torch.tensor([0, 1]).view(1, 2, 1, 1)
    assert abs(float(crit(p, onehot)) + float(torch.log(torch.tensor(0.75)))) < 1e-6


def test_trainer_and_epochers_import():
    from semi_seg.epochers import EvalEpocher, SemiSupervisedEpocher
    from semi_seg.epochers.features import MultiCoreEvalEpocher, MultiCoreTrainEpocher
    from semi_seg.trainers import SemiTrainer, trainer_zoo
    from semi_seg.trainers.features import MulticoreTrainer
    assert issubclass(MultiCoreTrainEpocher, SemiSupervisedEpocher)
    assert issubclass(MultiCoreEvalEpocher, EvalEpocher)
    assert issubclass(MulticoreTrainer, SemiTrainer)
    assert MulticoreTrainer.train_epocher.fget(None) is MultiCoreTrainEpocher
    assert MulticoreTrainer not in trainer_zoo.values()  # the reference does not list it there either


def test_contiguous_partition_detection():
    from contrastyou.losses.multicore_loss import MultiCoreKL, contiguous_partition
    for C, m in ((4, 1), (3, 5), (4, 8), (8, 8)):
        assert contiguous_partition(groups_of(C, m)) == (C * m, C)
        assert contiguous_partition([range(c * m, (c + 1) * m) for c in range(C)]) == (C * m, C)
        assert MultiCoreKL(groups_of(C, m)).fusable(C * m)
    assert contiguous_partition([[2, 3], [0, 1]]) is None            # permuted classes
    assert contiguous_partition([[1, 0], [2, 3]]) is None            # permuted inside a class
    assert contiguous_partition([[0, 2], [1, 3]]) is None            # interleaved
    assert contiguous_partition([[0, 1, 2], [3]]) is None            # unequal
    assert contiguous_partition([[0, 1], [1, 2]]) is None            # overlapping
    assert contiguous_partition([[1, 2], [3, 4]]) is None            # does not start at 0
    assert contiguous_partition([]) is None
    assert not MultiCoreKL(groups_of(4, 8)).fusable(16)              # another channel count
    assert not MultiCoreKL(groups_of(5, 16)).fusable(80)             # wider than the kernels


def test_num_classes_comes_from_the_criterion():
    from contrastyou.losses.multicore_loss import MultiCoreKL
    from semi_seg.epochers.features.multicore_epocher import _MultiCoreMixin

    class Ep(_MultiCoreMixin):
        def __init__(self, config):
            self._sup_criterion = MultiCoreKL(groups_of(4, 8))
            self._trainer = None if config is None else type("T", (), {"_config": config})()

    assert Ep(None).num_classes == 4
    assert Ep({"Arch": {"true_num_classes": 4}}).num_classes == 4
    assert Ep({"Optim": {}}).num_classes == 4
    with pytest.raises(AssertionError):
        Ep({"Arch": {"true_num_classes": 5}}).num_classes


def test_fused_radam_tolerates_an_empty_param_group():
    import torch
    from contrastyou.optim.fused_radam import FlatParams
    flat = FlatParams([])
    assert flat.numel == 0 and flat.offsets == [0] and not flat.stale() and flat.touched() == []
    flat.zero_grad()
    assert flat.grad.numel() == 0 and flat.data.dtype == torch.float32


def _host_buffer():
    """a host address: the entries below return before they would touch it"""
    buf = ctypes.create_string_buffer(4096)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_argument_errors_are_reported_not_launched():
    from cyhip import _lib
    lib = _lib.load()
    keep, p = _host_buffer()
    big = 1 << 20
    # NULL pointers / no pixels -> CY_ERR_ARG
    assert lib.cy_softmax_group_kl_fwd(None, p, p, 572, 32, 4, 1e-16, p, big, None) == ERR_ARG
    assert lib.cy_softmax_group_kl_fwd(p, None, p, 572, 32, 4, 1e-16, p, big, None) == ERR_ARG
    assert lib.cy_softmax_group_kl_fwd(p, p, None, 572, 32, 4, 1e-16, p, big, None) == ERR_ARG
    assert lib.cy_softmax_group_kl_fwd(p, p, p, 572, 32, 4, 1e-16, None, big, None) == ERR_ARG
    assert lib.cy_softmax_group_kl_fwd(p, p, p, 0, 32, 4, 1e-16, p, big, None) == ERR_ARG
    assert lib.cy_softmax_group_kl_bwd(p, p, p, None, 572, 32, 4, 1e-16, None) == ERR_ARG
    assert lib.cy_softmax_group_kl_bwd(p, p, None, p, 572, 32, 4, 1e-16, None) == ERR_ARG
    assert lib.cy_group_dice_counts(p, p, None, 2, 286, 32, 4, None) == ERR_ARG
    assert lib.cy_group_dice_counts(None, p, p, 2, 286, 32, 4, None) == ERR_ARG
    assert lib.cy_group_dice_counts(p, p, p, 0, 286, 32, 4, None) == ERR_ARG
    # K out of range, G that does not divide K -> CY_ERR_SHAPE
    for K, G in ((65, 5), (65, 65), (0, 1), (32, 5), (32, 0), (21, 2), (4, 8)):
        assert lib.cy_softmax_group_kl_fwd(p, p, p, 572, K, G, 1e-16, p, big, None) == ERR_SHAPE, (K, G)
        assert lib.cy_softmax_group_kl_bwd(p, p, p, p, 572, K, G, 1e-16, None) == ERR_SHAPE, (K, G)
        assert lib.cy_group_dice_counts(p, p, p, 2, 286, K, G, None) == ERR_SHAPE, (K, G)
    # the softmax-MSE now takes K <= 64, not more
    assert lib.cy_softmax_mse_fwd(p, p, p, 572, 65, p, big, None) == ERR_SHAPE
    assert lib.cy_softmax_mse_bwd(p, p, p, p, p, 572, 65, None) == ERR_SHAPE
    assert lib.cy_softmax_mse_fwd(None, p, p, 572, 32, p, big, None) == ERR_ARG
    assert lib.cy_softmax_mse_bwd(p, p, p, None, None, 572, 32, None) == ERR_ARG
    # a short workspace -> CY_ERR_WORKSPACE
    for K in (4, 16, 21, 32, 64):
        need = lib.cy_softmax_group_kl_ws_bytes(572, K)
        assert lib.cy_softmax_group_kl_fwd(p, p, p, 572, K, 1, 1e-16, p, need - 1, None) == ERR_WORKSPACE, K
    assert lib.cy_softmax_mse_fwd(p, p, p, 572, 32, p, lib.cy_softmax_mse_ws_bytes(572) - 1, None) == ERR_WORKSPACE
    with pytest.raises(_lib.HipKernelError):
        _lib.call("cy_softmax_group_kl_fwd", p, p, p, 572, 65, 5, 1e-16, p, big, None)
    del keep


def test_workspace_sizes_follow_the_header():
    """8 bytes per block, blocks = min(1024, ceil(npix / P)), P = 256 pixels for K <= 16 and 16 above"""
    from cyhip import _lib
    lib = _lib.load()
    for npix in (1, 15, 16, 17, 255, 256, 257, 572, 16384, 16385, 18432, 262144, 262145, 802816):
        for K in (1, 4, 15, 16):
            assert lib.cy_softmax_group_kl_ws_bytes(npix, K) == 8 * min(1024, -(-npix // 256)), (npix, K)
            assert lib.cy_softmax_group_kl_ws_bytes(npix, K) == lib.cy_softmax_kl_ws_bytes(npix)
        for K in (17, 20, 21, 32, 64):
            assert lib.cy_softmax_group_kl_ws_bytes(npix, K) == 8 * min(1024, -(-npix // 16)), (npix, K)
        assert lib.cy_softmax_mse_ws_bytes(npix) == 8 * min(1024, -(-npix // 256))  # unchanged, whatever K
