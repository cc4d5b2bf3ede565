"""Cross-correlation regulariser on a tapped feature map -- the hook family of semi_seg/hooks/ccblock.py:38-490.

A `ProjectorGeneralHook` taps `feature_name`, projects the two unlabeled views' features with a
`CrossCorrelationProjector` (an over-segmentation into `num_clusters` classes, several sub-heads) and sums what its
registered *tiny hooks* compute on the two probability maps:

    cc       _CrossCorrelationHook   CCLoss between the entropy map of each view's prediction and the edge map of the image
    mi       _MIHook                 IIDSegmentationLoss between the two views
    rr       _RedundancyReduction    RedundancyCriterion between the two views
    consist  _ConsistencyHook        KL_div of view 1 against the detached view 2

loss = feature terms + mean over sub-heads of the distribution terms.  The cc term runs on csrc/cy_cc.hip:
per head 4 launches forward (entropy + extrema, normalise, window sums, final sum) and 2 backward; the edge map of
the image (2 launches, + 1 when the image is resized first) is computed once per call and image size and shared by
both views and all sub-heads.  Meters take device scalars (no `.item()` per tiny hook); the image dumps of the
reference (`save=`, FeatureMapSaver, DistributionTracker, joint_2D_figure) are logging and not part of this build:
`save=True` is accepted and ignored.  `_ConsistencyHook` leaves out the reference's `assert simplex(input1)` (a host
sync per call).  None of the tiny hooks built here draws random numbers, so the reference's
`fix_all_seed_within_context(seed)` around them (it serves the deprecated compactness hook) is not entered.
"""
from __future__ import annotations

import typing as t
import weakref
from abc import ABCMeta
from itertools import chain

import torch
from torch import Tensor, nn

from contrastyou.arch.utils import SingleFeatureExtractor
from contrastyou.hooks.base import EpocherHook, TrainerHook
from contrastyou.losses.cross_correlation import CCLoss
from contrastyou.losses.discreteMI import IIDSegmentationLoss
from contrastyou.losses.kl import KL_div
from contrastyou.losses.redundancy_reduction import RedundancyCriterion
from contrastyou.meters import AverageValueMeter
from contrastyou.projectors import CrossCorrelationProjector
from contrastyou.utils import class_name
from cyhip.functions import EntropyMapFn, edge_map

__all__ = ["ProjectorGeneralHook", "_CrossCorrelationHook", "_MIHook"]


class EdgeMapCache:
    """norm(diff(image)) ** power per (image, map size, power): both views of a hook call, and all its sub-heads, see
    the same `unlabeled_image_tf` object.  Remembers the maps of the last image only, and that image by weak reference
    (it is not kept alive, and a later tensor at the same address is not mistaken for it)."""

    def __init__(self) -> None:
        self._image, self._version, self._maps = None, None, {}

    def __call__(self, image: Tensor, size: t.Tuple[int, int], power: float) -> Tensor:
        if self._image is None or self._image() is not image or self._version != image._version:
            self._image, self._version, self._maps = weakref.ref(image), image._version, {}
        key = (tuple(size), float(power))
        if key not in self._maps:
            self._maps[key] = edge_map(image, power, size)
        return self._maps[key]

    def clear(self) -> None:
        self._image, self._version, self._maps = None, None, {}


def cc_loss_per_head(criterion: CCLoss, image: Tensor, predict_simplex: Tensor, diff_power: float, slicewise: bool,
                     edges: EdgeMapCache):
    """ccblock.py:295-309 (slicewise) / cc.py:127-142 (batch-wide extrema of the entropy map):
    -> (loss, diff_image, diff_tf_softmax)"""
    diff_image = edges(image, tuple(predict_simplex.shape[-2:]), diff_power)
    diff_tf_softmax = EntropyMapFn.apply(predict_simplex, slicewise)
    return criterion(diff_tf_softmax, diff_image), diff_image, diff_tf_softmax


def _zero(like: Tensor) -> Tensor:
    return torch.tensor(0, device=like.device, dtype=like.dtype)


# new interface
class _TinyHook(metaclass=ABCMeta):

    def __init__(self, *, name: str, criterion: nn.Module, weight: float) -> None:
        self.name = name
        self.criterion = criterion
        self.weight = weight
        self.meters = None
        self.hook = None

    def configure_meters(self, meters):
        meters.register_meter(self.name, AverageValueMeter())
        return meters

    def _record(self, loss) -> None:
        if self.meters:
            self.meters[self.name].add(loss.detach() if isinstance(loss, Tensor) else loss)

    def __call__(self, **kwargs) -> Tensor:
        loss = self.criterion(**kwargs)
        self._record(loss)
        return loss * self.weight

    def close(self):
        pass

    def __repr__(self):
        return f"{self.__class__.__name__}: {self.name}{self.__repr_extra__()}"

    def __repr_extra__(self):
        return f"weight={self.weight}"


class ProjectorGeneralHook(TrainerHook):

    def __init__(self, *, name: str, model: nn.Module, feature_name: str, projector_params: t.Dict[str, t.Any],
                 save: bool = False):
        super().__init__(hook_name=name)
        self._feature_name = feature_name
        self._extractor = SingleFeatureExtractor(model=model, feature_name=feature_name)
        input_dim = model.get_channel_dim(feature_name)
        self._projector = CrossCorrelationProjector(input_dim=input_dim, **projector_params)
        self._feature_hooks: t.List[_TinyHook] = []
        self._dist_hooks: t.List[_TinyHook] = []
        self.save = save
        self.saver = self.dist_saver = self.matrix_saver = None  # the image dumps are not part of this build

    def register_feat_hook(self, *hook: "_TinyHook"):
        self._feature_hooks.extend(hook)

    def register_dist_hook(self, *hook: "_TinyHook"):
        self._dist_hooks.extend(hook)

    def __call__(self, **kwargs):
        if (len(self._feature_hooks) + len(self._dist_hooks)) == 0:
            raise RuntimeError(f"hooks not registered for {class_name(self)}.")
        return _ProjectorEpocherGeneralHook(
            name=self._hook_name, extractor=self._extractor, projector=self._projector, dist_hooks=self._dist_hooks,
            feat_hooks=self._feature_hooks, saver=self.saver, dist_saver=self.dist_saver,
            matrix_saver=self.matrix_saver)

    @property
    def learnable_modules(self) -> t.List[nn.Module]:
        return [self._projector, ]


class _ProjectorEpocherGeneralHook(EpocherHook):

    def __init__(self, *, name: str, extractor: SingleFeatureExtractor, projector: nn.Module,
                 dist_hooks: t.Sequence[_TinyHook] = (), feat_hooks: t.Sequence[_TinyHook] = (), saver=None,
                 dist_saver=None, matrix_saver=None) -> None:
        super().__init__(name=name)
        self.extractor = extractor
        self.extractor.bind()
        self.projector = projector
        self._feature_hooks = feat_hooks
        self._dist_hooks = dist_hooks
        self.saver, self.dist_saver, self.mx_saver = saver, dist_saver, matrix_saver

    def configure_meters_given_epocher(self, meters):
        meters = super().configure_meters_given_epocher(meters)
        for h in chain(self._dist_hooks, self._feature_hooks):
            h.meters = meters
            h.hook = weakref.proxy(self)
            h.configure_meters(meters)
        return meters

    def before_forward_pass(self, **kwargs):
        self.extractor.clear()
        self.extractor.set_enable(True)

    def after_forward_pass(self, **kwargs):
        self.extractor.set_enable(False)

    def _call_implementation(self, unlabeled_image_tf: Tensor, unlabeled_logits_tf: Tensor,
                             affine_transformer: t.Callable[[Tensor], Tensor], **kwargs):
        cur_epoch, cur_batch_num = self.epocher.cur_epoch, self.epocher.cur_batch_num
        n_unl = len(unlabeled_logits_tf)
        _unlabeled_features, unlabeled_tf_features = torch.chunk(self.extractor.tail(n_unl * 2), 2, dim=0)
        unlabeled_features_tf = affine_transformer(_unlabeled_features)
        feature_loss = self._run_feature_hooks(input1=unlabeled_features_tf, input2=unlabeled_tf_features,
                                               image=unlabeled_image_tf)
        projected_dist_tf, projected_tf_dist = zip(*[torch.chunk(x, 2) for x in self.projector(
            torch.cat([unlabeled_features_tf, unlabeled_tf_features], dim=0))])
        dist_losses = tuple(
            self._run_dist_hooks(
                input1=prob1, input2=prob2, image=unlabeled_image_tf, feature_map1=unlabeled_tf_features,
                feature_map2=unlabeled_features_tf, saver=self.saver, save_image_condition=False,
                cur_epoch=cur_epoch, cur_batch_num=cur_batch_num)
            for prob1, prob2 in zip(projected_tf_dist, projected_dist_tf))
        return feature_loss + sum(dist_losses) / len(dist_losses)

    def _run_feature_hooks(self, **kwargs):
        return sum(h(**kwargs) for h in self._feature_hooks)

    def _run_dist_hooks(self, **kwargs):
        return sum(h(**kwargs) for h in self._dist_hooks)

    def close(self):
        self.extractor.remove()
        for h in chain(self._feature_hooks, self._dist_hooks):
            h.close()


class _CrossCorrelationHook(_TinyHook):

    def __init__(self, *, name: str = "cc", weight: float, kernel_size: int, diff_power: float = 0.75) -> None:
        criterion = CCLoss(win=(kernel_size, kernel_size))
        super().__init__(name=name, criterion=criterion, weight=weight)
        self._diff_power = diff_power
        self._edges = EdgeMapCache()  # one tiny hook serves both views and every sub-head of a call
        self.diff_image = self.diff_prediction = None

    def __repr_extra__(self):
        return f"{super().__repr_extra__()} diff_power={self._diff_power}"

    def __call__(self, *, image: Tensor, input1: Tensor, input2: Tensor, **kwargs):
        # f32 whatever the autocast state: the kernels are f32 (the reference forces autocast off here)
        losses, self.diff_image, self.diff_prediction = zip(*[
            self.cc_loss_per_head(image=image, predict_simplex=x) for x in (input1, input2)])
        loss = sum(losses) / len(losses)
        self._record(loss)
        return loss * self.weight

    def cc_loss_per_head(self, image: Tensor, predict_simplex: Tensor):
        return cc_loss_per_head(self.criterion, image, predict_simplex, self._diff_power, True, self._edges)


class _WeightedPairHook(_TinyHook):
    """criterion(input1, input2) * weight with the reference's `weight == 0` short cut"""

    def _second(self, input2: Tensor) -> Tensor:
        return input2

    def __call__(self, input1: Tensor, input2: Tensor, cur_epoch: int = 0, **kwargs):
        if self.weight == 0:
            self._record(0)
            return _zero(input1)
        loss = self.criterion(input1, self._second(input2))
        self._record(loss)
        return loss * self.weight


class _MIHook(_WeightedPairHook):

    def __init__(self, *, name: str = "mi", weight: float, lamda: float, padding: int = 0, symmetric=True) -> None:
        self.lamda, self.padding, self.symmetric = lamda, padding, symmetric
        super().__init__(name=name, criterion=IIDSegmentationLoss(lamda=lamda, padding=padding, symmetric=symmetric),
                         weight=weight)

    def __repr_extra__(self):
        return super().__repr_extra__() + f" lamda={self.lamda} padding={self.padding} symmetric={self.symmetric}"


class _RedundancyReduction(_WeightedPairHook):

    def __init__(self, *, name: str = "rr", weight: float, symmetric: bool = True, lamda: float = 1,
                 alpha: float) -> None:
        self.lamda, self.symmetric, self.alpha = lamda, symmetric, alpha
        super().__init__(name=name, criterion=RedundancyCriterion(symmetric=symmetric, lamda=lamda, alpha=alpha),
                         weight=weight)

    def __repr_extra__(self):
        return super().__repr_extra__() + f" lamda={self.lamda} alpha={self.alpha} symmetric={self.symmetric}"


class _ConsistencyHook(_WeightedPairHook):

    def __init__(self, *, name: str = "consistency", weight: float) -> None:
        super().__init__(name=name, criterion=KL_div(), weight=weight)

    def _second(self, input2: Tensor) -> Tensor:
        return input2.detach()


class _CenterCompactnessHook(_TinyHook):
    """`@deprecated` in the reference (ccblock.py:379-425)"""

    def __init__(self, *, name: str = "center", weight: float) -> None:
        raise NotImplementedError("_CenterCompactnessHook is deprecated in the reference and not part of this build")


class _IMSATHook(_TinyHook):
    """needs IMSATDynamicWeight, a loss outside this build (ccblock.py:428-472)"""

    def __init__(self, *, name: str = "imsat", weight: float, use_dynamic=True, lamda: float = 1.0) -> None:
        raise NotImplementedError("_IMSATHook needs the IMSAT losses, which are not part of this build")
