"""Patch-based cross-correlation between the over-segmentation softmax of the network OUTPUT and the image
(semi_seg/hooks/cc.py:21-146): for both unlabeled logit views, CCLoss between the entropy map of softmax(logits)
(normalised with the extrema of the whole batch) and the image's edge map, averaged over the two views, plus an
IIDSegmentationLoss term between the two views.  Gradient flows through both views' logits.

Kernels: csrc/cy_cc.hip through cyhip.functions (see semi_seg/hooks/ccblock.py); the softmax of each view runs once
(the reference evaluates it twice) on the grouped-softmax kernel.  The image dumps (`save=`) are not part of this build.
"""
from __future__ import annotations

import typing as t

from torch import Tensor

from contrastyou.arch import UNetFeatureMapEnum
from contrastyou.hooks.base import EpocherHook, TrainerHook
from contrastyou.losses.cross_correlation import CCLoss
from contrastyou.losses.discreteMI import IIDSegmentationLoss
from contrastyou.meters import AverageValueMeter
from contrastyou.utils import average_iter

from .ccblock import EdgeMapCache, cc_loss_per_head
from .midl import _softmax_map


class CrossCorrelationOnLogitsHook(TrainerHook):

    def __init__(self, *, name: str, feature_name: UNetFeatureMapEnum, cc_weight: float, mi_weight: float = 0.0,
                 kernel_size: int, mi_criterion_params: t.Dict[str, t.Any], norm_params: t.Dict[str, t.Any],
                 save: bool = True, **kwargs):
        super().__init__(hook_name=name)
        self._cc_weight = float(cc_weight)
        self._mi_weight = float(mi_weight)
        feature_name = UNetFeatureMapEnum(feature_name)
        self._feature_name = feature_name.value
        assert feature_name == UNetFeatureMapEnum.Deconv_1x1
        self._cc_criterion = CCLoss(win=(kernel_size, kernel_size))
        self._mi_criterion = IIDSegmentationLoss(**mi_criterion_params)
        self._diff_power: float = float(norm_params["power"])
        assert 0 <= self._diff_power <= 1, self._diff_power
        self.save = save
        self.saver = None

    def __call__(self, **kwargs):
        return _CrossCorrelationLogitEpocherHook(
            name=self._hook_name, cc_criterion=self._cc_criterion, mi_criterion=self._mi_criterion,
            cc_weight=self._cc_weight, mi_weight=self._mi_weight, diff_power=self._diff_power, saver=self.saver)


class _CrossCorrelationLogitEpocherHook(EpocherHook):

    def __init__(self, *, name: str = "cc", cc_criterion: CCLoss, mi_criterion: IIDSegmentationLoss, cc_weight: float,
                 mi_weight: float, diff_power: float, saver=None) -> None:
        super().__init__(name=name)
        self.cc_weight, self.mi_weight = cc_weight, mi_weight
        self.cc_criterion, self.mi_criterion = cc_criterion, mi_criterion
        self._diff_power = diff_power
        self.saver = saver
        self.edges = EdgeMapCache()

    def configure_meters_given_epocher(self, meters):
        meters.register_meter("cc_ls", AverageValueMeter())
        meters.register_meter("mi_ls", AverageValueMeter())
        return meters

    def _call_implementation(self, unlabeled_image_tf: Tensor, unlabeled_tf_logits: Tensor,
                             unlabeled_logits_tf: Tensor, **kwargs):
        prob_tf, tf_prob = _softmax_map(unlabeled_logits_tf), _softmax_map(unlabeled_tf_logits)
        losses, _diff_image, _diff_prediction = zip(*[
            self.cc_loss_per_head(image=unlabeled_image_tf, predict_simplex=x) for x in (prob_tf, tf_prob)])
        cc_loss = average_iter(losses)
        mi_loss = self.mi_loss_per_head(prob_tf, tf_prob)
        if self.meters:
            self.meters["cc_ls"].add(cc_loss.detach())
            self.meters["mi_ls"].add(mi_loss.detach())
        return cc_loss * self.cc_weight + mi_loss * self.mi_weight

    def cc_loss_per_head(self, image: Tensor, predict_simplex: Tensor):
        return cc_loss_per_head(self.cc_criterion, image, predict_simplex, self._diff_power, False, self.edges)

    def mi_loss_per_head(self, prob1, prob2):
        return self.mi_criterion(prob1, prob2)
