"""MixUp on the labeled batch (semi_seg/hooks/mixup.py:15-78 of the reference): under the step's seed one (lam, index)
is drawn for the 2B batch cat([labeled_image, labeled_image_tf]) with alpha = 1, the images are mixed
(`ops.mix_images` = cy_mix_images, bit-equal to the reference's `lam * x + (1 - lam) * x[index]`), the model runs on
them -- outside the running BatchNorm statistics when `enable_bn` is false -- and
weight * KL_div()(softmax(mixed_logits), lam * onehot(y) + (1 - lam) * onehot(y)[index]) is returned.  The mixed target
has at most two classes per pixel: `MixupKLFn` (cy_softmax_mixkl_*) reads the two integer labels, so neither one-hot
tensor, nor their concatenation, gathered copy and blend, nor a softmax is formed.  The meter takes the device scalar."""
from __future__ import annotations

from contextlib import nullcontext

import torch
from torch import Tensor

from contrastyou.hooks.base import EpocherHook, TrainerHook
from contrastyou.losses.kl import KL_div
from contrastyou.meters import AverageValueMeter, MeterInterface
from contrastyou.utils.utils import disable_tracking_bn_stats, fix_all_seed_within_context
from cyhip import ops
from cyhip.functions import MixupKLFn
from semi_seg.hooks.utils import mixup_draw


class MixUpTrainHook(TrainerHook):
    def __init__(self, *, hook_name: str, weight: float, enable_bn=True):
        super().__init__(hook_name=hook_name)
        self._weight = weight
        self._enable_bn = enable_bn

    def __call__(self, **kwargs):
        return _MixUpEpocherHook(name="mix_reg", weight=self._weight, criterion=KL_div(), enable_bn=self._enable_bn)


class _MixUpEpocherHook(EpocherHook):
    def __init__(self, *, name: str, weight: float, alpha: float = 1.0, criterion, enable_bn: bool) -> None:
        super().__init__(name=name)
        self._weight = weight
        self._alpha = alpha  # (kept as the reference keeps it: its call draws with alpha = 1 whatever this says)
        self._criterion = criterion
        self._eps = float(getattr(criterion, "_eps", 1e-16))
        self._enable_bn = enable_bn

    def configure_meters_given_epocher(self, meters: MeterInterface):
        meters = super().configure_meters_given_epocher(meters)
        meters.register_meter("loss", AverageValueMeter())
        return meters

    def _call_implementation(self, *, labeled_image: Tensor, labeled_image_tf: Tensor, labeled_target: Tensor,
                             labeled_target_tf: Tensor, seed: int, **kwargs):
        images = torch.cat([labeled_image, labeled_image_tf], dim=0)
        n = images.shape[0]
        target = torch.cat([labeled_target.to(torch.int64).reshape(n // 2, *labeled_image.shape[-2:]),
                            labeled_target_tf.to(torch.int64).reshape(n // 2, *labeled_image.shape[-2:])], dim=0)
        with fix_all_seed_within_context(seed):
            lam, index = mixup_draw(n, alpha=1)
        w_self, w_other = ops.mix_weights(lam)
        index = ops.mix_index(index, n, images.device)
        mixed_image = ops.mix_images(images.float(), index, w_self, w_other)
        with self.bn_context_manger(self._model):
            mixed_logits = self._model(mixed_image)
        reg_loss = MixupKLFn.apply(mixed_logits, target, index, w_self, w_other, self._eps)
        if self.meters:
            self.meters["loss"].add(reg_loss.detach())
        return reg_loss * self._weight

    @property
    def _model(self):
        return self.epocher._model  # noqa

    @property
    def device(self):
        return self.epocher.device

    @property
    def num_classes(self):
        return self.epocher.num_classes

    @property
    def bn_context_manger(self):
        return disable_tracking_bn_stats if not self._enable_bn else nullcontext
