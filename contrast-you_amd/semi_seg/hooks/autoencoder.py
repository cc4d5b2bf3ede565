"""The denoising-auto-encoder prior (semi_seg/hooks/autoencoder.py:14-60 of the reference): a learnable 1x1
convolution K -> 1 with a sigmoid (or tanh) reconstructs the unlabeled image from its own logits, and
weight * F.mse_loss(reconstruction, unlabeled_image_tf) joins the regularisation loss.  `DAELossFn` (cy_dae_*) reads
the logits once each way: the reconstruction, the difference map and their gradients are never formed, and the
gradients of the layer's weight and bias leave the same pass through f64 block partials.  The layer's parameters join
the optimizer's second group and the checkpoint through `learnable_modules`.  The meter takes the device scalar.

Kept as the reference has it: the epocher hook is always named "deAE", whatever `hook_name` the trainer hook was given;
further keyword arguments of the trainer hook are accepted and ignored."""
from __future__ import annotations

import typing as t

from torch import Tensor, nn

from contrastyou.hooks.base import EpocherHook, TrainerHook
from contrastyou.meters import AverageValueMeter
from cyhip.functions import DAELossFn, HeadFn

if t.TYPE_CHECKING:
    from contrastyou.meters import MeterInterface


class AuxiliaryLayer(nn.Module):
    """a 1x1 convolution and a sigmoid or tanh: logits -> a map in the image's range"""

    def __init__(self, *, in_features: int, out_features: int = 1, activation: str = 'sigmoid'):
        assert activation in {'sigmoid', 'tanh'}, activation
        super().__init__()
        self.fc = nn.Conv2d(in_features, out_features, kernel_size=1)
        self.activation = nn.Sigmoid() if activation == 'sigmoid' else nn.Tanh()
        self.activation_name = activation

    def forward(self, x):
        """the activated map, for callers that want it (the loss does not come through here)"""
        return self.activation(HeadFn.apply(x, self.fc.weight, self.fc.bias))


class DenoisingAutoEncoderTrainerHook(TrainerHook):
    def __init__(self, *, hook_name: str = "deAE", num_classes: int, weight: float = 0.0, **kwargs):
        super().__init__(hook_name=hook_name)
        self.num_classes = num_classes
        self.aux_layer = AuxiliaryLayer(in_features=num_classes, out_features=1)
        self.weight = weight

    @property
    def learnable_modules(self) -> t.List[nn.Module]:
        return [self.aux_layer, ]

    def __call__(self, *args, **kwargs):
        return DenoisingAutoEncoderEpocherHook(extra_layer=self.aux_layer, weight=self.weight)


class DenoisingAutoEncoderEpocherHook(EpocherHook):

    def __init__(self, *, name: str = "deAE", extra_layer: "AuxiliaryLayer", weight) -> None:
        super().__init__(name=name)
        if extra_layer.fc.out_channels != 1:
            raise ValueError("the fused DAE loss reconstructs one channel (it broadcasts over the image's, as "
                             f"F.mse_loss does): out_features must be 1, got {extra_layer.fc.out_channels}")
        self.layer = extra_layer
        self._weight = weight

    def _call_implementation(self, *, unlabeled_image_tf: Tensor, unlabeled_tf_logits: Tensor, **kwargs):
        loss = DAELossFn.apply(unlabeled_tf_logits, self.layer.fc.weight, self.layer.fc.bias, unlabeled_image_tf,
                               self.layer.activation_name)
        if self.meters:
            self.meters["ls"].add(loss.detach())
        return self._weight * loss

    def configure_meters_given_epocher(self, meters: 'MeterInterface'):
        self.meters.register_meter("ls", AverageValueMeter())
