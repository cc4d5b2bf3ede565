"""Entropy minimisation (semi_seg/hooks/entmin.py:7-33): weight * Entropy()(softmax(unlabeled_logits_tf)), through
`Entropy.from_logits` -- one fused HIP pass over the logits each way (cy_softmax_entropy_*; cy_softmax_entropy_row_*
on multi-prototype logits, 16 < K <= 64), no probability tensor.
The reference's `assert not simplex(logits)` is a host sync and is left out; the meter receives a device scalar."""
from __future__ import annotations

from contrastyou.hooks.base import EpocherHook, TrainerHook
from contrastyou.losses.kl import Entropy
from contrastyou.meters import AverageValueMeter, MeterInterface


class EntropyMinTrainerHook(TrainerHook):

    def __init__(self, name: str, weight: float):
        super().__init__(hook_name=name)
        self._weight = weight
        self._criterion = Entropy()

    def __call__(self):
        return _EntropyEpocherHook(name=self._hook_name, weight=self._weight, criterion=self._criterion)


class _EntropyEpocherHook(EpocherHook):
    def __init__(self, name: str, weight: float, criterion) -> None:
        super().__init__(name=name)
        self._weight, self._criterion = weight, criterion

    def configure_meters_given_epocher(self, meters: MeterInterface):
        meters = super().configure_meters_given_epocher(meters)
        meters.register_meter("loss", AverageValueMeter())
        return meters

    def _call_implementation(self, *, unlabeled_tf_logits, unlabeled_logits_tf, seed, affine_transformer, **kwargs):
        loss = self._criterion.from_logits(unlabeled_logits_tf)
        self.meters["loss"].add(loss.detach())
        return self._weight * loss
