"""Pseudo-label regulariser (semi_seg/hooks/pseudolabel.py:9-38): weight * MSELoss()(p, one_hot(argmax p)) with
p = softmax(unlabeled_logits_tf) and the one-hot a constant -- one fused HIP pass over the logits each way
(cy_softmax_selfmse_*; cy_softmax_selfmse_row_* on multi-prototype logits, 16 < K <= 64), no probability, label or
one-hot tensor.  The meter receives a device scalar."""
from __future__ import annotations

from torch.nn import MSELoss

from contrastyou.hooks.base import EpocherHook, TrainerHook
from contrastyou.meters import AverageValueMeter, MeterInterface
from cyhip.functions import SoftmaxSelfMSEFn


class PseudoLabelTrainerHook(TrainerHook):

    def __init__(self, name: str, weight: float):
        super().__init__(hook_name=name)
        self._weight = weight
        self._criterion = MSELoss()  # (the reference's attribute; the fused kernel is this criterion, mean reduction)

    def __call__(self):
        return _PLEpocherHook(name=self._hook_name, weight=self._weight, criterion=self._criterion)


class _PLEpocherHook(EpocherHook):
    def __init__(self, name: str, weight: float, criterion) -> None:
        super().__init__(name=name)
        if not isinstance(criterion, MSELoss) or criterion.reduction != "mean":
            raise NotImplementedError(f"the pseudo-label kernel is MSELoss() with mean reduction, given {criterion}")
        self._weight, self._criterion = weight, criterion

    def configure_meters_given_epocher(self, meters: MeterInterface):
        meters = super().configure_meters_given_epocher(meters)
        meters.register_meter("loss", AverageValueMeter())
        return meters

    def _call_implementation(self, *, unlabeled_tf_logits, unlabeled_logits_tf, seed, affine_transformer, **kwargs):
        loss = SoftmaxSelfMSEFn.apply(unlabeled_logits_tf)
        self.meters["loss"].add(loss.detach())
        return self._weight * loss
