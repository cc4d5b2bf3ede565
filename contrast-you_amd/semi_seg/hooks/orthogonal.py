"""The orthogonal-prototype regulariser (semi_seg/hooks/orthogonal.py:12-50 of the reference): the rows of a prototype
matrix -- the live weight of the 1x1 segmentation head, [K, C, 1, 1] -- are pushed towards an orthonormal set by
weight * ((n n^T - I)^2).mean(), n = F.normalize(prototypes).  `OrthoLossFn` (cy_ortho_*) is one launch each way in
place of the reference's normalise, squeeze, matmul, eye, subtract, square and mean with their backward, and the
meter receives the device scalar where the reference synchronises with `.item()`."""
from __future__ import annotations

from torch import Tensor
from torch.nn import functional as F

from contrastyou.hooks.base import EpocherHook, TrainerHook
from contrastyou.meters import AverageValueMeter, MeterInterface
from cyhip.functions import OrthoLossFn


def pairwise_matrix(vec1: Tensor, vec2: Tensor):
    assert vec1.shape == vec2.shape
    assert vec1.dim() == 2
    return vec1 @ vec2.t()


def normalize(vec: Tensor, dim: int = 1):
    return F.normalize(vec, p=2, dim=dim)


class OrthogonalTrainerHook(TrainerHook):

    def __init__(self, *, hook_name: str, prototypes: Tensor, weight: float = 0.0):
        super().__init__(hook_name=hook_name)
        self._weight = weight
        self._prototype_weights = prototypes

    def __call__(self):
        return _OrthogonalEpocherHook(name=self._hook_name, prototypes=self._prototype_weights, weight=self._weight)


class _OrthogonalEpocherHook(EpocherHook):

    def __init__(self, *, name: str, prototypes: Tensor, weight: float) -> None:
        super().__init__(name=name)
        self._prototypes = prototypes
        self._weight = weight

    def configure_meters_given_epocher(self, meters: MeterInterface):
        meters.register_meter("loss", AverageValueMeter())
        return meters

    def _call_implementation(self, **kwargs):
        loss = OrthoLossFn.apply(self._prototypes)
        self.meters["loss"].add(loss.detach())
        return loss * self._weight
