"""`MultiCoreKL`: the supervised loss of the multi-prototype recipes, with the interface of
contrastyou/losses/multicore_loss.py:33-60.

The network has `multiplier x true_num_classes` outputs; `groups[c]` lists the output channels (prototypes) of class c.
The loss sums the softmax over each class's channels (`reduced_simplex`) and takes `KL_div` against the one-hot target.

`forward(predict_simplex, onehot_target)` keeps the reference's probability-space signature for arbitrary callers.  The
epochers go through `from_logits(logits, labels)`: when `groups` is the contiguous equal partition of range(K) -- what
main_multicore.py builds with `grouper(range(K), C)` -- and K <= 64, that is one fused HIP pass each way
(cyhip.functions.SoftmaxGroupKLFn: softmax, group sum, log, mean; no softmax, one-hot or reduced tensor in memory).  Any
other grouping composes softmax -> reduced_simplex -> KL_div in torch ops.

The adaptive over-segmented criteria of the reference file (learnable translation matrices) are not built:
main_multicore.py accepts only the "naive" criterion.
"""
from __future__ import annotations

import typing as t
from abc import abstractmethod

import torch
from torch import Tensor, nn

from contrastyou.losses.kl import KL_div
from contrastyou.utils.general import class2one_hot
from cyhip.functions import SoftmaxGroupKLFn

__all__ = ["GeneralOverSegmentedLoss", "MultiCoreKL", "contiguous_partition"]

FUSED_KMAX = 64  # widest row of csrc/cy_group_loss.hip


def contiguous_partition(groups: t.Sequence[t.Sequence[int]]) -> t.Optional[t.Tuple[int, int]]:
    """(K, G) when `groups` is G equal runs [g*m, (g+1)*m) that together are range(K) in order, else None"""
    groups = [list(g) for g in groups]
    if not groups or not groups[0]:
        return None
    m = len(groups[0])
    flat = [int(k) for g in groups for k in g]
    if any(len(g) != m for g in groups) or flat != list(range(len(groups) * m)):
        return None
    return len(flat), len(groups)


class GeneralOverSegmentedLoss(nn.Module):
    kl: KL_div

    @abstractmethod
    def reduced_simplex(self, predict_simplex: Tensor) -> Tensor:
        """[B, K, ...] probabilities over the prototypes -> [B, C, ...] probabilities over the true classes"""


class MultiCoreKL(GeneralOverSegmentedLoss):
    def __init__(self, groups: t.List[t.List[int]]):
        super().__init__()
        self._groups = groups
        self.kl = KL_div()
        self._partition = contiguous_partition(groups)

    @property
    def groups(self) -> t.List[t.List[int]]:
        return self._groups

    def fusable(self, K: int) -> bool:
        return self._partition is not None and self._partition[0] == K and K <= FUSED_KMAX and self.kl.fusable

    def from_logits(self, logits: Tensor, labels: Tensor) -> Tensor:
        """== self(logits.softmax(1), one_hot(labels, len(groups)))"""
        if self.fusable(logits.shape[1]):
            return SoftmaxGroupKLFn.apply(logits, labels, self._partition[1], float(self.kl._eps))
        return self(logits.softmax(1), class2one_hot(labels, len(self._groups)))

    def forward(self, predict_simplex: Tensor, onehot_target: Tensor) -> Tensor:
        return self.kl(self.reduced_simplex(predict_simplex), onehot_target)

    def reduced_simplex(self, predict_simplex: Tensor) -> Tensor:
        return torch.cat([predict_simplex[:, list(g)].sum(1, keepdim=True) for g in self._groups], dim=1)
