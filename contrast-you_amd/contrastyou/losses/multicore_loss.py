"""The over-segmented ("multicore") supervised criteria, with the interface of
contrastyou/losses/multicore_loss.py:16-149.

The network has K outputs (prototypes) for C < K true classes.  Every criterion maps the softmax over the prototypes to
probabilities over the true classes (`reduced_simplex`) and takes `KL_div` against the one-hot target.

`MultiCoreKL(groups)`: `groups[c]` lists the prototypes of class c and the map is their sum.  When `groups` is the
contiguous equal partition of range(K) -- what main_multicore.py builds with `grouper(range(K), C)` -- and K <= 64,
`from_logits` is one fused HIP pass each way (cyhip.functions.SoftmaxGroupKLFn); any other grouping composes
softmax -> reduced_simplex -> KL_div in torch ops.

`AdaptiveOverSegmentedLoss`, `StricterAdaptiveOverSegmentedLoss`, `StricterAdaptiveOverSegmentedLossWithMI`: the map is
a learnable K x C "translation matrix" T, `reduced = p @ softmax(T, 1)`.  Adaptive adds an entropy penalty on
softmax(T, 1); Stricter pins the first C prototypes to their classes (a fixed 30 * eye(C) above the learnable
(K - C) x C rows); WithMI adds `mi_weight * IIDLoss()(S, S)[0]`, S = softmax(translate_matrix, 1), where there is
anything to learn.  Their members:
    forward(predict_simplex, onehot_target), reduced_simplex(predict_simplex)   probability space, plain torch ops
    mix()                     the K x C matrix softmax(T, 1), with autograd history
    kl_from_logits(z, labels) the KL term alone (the eval epocher's `true_loss`)
    kl_and_loss_from_logits   both from one pass over the logits; output_num_classes: the true class count C
    from_logits(z, labels)    == forward(z.softmax(1), one_hot(labels)): kl_from_logits + the criterion's extra terms
For K <= 64 and C <= 16 `kl_from_logits` is cyhip.functions.SoftmaxMixKLFn -- the logits are read once each way, no
softmax, one-hot or reduced tensor is formed, and dL/dmix comes out of the backward kernel and flows on to T through
the softmax of the (at most 1024-element) matrix in torch ops.  Wider shapes compose in probability space.
"""
from __future__ import annotations

import typing as t
from abc import abstractmethod

import torch
from torch import Tensor, nn

from contrastyou.losses.discreteMI import IIDLoss
from contrastyou.losses.kl import Entropy, KL_div
from contrastyou.utils.general import class2one_hot
from cyhip.functions import SoftmaxGroupKLFn, SoftmaxMixKLFn

__all__ = ["GeneralOverSegmentedLoss", "MultiCoreKL", "contiguous_partition", "GradientReverse", "scale_grad",
           "AdaptiveOverSegmentedLoss", "StricterAdaptiveOverSegmentedLoss", "StricterAdaptiveOverSegmentedLossWithMI"]

FUSED_KMAX = 64  # widest row of csrc/cy_group_loss.hip, csrc/cy_mix_loss.hip
FUSED_CMAX = 16  # most true classes of csrc/cy_mix_loss.hip


class GradientReverse(torch.autograd.Function):
    """identity; on the way back the gradient is multiplied by the class-wide `scale` that `scale_grad` last set"""
    scale = 1.0

    @staticmethod
    def forward(ctx, tensor: Tensor) -> Tensor:
        return tensor.view_as(tensor)

    @staticmethod
    def backward(ctx, grad: Tensor) -> Tensor:
        return grad * GradientReverse.scale


def scale_grad(x: Tensor, scale: float = 1.0) -> Tensor:
    """x with its gradient scaled by `scale` (one scale for the whole process, read when the gradient passes)"""
    GradientReverse.scale = float(scale)
    return GradientReverse.apply(x)


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


class _MixedOverSegmentedLoss(GeneralOverSegmentedLoss):
    """what the criteria with a translation matrix share: the parameter `_translate_matrix` (the only entry of the
    state dict) and everything downstream of `translate_matrix`, the [K, C] logits of the prototype -> class map"""

    def __init__(self, K: int, C: int, learnable_rows: int, device, init) -> None:
        super().__init__()
        self.kl = KL_div()
        self._input_num_classes, self._output_num_classes = int(K), int(C)
        self._translate_matrix = nn.Parameter(init(learnable_rows, int(C), device=device))

    @property
    def input_num_classes(self) -> int:
        return self._input_num_classes

    @property
    def output_num_classes(self) -> int:
        return self._output_num_classes

    @property
    def translate_matrix(self) -> Tensor:
        return self._translate_matrix

    def mix(self) -> Tensor:
        """[K, C] = softmax(translate_matrix, 1), with autograd history"""
        return scale_grad(self.translate_matrix.softmax(1), 1)

    def reduced_simplex(self, predict_simplex: Tensor) -> Tensor:
        return (predict_simplex.movedim(1, -1) @ self.mix()).movedim(-1, 1)

    def fusable(self, K: int) -> bool:
        return (K == self._input_num_classes and K <= FUSED_KMAX and self._output_num_classes <= FUSED_CMAX
                and self.kl.fusable)

    def extra_terms(self) -> t.Optional[Tensor]:
        """what the criterion adds to the KL term (None: nothing)"""
        return None

    def kl_from_logits(self, logits: Tensor, labels: Tensor) -> Tensor:
        """== self.kl(self.reduced_simplex(logits.softmax(1)), one_hot(labels))"""
        if self.fusable(logits.shape[1]):
            return SoftmaxMixKLFn.apply(logits, labels, self.mix(), float(self.kl._eps))
        return self.kl(self.reduced_simplex(logits.softmax(1)), class2one_hot(labels, self._output_num_classes))

    def kl_and_loss_from_logits(self, logits: Tensor, labels: Tensor) -> t.Tuple[Tensor, Tensor]:
        """(the KL term, the criterion's loss = the KL term + its extra terms) from one pass over the logits"""
        kl, extra = self.kl_from_logits(logits, labels), self.extra_terms()
        return kl, kl if extra is None else kl + extra

    def from_logits(self, logits: Tensor, labels: Tensor) -> Tensor:
        """== self(logits.softmax(1), one_hot(labels))"""
        return self.kl_and_loss_from_logits(logits, labels)[1]

    def forward(self, predict_simplex: Tensor, onehot_target: Tensor) -> Tensor:
        kl, extra = self.kl(self.reduced_simplex(predict_simplex), onehot_target), self.extra_terms()
        return kl if extra is None else kl + extra


class AdaptiveOverSegmentedLoss(_MixedOverSegmentedLoss):
    """T is a free K x C parameter (standard normal at the start); the loss adds
    entropy_decay * Entropy(softmax(T, 1))"""

    def __init__(self, input_num_classes: int, output_num_classes: int, device: str, entropy_decay=1e-3) -> None:
        super().__init__(input_num_classes, output_num_classes, input_num_classes, device, torch.randn)
        self.entropy = Entropy()
        self._entropy_decay = entropy_decay

    def extra_terms(self) -> Tensor:
        return self._entropy_decay * self.entropy(self._translate_matrix.softmax(1))


class StricterAdaptiveOverSegmentedLoss(_MixedOverSegmentedLoss):
    """the first C prototypes are pinned to their classes by a fixed 30 * eye(C); only the other K - C rows (zero at the
    start) are learnable.  The diagonal is a plain attribute: not in the state dict, not moved by `.to()`."""

    def __init__(self, input_num_classes: int, output_num_classes: int, device: str, **kwargs) -> None:
        assert input_num_classes >= output_num_classes, \
            f"{input_num_classes} prototypes cannot cover {output_num_classes} classes"
        super().__init__(input_num_classes, output_num_classes, input_num_classes - output_num_classes, device,
                         torch.zeros)
        self._diagonal_matrix = 30.0 * torch.eye(self._output_num_classes, device=device)

    @property
    def needs_optimize(self) -> bool:
        return self._translate_matrix.numel() > 0

    @property
    def translate_matrix(self) -> Tensor:
        if not self.needs_optimize:
            return self._diagonal_matrix
        return torch.cat((self._diagonal_matrix, self._translate_matrix), dim=0)


class StricterAdaptiveOverSegmentedLossWithMI(StricterAdaptiveOverSegmentedLoss):
    """adds mi_weight * IIDLoss()(S, S)[0], S = softmax(translate_matrix, 1), where there is something to learn"""

    def __init__(self, input_num_classes: int, output_num_classes: int, device: str, *, mi_weight: float,
                 **kwargs) -> None:
        super().__init__(input_num_classes, output_num_classes, device, **kwargs)
        self._mi = IIDLoss()
        self._mi_weight = mi_weight

    def extra_terms(self) -> t.Optional[Tensor]:
        if not self.needs_optimize:
            return None
        simplex = self.translate_matrix.softmax(1)
        return self._mi_weight * self._mi(simplex, simplex)[0]
