"""`KL_div` / `Entropy` with the interface of contrastyou/losses/kl.py:31-135.

`KL_div.forward(prob, target)` keeps the reference's probability-space signature for arbitrary
callers.  The supervised loss of the epochers -- KL_div(softmax(logits), one_hot(labels))
(epocher.py:317-318) -- goes through `KL_div.from_logits(logits, labels)`: one fused HIP pass
(softmax + log + reduction) forward and one backward, with no one-hot tensor and no `unique()` host
sync.  Mean reduction without class weights runs cy_softmax_kl_*; class weights and the reductions
"sum" and "none" run cy_softmax_wkl_* (csrc/cy_seg_loss.hip), or compose torch ops past 16 classes.
`Entropy.from_logits(logits)` is the same for `Entropy()(logits.softmax(1))`
(semi_seg/hooks/entmin.py:29-30).

`JSD_div(reduction, eps)(*maps)` = Entropy(mean of the maps) - mean of the Entropies (kl.py:142-174) and
`EntropyPrior(reduction="mean", eps)(input_, prior=None)` = log C - KL_div()(prior, input_) (kl.py:63-78) are one
streaming HIP pass each way (csrc/cy_pica.hip); the reference's `simplex` assertions are host syncs and are left out.
"""
from __future__ import annotations

from typing import List, Optional, Union

import torch
from torch import Tensor, nn

from cyhip import ops
from cyhip.functions import EntropyPriorFn, JSDFn, SoftmaxEntropyFn, SoftmaxKLFn, SoftmaxWeightedKLFn

__all__ = ["Entropy", "KL_div", "JSD_div", "EntropyPrior"]

FUSED_KMAX = 16  # classes of the fused kernels (cy_softmax_kl_*, cy_softmax_wkl_*)


def _check_reduction_params(reduction):
    assert reduction in ("mean", "sum", "none"), \
        f"reduction should be in ``'none'`` | ``'mean'`` | ``'sum'``. ``'none'``, given {reduction}"


class Entropy(nn.Module):
    """- sum_c p log(p + eps)"""

    def __init__(self, reduction="mean", eps=1e-16):
        super().__init__()
        _check_reduction_params(reduction)
        self._eps, self._reduction = eps, reduction

    def from_logits(self, logits: Tensor) -> Tensor:
        """== self(logits.softmax(1)); one fused HIP pass each way for the mean reduction"""
        if self._reduction != "mean":
            return self(logits.softmax(1))
        return SoftmaxEntropyFn.apply(logits, float(self._eps))

    def forward(self, input_: Tensor) -> Tensor:
        assert input_.dim() >= 2
        e = -(input_ * (input_ + self._eps).log()).sum(1)
        if self._reduction == "mean":
            return e.mean()
        if self._reduction == "sum":
            return e.sum()
        return e


class KL_div(nn.Module):
    """KL(target, prob) = - sum_c target * log((prob + eps) / (target + eps))"""

    def __init__(self, reduction="mean", eps=1e-16, weight: Union[List[float], Tensor] = None):
        super().__init__()
        _check_reduction_params(reduction)
        self._eps, self._reduction = eps, reduction
        self._weight: Optional[Tensor] = None
        if weight is not None:
            w = torch.as_tensor(weight).float()
            self._weight = w / w.sum() * len(w)
        self._device_weight = {}  # device -> the normalised weights as the kernels read them

    @property
    def fusable(self) -> bool:
        """every weight and reduction has a fused pass (up to 16 classes: `from_logits`)"""
        return True

    def _weight_on(self, device) -> Optional[Tensor]:
        if self._weight is None:
            return None
        if device not in self._device_weight:
            self._device_weight[device] = self._weight.float().to(device).contiguous()
        return self._device_weight[device]

    def from_logits(self, logits: Tensor, labels: Tensor) -> Tensor:
        """== self(logits.softmax(1), one_hot(labels))"""
        if self._reduction == "mean" and self._weight is None:
            return SoftmaxKLFn.apply(logits, labels, float(self._eps))
        C = logits.shape[1]
        if C > FUSED_KMAX:
            onehot = torch.nn.functional.one_hot(labels.long(), C).movedim(-1, 1)
            return self(logits.softmax(1), onehot)
        if self._weight is not None:
            assert len(self._weight) == C, (len(self._weight), C)
        return SoftmaxWeightedKLFn.apply(logits, labels.long(), self._weight_on(logits.device), float(self._eps),
                                         self._reduction)

    def forward(self, prob: Tensor, target: Tensor, **kwargs) -> Tensor:
        b, c, *hwd = target.shape
        kl = -target * torch.log((prob + self._eps) / (target + self._eps))
        if self._weight is not None:
            assert len(self._weight) == c
            shape = [1, c] + [1] * len(hwd)
            kl = kl * self._weight.to(kl.device).view(*shape)
        kl = kl.sum(1)
        if self._reduction == "mean":
            return kl.mean()
        if self._reduction == "sum":
            return kl.sum()
        return kl

    def __repr__(self):
        return f"{self.__class__.__name__}\n, weight={self._weight}"


class EntropyPrior(Entropy):
    """log C - KL_div()(prior, input_) on [n,C] rows, `prior` a [1,C] row (default: uniform) taken as a constant.  Only
    the mean reduction exists; inputs of more than two dimensions fail the reference's own shape assertion, here too."""

    def __init__(self, reduction="mean", eps=1e-16):
        super().__init__(reduction, eps)
        assert reduction == "mean", "only support mean"

    def forward(self, input_: Tensor, prior: Tensor = None) -> Tensor:
        assert input_.dim() >= 2
        C = input_.shape[1]
        if prior is not None:
            assert isinstance(prior, Tensor)
            assert prior.shape == (1, *input_.shape[1:]), (prior.shape, input_.shape)
        assert input_.dim() == 2, f"a prior row of shape [1,{C}] does not match the mean of a {tuple(input_.shape)} input"
        ops.require_gpu(input_, prior)
        if C > ops.PICA_KMAX:
            raise NotImplementedError(f"EntropyPrior runs on up to {ops.PICA_KMAX} classes, got {C}")
        row = None if prior is None else prior.detach().float().reshape(C).contiguous()
        return EntropyPriorFn.apply(input_.float(), row, float(self._eps))


class JSD_div(nn.Module):
    """Entropy(mean of the maps) - mean of the Entropies, each in the given reduction (general Jensen-Shannon divergence
    with equal weights): one fused pass reads the maps once, one backward kernel.  2 to 8 f32 maps of one shape with up
    to 64 classes on dim 1, NCHW or NHWC (or [n,C] rows); anything else raises NotImplementedError."""

    def __init__(self, reduction="mean", eps=1e-16):
        super().__init__()
        _check_reduction_params(reduction)
        self._reduction = reduction
        self._eps = eps
        self._entropy_criterion = Entropy(reduction=reduction, eps=eps)

    def forward(self, *input_: Tensor) -> Tensor:
        assert all(x.shape == input_[0].shape for x in input_), "input tensor should have the same dimension"
        lo, hi = ops.JSD_MAPS
        if not (lo <= len(input_) <= hi) or input_[0].dim() < 2 or input_[0].shape[1] > ops.PICA_KMAX or any(
                x.dtype != torch.float32 for x in input_):
            raise NotImplementedError(
                f"JSD_div runs on {lo} to {hi} float32 maps of up to {ops.PICA_KMAX} classes (NCHW or NHWC), got "
                f"{len(input_)} of shape {tuple(input_[0].shape) if input_ else None} and dtypes "
                f"{[str(x.dtype) for x in input_]}")
        ops.require_gpu(*input_)
        return JSDFn.apply(self._reduction, float(self._eps), *input_)
