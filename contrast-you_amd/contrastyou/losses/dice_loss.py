"""`make_one_hot`, `BinaryDiceLoss`, `DiceLoss` with the interface of contrastyou/losses/dice_loss.py:13-105.

`forward(predict, target)` keeps the reference's probability-space signature for arbitrary callers, in torch ops.
The supervised loss of the epochers -- DiceLoss(softmax(logits), one_hot(labels)) -- goes through
`DiceLoss.from_logits(logits, labels)`: one fused HIP pass over the logits and a one-block finalize forward, one pass
backward (cy_softmax_dice_*, csrc/cy_seg_loss.hip), with no softmax, one-hot or per-class tensor.

Per image n and class c:  num = sum p_c t_c + smooth,  den = sum (p_c^p + t_c^p) + smooth,  L_nc = 1 - num / den
(no factor 2);  loss = (1 / C) sum_{c != ignore_index} reduction_n(L_nc): the divisor counts the ignored class too
(dice_loss.py:105).

`DiceLoss(weight=...)` cannot run in the reference: dice_loss.py:102 reads `self.weights` where the attribute is
`weight`, an AttributeError on the first class.  There is nothing to be in parity with, so it is refused here at
construction.
"""
from __future__ import annotations

import torch
from torch import Tensor, nn

from cyhip.functions import SoftmaxDiceFn

__all__ = ["make_one_hot", "BinaryDiceLoss", "DiceLoss"]

FUSED_KMAX = 16  # classes of cy_softmax_dice_*


def make_one_hot(input: Tensor, num_classes: int) -> Tensor:
    """class indices [N, 1, *] -> f32 one-hot [N, num_classes, *] (on the indices' device)"""
    shape = list(input.shape)
    shape[1] = num_classes
    return torch.zeros(shape, device=input.device).scatter_(1, input.long(), 1)


class BinaryDiceLoss(nn.Module):
    """1 - (sum x y + smooth) / (sum x^p + sum y^p + smooth) per sample, `predict` and `target` of shape [N, *];
    reduction "mean" / "sum" over the batch, "none" returns [N]"""

    def __init__(self, smooth=1, p=2, reduction="mean"):
        super().__init__()
        self.smooth, self.p, self.reduction = smooth, p, reduction

    def forward(self, predict: Tensor, target: Tensor) -> Tensor:
        assert predict.shape[0] == target.shape[0], "predict & target batch size don't match"
        predict = predict.contiguous().view(predict.shape[0], -1)
        target = target.contiguous().view(target.shape[0], -1)
        num = torch.sum(torch.mul(predict, target), dim=1) + self.smooth
        den = torch.sum(predict.pow(self.p) + target.pow(self.p), dim=1) + self.smooth
        loss = 1 - num / den
        if self.reduction == "mean":
            return loss.mean()
        if self.reduction == "sum":
            return loss.sum()
        if self.reduction == "none":
            return loss
        raise Exception("Unexpected reduction {}".format(self.reduction))


class DiceLoss(nn.Module):
    """soft Dice loss of a simplex `predict` [N, C, *] against a one-hot `target` of the same shape; `ignore_index`: a
    class left out of the sum (not of the divisor C); the other keywords are BinaryDiceLoss's"""

    def __init__(self, weight=None, ignore_index=None, **kwargs):
        super().__init__()
        if weight is not None:
            raise NotImplementedError(
                "DiceLoss(weight=...): the reference cannot run it either (contrastyou/losses/dice_loss.py:102 reads "
                "`self.weights`, the attribute is `weight`: an AttributeError), so there is no behaviour to match")
        self.kwargs = kwargs
        self.weight = weight
        self.ignore_index = ignore_index
        self._binary = BinaryDiceLoss(**kwargs)

    def _fused(self, K: int) -> bool:
        b = self._binary
        return b.p in (1, 2) and K <= FUSED_KMAX and b.reduction in ("mean", "sum", "none")

    def from_logits(self, logits: Tensor, labels: Tensor) -> Tensor:
        """== self(logits.softmax(1), one_hot(labels)), labels [N, *] integer"""
        C = logits.shape[1]
        if logits.dim() != 4 or not self._fused(C):
            return self(logits.softmax(1), make_one_hot(labels.unsqueeze(1), C))
        b = self._binary
        return SoftmaxDiceFn.apply(logits, labels.long(), int(b.p), float(b.smooth), self.ignore_index, b.reduction)

    def forward(self, predict: Tensor, target: Tensor) -> Tensor:
        assert predict.shape == target.shape, "predict & target shape do not match"
        dice, total_loss = self._binary, 0
        for i in range(target.shape[1]):
            if i != self.ignore_index:
                total_loss = total_loss + dice(predict[:, i], target[:, i])
        return total_loss / target.shape[1]
