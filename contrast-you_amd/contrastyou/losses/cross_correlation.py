"""`CCLoss`: local (windowed) normalised cross-correlation of two single-channel maps, with the interface of
contrastyou/losses/cross_correlation.py:10-74.

    loss = -mean(cross^2 / (I_var * J_var))   over zero-padded k x k windows, each term clamped at eps from below

The reference evaluates it with five `conv2d` calls and ~20 elementwise ops; here forward and backward are the
tile kernels of csrc/cy_cc.hip (cyhip.functions.CCLossFn): two launches forward, one backward, nothing stored
between them but the two maps.
"""
from __future__ import annotations

import typing as t

import numpy as np
import torch
from torch import Tensor, nn

from cyhip.functions import CCLossFn

__all__ = ["CCLoss"]


class CCLoss(nn.Module):
    """
    Local (over window) normalized cross correlation loss.
    """

    def __init__(self, win: t.Tuple[int, int], *, eps: float = 1e-5):
        super().__init__()
        win = tuple(int(w) for w in win)
        # an even window changes the reference's output size (pad = k // 2 on both sides) and appears in no config
        if len(win) != 2 or win[0] != win[1] or win[0] % 2 == 0 or not 3 <= win[0] <= 15:
            raise NotImplementedError(f"CCLoss: window {win} is not supported (square, odd, 3 ... 15)")
        self.win = win
        self.register_buffer("_sum_filt", torch.ones([1, 1, *win]))
        self.win_size = np.prod(win)
        self.eps = eps

    def __call__(self, y_true: Tensor, y_pred: Tensor) -> Tensor:
        ndims = y_true.ndim - 2
        assert ndims in [1, 2, 3], "volumes should be 1 to 3 dimensions. found: %d" % ndims
        if ndims != 2:
            raise NotImplementedError("CCLoss: the HIP kernels take [n, 1, H, W] maps")
        if y_true.shape[1] != 1 or y_pred.shape[1] != 1:  # what conv2d with the [1, 1, k, k] filter raises
            raise RuntimeError(f"CCLoss expects single-channel inputs, got {tuple(y_true.shape)} and "
                               f"{tuple(y_pred.shape)}")
        if y_true.shape != y_pred.shape:
            raise RuntimeError(f"CCLoss: shapes differ, {tuple(y_true.shape)} and {tuple(y_pred.shape)}")
        return CCLossFn.apply(y_true, y_pred, self.win[0], float(self.eps))
