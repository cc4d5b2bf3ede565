"""PICA losses with the interface of contrastyou/losses/pica_loss.py:10-85, restated as the reference writes them,
quirks included:

    PUILoss(lamda=2.0)(x, y)                         on [N,K] rows
        pui_ij  = sum_n x_ni y_nj / (max(|x_.i|, 1e-12) max(|y_.j|, 1e-12))
        loss_ce = mean_i [logsumexp_j pui_ij - pui_ii]
        loss_ne = log K + sum_i p_i log p_i,  p = x.mean(0)                      (no eps)
    PUISegLoss(lamda=2.0, padding=3)(x_out, x_tf_out) on [n,k,H,W] maps
        the displaced joint of compute_joint_2D; minus its global minimum plus 1e-16 (not 1e-8); normalised per
        displacement; always symmetrised; the mean over the T*T displacements gives P[k][k];
        loss_ce = -(1/k^2) sum_i log(P_ii + 1e-16)
        loss_ne = log M + sum_m p_m log p_m over the PERMUTED tensor: p_m = (1/k) sum_c x_out[., c, .] is the per-pixel
        mean over the classes, M = n H W.  For simplex inputs it is a constant, but its gradient with respect to the
        probabilities, lamda (log p_m + 1) / k on every class of a pixel, is not zero.
    both return loss_ce + lamda * loss_ne.

The joints come from the HIP joint kernels (csrc/cy_mi.hip), the rest from one finishing block and the streaming kernels
of csrc/cy_pica.hip.  The reference's `simplex` assertion in PUILoss is a host sync and is left out.
"""
from __future__ import annotations

from torch import Tensor, nn

from cyhip import ops
from cyhip.functions import PUIFn, PUISegFn

__all__ = ["PUILoss", "PUISegLoss"]


class PUILoss(nn.Module):
    """classification loss"""

    def __init__(self, lamda=2.0):
        super().__init__()
        self.lamda = lamda

    def forward(self, x: Tensor, y: Tensor) -> Tensor:
        assert x.shape == y.shape and x.dim() == 2, "Inputs are required to have same shape"
        ops.require_gpu(x, y)
        return PUIFn.apply(x.float().contiguous(), y.float().contiguous(), float(self.lamda))


class PUISegLoss(nn.Module):

    def __init__(self, lamda=2.0, padding=3):
        super().__init__()
        self.lamda = lamda
        self.padding = int(padding)

    def forward(self, x_out: Tensor, x_tf_out: Tensor) -> Tensor:
        assert x_out.shape == x_tf_out.shape and x_out.dim() == 4, "Inputs are required to have same shape"
        ops.require_gpu(x_out, x_tf_out)
        a = x_out.float().permute(0, 2, 3, 1).contiguous()
        b = x_tf_out.float().permute(0, 2, 3, 1).contiguous()
        return PUISegFn.apply(a, b, self.padding, float(self.lamda))
