"""Discrete mutual-information (IIC) and IMSAT losses with the interface of
contrastyou/losses/discreteMI.py:20-170,201-297:

    IIDLoss(lamb)(x_out, x_tf_out)                 -> (loss, loss_no_lamb, p_i_j)   on [n,k] simplexes
    IIDSegmentationLoss(lamda, padding, eps, symmetric)(x_out, x_tf_out, mask=None) -> loss
                                                                                  on [n,k,H,W] maps
    compute_joint / compute_joint_2D / compute_joint_2D_with_padding_zeros
    imsat_with_entropy(prediction)                 -> (marginal entropy, mean conditional entropy)
    imsat_loss(prediction, lamda)                  -> conditional - lamda * marginal
    IMSATLoss(lamda, eps)(x_out, x_tf_out=None)    -> imsat_loss, or the mean of the two views'   on [n,k] simplexes
    IMSATDynamicWeight(lamda, use_dynamic, eps)(x_out) -> -w * marginal + conditional, w a buffer that follows
                                                      log k - marginal
    IIDSegmentationSmallPathLoss(lamda, padding, eps, patch_size)(x_out, x_tf_out, mask=None) -> the mean of
                                                      IIDSegmentationLoss over square patches (discreteMI.py:173-198)
    patch_generator(feature_map, patch_size, step_size) / patch_origins(L, p, s)   (discreteMI.py:264-272)

The k x k (or (2p+1)^2 x k x k) joint is a contraction over all n*H*W pixels -- HBM-bound, k = 20 --
done by the HIP joint kernels; the loss on the joint and its gradient come from one single-block
kernel (csrc/cy_mi.hip).  Inputs must be probability maps; the reference's `simplex()` assertion is a
host sync and is evaluated on demand by `validate()`.

The IMSAT family is one streaming pass over the [rows][k] probabilities (csrc/cy_imsat.hip): it yields the two
entropies as device scalars and every combination above is formed from them with ordinary tensor ops.  Its entropies
use eps = 1e-8, the module-level `entropy_criterion` of semi_seg/hooks/midl.py:13; the `eps` argument of the two
classes is kept and, as in the reference, never read.  The reference's `assert simplex(...)` calls in `IMSATLoss` and
`IMSATDynamicWeight` are host syncs and are left out; the dynamic weight is updated on the device.
"""
from __future__ import annotations

import math
import sys
from typing import Tuple

import torch
from torch import Tensor, nn

from cyhip import ops
from cyhip.functions import IIDFn, IIDPatchFn, IMSATFn, IMSATPairFn

__all__ = ["IIDLoss", "IIDSegmentationLoss", "compute_joint", "compute_joint_2D",
           "compute_joint_2D_with_padding_zeros", "IMSATLoss", "IMSATDynamicWeight", "imsat_loss", "imsat_with_entropy",
           "IIDSegmentationSmallPathLoss", "patch_generator", "patch_origins"]


def _nhwc_f32(x: Tensor) -> Tensor:
    """[n,k,H,W] (any memory format) -> contiguous f32 [n,H,W,k] buffer (no copy for NHWC f32)"""
    x = x if x.dtype == torch.float32 else x.float()
    return x.permute(0, 2, 3, 1).contiguous()


class IIDLoss(nn.Module):

    def __init__(self, lamb: float = 1.0, eps: float = sys.float_info.epsilon):
        super().__init__()
        self.lamb, self.eps = float(lamb), float(eps)

    def forward(self, x_out: Tensor, x_tf_out: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
        assert x_out.dim() == 2 and x_out.shape == x_tf_out.shape, (x_out.shape, x_tf_out.shape)
        ops.require_gpu(x_out, x_tf_out)
        n, k = x_out.shape
        a = x_out.float().contiguous().view(n, 1, 1, k)
        b = x_tf_out.float().contiguous().view(n, 1, 1, k)
        loss, loss_no_lamb, P = IIDFn.apply(a, b, 2, 0, True, self.lamb, 1e-10)  # the reference hard-codes 1e-10
        return loss, loss_no_lamb, P.view(k, k)


class IIDSegmentationLoss(nn.Module):

    def __init__(self, lamda=1.0, padding=0, eps: float = 1e-5, symmetric: bool = False) -> None:
        super().__init__()
        if padding < 0:
            raise ValueError(padding)
        self.lamda, self.padding, self._eps, self.symmetric = lamda, int(padding), eps, symmetric
        self._p_i_j = None

    def forward(self, x_out: Tensor, x_tf_out: Tensor, mask: Tensor = None) -> Tensor:
        assert x_out.shape == x_tf_out.shape and x_out.dim() == 4, (x_out.shape, x_tf_out.shape)
        ops.require_gpu(x_out, x_tf_out)
        if mask is not None:
            x_out, x_tf_out = x_out * mask, x_tf_out * mask
        a, b = _nhwc_f32(x_out), _nhwc_f32(x_tf_out)
        mode = 0 if self.padding == 0 else 1
        loss, _, P = IIDFn.apply(a, b, mode, self.padding, bool(self.symmetric), float(self.lamda), float(self._eps))
        self._p_i_j = P[0]
        return loss

    def get_joint_matrix(self):
        if self._p_i_j is None:
            raise RuntimeError()
        return self._p_i_j.detach().cpu().numpy()


def patch_origins(L: int, p: int, s: int):
    """the origins of the patches of size p, step s, along an axis of length L (discreteMI.py:266-269): the multiples
    of s below L - p, then max(L - p, 0).  A patch is clipped to the axis, so L <= p gives the one origin 0."""
    return list(range(0, L - p, s)) + [max(L - p, 0)]


def patch_generator(feature_map, patch_size=(32, 32), step_size=(16, 16)):
    """the views feature_map[:, :, h0:h0+ph, w0:w0+pw] clipped to the map, rows first (discreteMI.py:264-272)"""
    b, c, h, w = feature_map.shape
    for _h in patch_origins(h, patch_size[0], step_size[0]):
        for _w in patch_origins(w, patch_size[1], step_size[1]):
            yield feature_map[:, :, _h:min(_h + patch_size[0], h), _w:min(_w + patch_size[1], w)]


class IIDSegmentationSmallPathLoss(IIDSegmentationLoss):
    """The mean over square patches (side patch_size, step patch_size // 2, `patch_origins`) of IIDSegmentationLoss on
    the patch, never symmetric (discreteMI.py:173-198).  The reference loops over the patches in Python; here all joints
    come from one launch (the zero padding of a displaced read is at the patch border, as a conv2d on the slice has it),
    one block per patch forms the losses and a fixed-order mean follows (csrc/cy_mi.hip).

    `mask`: the reference multiplies the slice views in place, which alters the caller's tensors and multiplies a pixel
    of overlapping patches once per patch.  Here the mask is applied out of place, once per map, before the kernels:
    the same value for 0/1 masks.  The reference's `torch.isnan` check of the patch losses is a host sync and is left
    out of `forward`, like the `simplex()` assertions of this module."""

    def __init__(self, lamda=1.0, padding=7, eps: float = sys.float_info.epsilon, patch_size=32) -> None:
        super().__init__(lamda, padding, eps)
        self._patch_size = (int(patch_size), int(patch_size))
        self._step_size = (int(patch_size) // 2, int(patch_size) // 2)

    def forward(self, x_out: Tensor, x_tf_out: Tensor, mask: Tensor = None) -> Tensor:
        assert x_out.shape == x_tf_out.shape and x_out.dim() == 4, (x_out.shape, x_tf_out.shape)
        ops.require_gpu(x_out, x_tf_out)
        if mask is not None:
            x_out, x_tf_out = x_out * mask, x_tf_out * mask
        a, b = _nhwc_f32(x_out), _nhwc_f32(x_tf_out)
        loss, self._patch_losses, P = IIDPatchFn.apply(a, b, self.padding, self._patch_size[0], float(self.lamda),
                                                       float(self._eps))
        self._p_i_j = P[0, 0]  # the first patch (origin (0, 0)), displacement index 0
        return loss

    def get_joint_matrix(self):
        """the [k,k] joint of the FIRST patch (origin (0, 0)) at displacement index 0"""
        return super().get_joint_matrix()

    def __repr__(self):
        return f"{self.__class__.__name__} with patch_size={self._patch_size} and padding={self.padding}."


@torch.no_grad()
def compute_joint(x_out: Tensor, x_tf_out: Tensor, symmetric=True) -> Tensor:
    """[n,k] x2 -> normalised (optionally symmetrised) k x k joint (discreteMI.py:201-222); no grad"""
    n, k = x_out.shape
    J = ops.joint_fwd(x_out.float().contiguous(), x_tf_out.float().contiguous(), n, 1, 1, k, 0, False)
    _, P, _ = ops.iid_loss(J, 2, bool(symmetric), 1.0, 1e-10, want_grad=False)
    return P.view(k, k)


@torch.no_grad()
def compute_joint_2D(x_out: Tensor, x_tf_out: Tensor, *, symmetric: bool = True, padding: int = 0) -> Tensor:
    """[n,k,H,W] x2 -> [T,T,k,k] displaced joint, T = 2*padding+1 (discreteMI.py:225-243); no grad"""
    n, k, H, W = x_out.shape
    J = ops.joint_fwd(_nhwc_f32(x_out), _nhwc_f32(x_tf_out), n, H, W, k, padding, False)
    _, P, _ = ops.iid_loss(J, 1, bool(symmetric), 1.0, 1e-5, want_grad=False)
    T = 2 * padding + 1
    return P.view(T, T, k, k)


@torch.no_grad()
def compute_joint_2D_with_padding_zeros(x_out: Tensor, x_tf_out: Tensor, *, symmetric: bool = True) -> Tensor:
    """[n,k,H,W] x2 -> [1,1,k,k] (discreteMI.py:246-261); no grad"""
    n, k, H, W = x_out.shape
    J = ops.joint_fwd(_nhwc_f32(x_out), _nhwc_f32(x_tf_out), n, H, W, k, 0, True)
    _, P, _ = ops.iid_loss(J, 0, bool(symmetric), 1.0, 1e-5, want_grad=False)
    return P.view(1, 1, k, k)


def imsat_with_entropy(prediction: Tensor) -> Tuple[Tensor, Tensor]:
    """[n,k] simplexes or an [n,k,H,W] map -> (entropy of the mean row, mean entropy of the rows)
    (discreteMI.py:287-297)"""
    return IMSATFn.apply(prediction)


def imsat_loss(prediction: Tensor, lamda: float = 1.0) -> Tensor:
    """-(lamda * marginal - conditional) (discreteMI.py:275-284)"""
    marginal, conditional = IMSATFn.apply(prediction)
    return conditional - marginal * lamda


class IMSATLoss(nn.Module):

    def __init__(self, lamda: float = 1.0, eps: float = sys.float_info.epsilon):
        super().__init__()
        self.eps = float(eps)
        self.lamda = float(lamda)

    def forward(self, x_out: Tensor, x_tf_out: Tensor = None):
        assert len(x_out.shape) == 2, x_out.shape
        self.x_out = x_out
        self.x_tf_out = x_out if x_tf_out is None else x_tf_out
        if x_tf_out is None:
            return imsat_loss(x_out, lamda=self.lamda)
        marg1, cond1, marg2, cond2, _ = IMSATPairFn.apply(x_out, x_tf_out)  # one pass over both; the MSE is not used
        return 0.5 * ((cond1 - marg1 * self.lamda) + (cond2 - marg2 * self.lamda))

    @torch.no_grad()
    def get_joint_matrix(self):
        """x_out^T x_tf_out / n as a numpy [k,k] array: compute_joint_2D_with_padding_zeros(symmetric=False) on [n,k]"""
        a, b = self.x_out.detach().float().contiguous(), self.x_tf_out.detach().float().contiguous()
        n, k = a.shape
        return ops.joint_fwd(a, b, n, 1, 1, k, 0, True).view(k, k).cpu().numpy()


class IMSATDynamicWeight(IMSATLoss):

    def __init__(self, lamda: float = 1.0, use_dynamic: bool = True, eps: float = sys.float_info.epsilon):
        super().__init__(lamda, eps)
        self.register_buffer("dynamic_weight", torch.tensor(lamda))
        self.use_dynamic_weight = use_dynamic

    def forward(self, x_out: Tensor, **kwargs):
        self.dynamic_weight = self.dynamic_weight.to(x_out.device).to(x_out.dtype)
        assert len(x_out.shape) == 2, x_out.shape
        self.x_out = self.x_tf_out = x_out
        marg, cond = imsat_with_entropy(x_out)
        mi = self.dynamic_weight * marg * -1.0 + cond
        if self.use_dynamic_weight:
            with torch.no_grad():  # on the device: the weight is never read on the host
                self.dynamic_weight = self.dynamic_weight + (math.log(x_out.shape[1]) - marg.detach()) * 0.01
        return mi
