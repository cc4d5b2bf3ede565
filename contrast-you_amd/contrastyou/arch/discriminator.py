"""`Discriminator` of the adversarial baseline (contrastyou/arch/discriminator.py:8-43 of the reference): the DCGAN
critic -- four Conv2d(4, 2, 1) and a closing Conv2d(4, 1, 0) to one channel, BatchNorm2d + LeakyReLU(0.2) in between.

`_main` holds the reference's own torch modules, so the state dict (keys, shapes, dtypes), `weights_init` and the
random draws under a seed are the reference's; they are containers only.  `forward` never calls them: the five
convolutions go through `Discriminator.conv` -- by default `cyhip.glue.Conv4x4Fn`, the implicit-GEMM kernels of
csrc/cy_conv4x4.hip (no patch matrix); `conv_im2col` is the `cyhip.glue.Conv2dFn` form (im2col + strided GEMM + col2im)
kept to compare against -- everything else through the kernels of csrc/cy_disc.hip, NHWC f32 from the input to the
score map.

    scores(x)                          the pre-sigmoid map [N, 1, h, w]: what the fused sigmoid + BCE loss takes
    scores_from_logits(image, logits)  scores(cat([image, softmax(logits)], 1)) with the softmax + concat fused
    forward(x)                         sigmoid(scores(x)), like the reference
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from cyhip import ops
from cyhip.functions import BNLeakyReLUFn, LeakyReLUFn, SoftmaxCatFn
from cyhip.glue import Conv2dFn, Conv4x4Fn

__all__ = ["Discriminator", "weights_init", "conv_implicit", "conv_im2col"]


def conv_implicit(x: Tensor, weight: Tensor, stride: int, pad: int) -> Tensor:
    """the bias-free 4 x 4 convolution on the implicit-GEMM kernels (the default of `Discriminator.conv`)"""
    return Conv4x4Fn.apply(x, weight, stride, pad)


def conv_im2col(x: Tensor, weight: Tensor, stride: int, pad: int) -> Tensor:
    """the same convolution through im2col + GEMM + col2im: `Discriminator.conv = staticmethod(conv_im2col)`"""
    return Conv2dFn.apply(x, weight, None, stride, pad)


def weights_init(m):
    """DCGAN initialisation by layer type: N(0, 0.02) convolution weights, N(1, 0.02) BatchNorm weights with zero bias"""
    kind = type(m).__name__
    if "Conv" in kind:
        nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif "BatchNorm" in kind:
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0)


class Discriminator(nn.Module):
    SLOPE = 0.2
    conv = staticmethod(conv_implicit)  # (x, weight, stride, pad) -> y; a class attribute, not an environment switch

    def __init__(self, input_dim, hidden_dim):
        super().__init__()
        self._main = nn.Sequential(
            nn.Conv2d(input_dim, hidden_dim, 4, 2, 1, bias=False),
            nn.LeakyReLU(self.SLOPE, inplace=True),
            nn.Conv2d(hidden_dim, hidden_dim * 2, 4, 2, 1, bias=False),
            nn.BatchNorm2d(hidden_dim * 2),
            nn.LeakyReLU(self.SLOPE, inplace=True),
            nn.Conv2d(hidden_dim * 2, hidden_dim * 4, 4, 2, 1, bias=False),
            nn.BatchNorm2d(hidden_dim * 4),
            nn.LeakyReLU(self.SLOPE, inplace=True),
            nn.Conv2d(hidden_dim * 4, hidden_dim * 8, 4, 2, 1, bias=False),
            nn.BatchNorm2d(hidden_dim * 8),
            nn.LeakyReLU(self.SLOPE, inplace=True),
            nn.Conv2d(hidden_dim * 8, 1, 4, 1, 0, bias=False),
            nn.Sigmoid(),
        )
        self.apply(weights_init)
        self._input_dim = input_dim

    def _trunk(self, x: Tensor, param_grads: bool) -> Tensor:
        m = self._main
        par = (lambda p: p) if param_grads else (lambda p: p.detach())
        x = LeakyReLUFn.apply(self.conv(x, par(m[0].weight), 2, 1), self.SLOPE)
        for conv, bn in ((m[2], m[3]), (m[5], m[6]), (m[8], m[9])):
            x = self.conv(x, par(conv.weight), 2, 1)
            x = BNLeakyReLUFn.apply(x, par(bn.weight), par(bn.bias), bn.running_mean, bn.running_var,
                                    bn.num_batches_tracked, self.training, bn.momentum, bn.eps, self.SLOPE)
        return self.conv(x, par(m[11].weight), 1, 0)

    def scores(self, input_: Tensor, param_grads: bool = True) -> Tensor:
        """the map in front of the sigmoid.  `param_grads=False` runs the same arithmetic on detached parameters: the
        gradient still reaches the input, the weight-gradient GEMMs and the parameter gradients are skipped"""
        ops.require_gpu(input_, self._main[0].weight)
        if input_.dim() != 4 or input_.shape[1] != self._input_dim:
            raise ValueError(f"expected [N, {self._input_dim}, H, W], given {tuple(input_.shape)}")
        return self._trunk(input_, param_grads)

    def scores_from_logits(self, image: Optional[Tensor], logits: Tensor, param_grads: bool = True) -> Tensor:
        """scores(torch.cat([image, logits.softmax(1)], 1)); image None: scores(logits.softmax(1))"""
        ops.require_gpu(image, logits, self._main[0].weight)
        return self.scores(SoftmaxCatFn.apply(image, logits), param_grads)

    def forward(self, input_: Tensor) -> Tensor:
        # (the step never comes here: the epocher takes `scores` into the fused sigmoid + BCE kernel)
        return torch.sigmoid(self.scores(input_))
