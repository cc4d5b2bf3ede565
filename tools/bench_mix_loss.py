#!/usr/bin/env python3
"""Timings of the class-mixing loss kernels of the adaptive over-segmented criteria (csrc/cy_mix_loss.hip) at
(K, C) = (32, 4) and (40, 5) on 16 x 224 x 224 pixels, next to the grouped kernels of `MultiCoreKL`
(csrc/cy_group_loss.hip) on the same logits -- they read the same bytes -- and next to the composition in torch-ROCm ops
the epochers would otherwise run (softmax -> reduced_simplex -> KL_div; reduced arg-max), the two alternating.

The harness is tools/bench_cc.py's: `gpu` = device time of back-to-back executions with the algorithmic bytes over it
(logits read once per pass, the gradient written once), `issue` = host wall time per call.  One line per entry.
"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from bench_cc import DEV, line  # noqa: E402  (puts contrast-you_amd on sys.path)
from cyhip import ops  # noqa: E402
from cyhip.functions import SoftmaxGroupKLFn, SoftmaxMixKLFn  # noqa: E402

EPS = 1e-16


# ---- the reference's formulas on torch ops (losses/multicore_loss.py:78-88, kl.py:112-125, multicore_epocher.py:64-67)
def t_loss(z, t_onehot, T):
    red = (z.softmax(1).moveaxis(1, -1) @ T.softmax(1)).moveaxis(-1, 1)
    return -(t_onehot * torch.log((red + EPS) / (t_onehot + EPS))).sum(1).mean()


def t_argmax(z, M):
    return (z.softmax(1).moveaxis(1, -1) @ M).moveaxis(-1, 1).max(1)[1]


def main():
    print(f"# device {torch.cuda.get_device_name(0)}; f32 logits, NHWC")
    gen = torch.Generator().manual_seed(0)
    n, H, W = 16, 224, 224
    P = n * H * W
    for K, C in ((32, 4), (40, 5)):
        nb = P * K * 4
        z = ops.to_nhwc((torch.randn(n, K, H, W, generator=gen) * 2).to(DEV))
        t = torch.randint(0, C, (n, H, W), generator=gen).to(DEV)
        T = torch.randn(K, C, generator=gen).to(DEV)
        M = T.softmax(1).contiguous()
        onehot = torch.nn.functional.one_hot(t, C).movedim(-1, 1).float()
        g = torch.ones(1, device=DEV)
        tag = f"{n}x{K}x{H}x{W} C={C}"
        print(f"# {tag}: {nb / 1e6:.1f} MB of logits")
        line(f"{tag} mix_kl_fwd (2 launches)", lambda: ops.softmax_mix_kl_fwd(z, t, M, EPS), None, nb)
        line(f"{tag} group_kl_fwd (2 launches)", lambda: ops.softmax_group_kl_fwd(z, t, C, EPS), None, nb)
        line(f"{tag} mix_kl_bwd, dmix (2 launches)", lambda: ops.softmax_mix_kl_bwd(z, t, M, g, EPS, True), None,
             2 * nb)
        line(f"{tag} mix_kl_bwd, no dmix", lambda: ops.softmax_mix_kl_bwd(z, t, M, g, EPS, False), None, 2 * nb)
        line(f"{tag} group_kl_bwd", lambda: ops.softmax_group_kl_bwd(z, t, g, C, EPS), None, 2 * nb)
        line(f"{tag} mix_dice_counts", lambda: ops.mix_dice_counts(z, t, M), lambda: t_argmax(z, M), nb)
        line(f"{tag} group_dice_counts", lambda: ops.group_dice_counts(z, t, C), None, nb)
        zl = z.detach().clone().requires_grad_(True)
        Tl = T.detach().clone().requires_grad_(True)

        def hip_call():
            zl.grad = Tl.grad = None
            SoftmaxMixKLFn.apply(zl, t, Tl.softmax(1), EPS).backward()

        def torch_call():
            zl.grad = Tl.grad = None
            t_loss(zl, onehot, Tl).backward()

        def group_call():
            zl.grad = None
            SoftmaxGroupKLFn.apply(zl, t, C, EPS).backward()

        line(f"{tag} adaptive KL call fwd+bwd (4 launches)", hip_call, torch_call)
        line(f"{tag} MultiCoreKL call fwd+bwd (3 launches)", group_call, None)


if __name__ == "__main__":
    main()
