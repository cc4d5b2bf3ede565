#!/usr/bin/env python3
"""Timings of the pixel-wise regulariser kernels (csrc/cy_pixel_reg.hip: entropy-min, pseudo-label, UA-MT) at
16 x 4 x 224 x 224 and 32 x 2 x 224 x 224, and of one loss call (forward + backward through autograd) of each kind next
to the same formulas composed from torch-ROCm ops on the same GPU in the same process, the two alternating.

The harness is tools/bench_cc.py's: `gpu` = device time of back-to-back executions with the algorithmic bytes over it
(logits read once per pass, the gradient written once), `issue` = host wall time per call.  One line per entry.
"""
import math
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
from bench_cc import DEV, line  # noqa: E402  (puts contrast-you_amd on sys.path)
from cyhip import ops  # noqa: E402
from cyhip.functions import SoftmaxEntropyFn, SoftmaxSelfMSEFn, UAMTLossFn  # noqa: E402

EPS = 1e-16


# ---- the reference's formulas on torch ops (entmin.py:29-30, pseudolabel.py:30-36, mt.py:242-248,266-267)
def t_entropy(z):
    p = z.softmax(1)
    return -(p * (p + EPS).log()).sum(1).mean()


def t_selfmse(z):
    p = z.softmax(1)
    with torch.no_grad():
        onehot = F.one_hot(p.max(1)[1], z.shape[1]).movedim(-1, 1).float()
    return F.mse_loss(p, onehot)


def t_uamt(zt, zs, thr, hard):
    s = zs.softmax(1)
    with torch.no_grad():
        t = zt.softmax(1)
        ent = -(t * (t + EPS).log()).sum(1)
        if hard:
            t = F.one_hot(t.argmax(1), zt.shape[1]).movedim(-1, 1).float()
    loss = F.mse_loss(t, s, reduction="none").mean(1)
    mask = (ent < thr).float()
    return (loss * mask).mean() / (mask.mean().item() + 1e-2)  # (the reference's host sync)


def fwd_bwd(fn, z):
    def run():
        z.grad = None
        fn(z).backward()
    return run


def main():
    print(f"# device {torch.cuda.get_device_name(0)}; f32 logits, NHWC")
    gen = torch.Generator().manual_seed(0)
    for n, K in ((16, 4), (32, 2)):
        H = W = 224
        P = n * H * W
        nb = P * K * 4
        thr = 0.85 * math.log(K)
        zs = ops.to_nhwc((torch.randn(n, K, H, W, generator=gen) * 2).to(DEV))
        zt = ops.to_nhwc((torch.randn(n, K, H, W, generator=gen) * 2).to(DEV))
        g = torch.ones(1, device=DEV)
        res = ops.uamt_mse_fwd(zt, zs, thr, False)
        tag = f"{n}x{K}x{H}x{W}"
        print(f"# {tag}: {nb / 1e6:.1f} MB per logit tensor")
        line(f"{tag} softmax_entropy_fwd (2 launches)", lambda: ops.softmax_entropy_fwd(zs, EPS), None, nb)
        line(f"{tag} softmax_entropy_bwd", lambda: ops.softmax_entropy_bwd(zs, g, EPS), None, 2 * nb)
        line(f"{tag} softmax_selfmse_fwd (2 launches)", lambda: ops.softmax_selfmse_fwd(zs), None, nb)
        line(f"{tag} softmax_selfmse_bwd", lambda: ops.softmax_selfmse_bwd(zs, g), None, 2 * nb)
        for hard in (False, True):
            line(f"{tag} uamt_mse_fwd hard {int(hard)} (2 launches)", lambda: ops.uamt_mse_fwd(zt, zs, thr, hard), None,
                 2 * nb)
            line(f"{tag} uamt_mse_bwd hard {int(hard)}", lambda: ops.uamt_mse_bwd(zt, zs, res, g, thr, hard), None,
                 3 * nb)
        z = zs.detach().clone().requires_grad_(True)
        line(f"{tag} entropy-min call fwd+bwd (3 launches)", fwd_bwd(lambda t: SoftmaxEntropyFn.apply(t, EPS), z),
             fwd_bwd(t_entropy, z))
        line(f"{tag} pseudo-label call fwd+bwd (3 launches)", fwd_bwd(SoftmaxSelfMSEFn.apply, z), fwd_bwd(t_selfmse, z))
        for hard in (False, True):
            line(f"{tag} UA-MT loss call hard {int(hard)} fwd+bwd (3)",
                 fwd_bwd(lambda t: UAMTLossFn.apply(zt, t, thr, hard)[0], z),
                 fwd_bwd(lambda t: t_uamt(zt, t, thr, hard), z))


if __name__ == "__main__":
    main()
