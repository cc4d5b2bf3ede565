#!/usr/bin/env python3
"""Timings of the supervised criteria (csrc/cy_seg_loss.hip): `KL_div(weight=...)` and `DiceLoss` through
`from_logits` (fused kernels) next to their probability-space `forward` on torch-ROCm ops (softmax, one-hot and the
autograd temporaries at [N, K, H, W]), forward plus backward, at 16 x 4 x 224 x 224 and 16 x 8 x 256 x 256.

Method: HIP events around one call, three warm-up calls, the median of 20 timed calls, the two paths alternating in the
same process.  Then each kernel entry alone: 20 back-to-back launches per timed run (a single launch is near the events'
resolution), median of 20 runs, with the algorithmic bytes over that time: logits and labels read once per pass, the
gradient written once.  One line per figure.
"""
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "contrast-you_amd")]
from contrastyou.losses.dice_loss import DiceLoss  # noqa: E402
from contrastyou.losses.kl import KL_div  # noqa: E402
from cyhip import ops  # noqa: E402

DEV = "cuda"
EPS = 1e-16
RUNS, WARMUP, BURST = 20, 3, 20


def median_us(fn, burst=1):
    """median over RUNS of the device time of `burst` calls of fn, per call"""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(burst):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / burst)
    return statistics.median(times), min(times), max(times)


def fwd_bwd(fn, z):
    def run():
        z.grad = None
        fn(z).backward()
    return run


def main():
    print(f"# device {torch.cuda.get_device_name(0)}; f32 logits NHWC, int64 labels; median of {RUNS} (min..max), us")
    gen = torch.Generator().manual_seed(0)
    for n, K, hw in ((16, 4, 224), (16, 8, 256)):
        tag = f"{n}x{K}x{hw}x{hw}"
        npix = n * hw * hw
        read, write = npix * (K * 4 + 8), npix * K * 4
        z = ops.to_nhwc((torch.randn(n, K, hw, hw, generator=gen) * 2).to(DEV)).requires_grad_(True)
        y = torch.randint(0, K, (n, hw, hw), generator=gen).to(DEV)
        onehot = F.one_hot(y, K).movedim(-1, 1).float()
        print(f"# {tag}: {read / 1e6:.1f} MB read per pass, {write / 1e6:.1f} MB of gradient")
        for name, crit in (("KL_div(weight)", KL_div(weight=[1.0] + [2.0] * (K - 1))),
                           ("DiceLoss(ignore_index=0)", DiceLoss(ignore_index=0))):
            fused = fwd_bwd(lambda t: crit.from_logits(t, y), z)
            torch_ops = fwd_bwd(lambda t: crit(t.softmax(1), onehot), z)  # (the one-hot is not even rebuilt per call)
            f1, t1 = median_us(fused), median_us(torch_ops)
            f2, t2 = median_us(fused), median_us(torch_ops)
            for which, (a, b) in (("fused", (f1, f2)), ("torch ops", (t1, t2))):
                print(f"{tag} {name:26s} fwd+bwd {which:9s} {a[0]:8.1f} ({a[1]:.1f}..{a[2]:.1f})  "
                      f"again {b[0]:8.1f} ({b[1]:.1f}..{b[2]:.1f})")
        zd = z.detach()
        w = torch.tensor([1.0] + [2.0] * (K - 1), device=DEV)
        w = w / w.sum() * K
        one = torch.ones(1, device=DEV)
        _, table = ops.softmax_dice_fwd(zd, y, 2, 1.0, 0, "mean")
        kernels = (("softmax_wkl_fwd (2 launches)", lambda: ops.softmax_wkl_fwd(zd, y, w, EPS, "mean"), read),
                   ("softmax_wkl_bwd", lambda: ops.softmax_wkl_bwd(zd, y, w, one, EPS, "mean"), read + write),
                   ("softmax_dice_fwd (2 launches)", lambda: ops.softmax_dice_fwd(zd, y, 2, 1.0, 0, "mean"), read),
                   ("softmax_dice_bwd", lambda: ops.softmax_dice_bwd(zd, y, table, one, 2, 0, "mean"), read + write))
        for name, fn, nbytes in kernels:
            med, lo, hi = median_us(fn, BURST)
            print(f"{tag} {name:32s} {med:8.1f} ({lo:.1f}..{hi:.1f})  {nbytes / med / 1e6:6.2f} TB/s of "
                  f"{nbytes / 1e6:.1f} MB")


if __name__ == "__main__":
    main()
