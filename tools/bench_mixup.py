#!/usr/bin/env python3
"""Time of the three MixUp / ICT kernel groups (csrc/cy_mixup.hip: ops.mix_images, MixupKLFn, MixSoftmaxMSEFn) against
the unfused composition of the same formulas from torch ops on the same tensors -- the baseline, since before these
kernels the project had neither method -- at the workloads' own shapes: the 2 x 16 slices a MixUp / ICT step mixes, at
224^2 with K = 4 (C2) and at 256^2 with K = 8 (C4).

    python tools/bench_mixup.py [--rounds 5] [--iters 5]        (on the GPU box, one process)

The two versions alternate round by round in one process; a figure is the median over the rounds of the mean of
`iters` back-to-back calls between two device events, after two warm-up calls of each.  Per group the table gives the
algorithmic bytes of the fused form (images: read x twice, write once; MixUp loss: logits + two labels forward, the
same + the gradient backward; ICT loss: student once and teacher twice forward, the same + the gradient backward), the
bytes/s they amount to, and the peak of device memory above the inputs during one forward + backward.  The two
versions' results are compared once per shape before anything is timed."""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "contrast-you_amd"))
from cyhip import ops  # noqa: E402
from cyhip.functions import MixSoftmaxMSEFn, MixupKLFn  # noqa: E402

EPS = 1e-16
SHAPES = (("C2", 32, 224, 4), ("C4", 32, 256, 8))  # workload, slices, side, K
LAM = 0.3628452076929192


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def groups(n, side, K, dev, gen):
    """-> {group: ({version: forward}, leaf or None, (forward bytes, backward bytes))}"""
    index = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    idx = index.to(dev)
    w_self, w_other = ops.mix_weights(LAM)
    image = torch.rand(n, 1, side, side, device=dev, generator=gen)
    z = (torch.randn(n, side, side, K, device=dev, generator=gen) * 2).permute(0, 3, 1, 2).requires_grad_(True)
    t = (torch.randn(n, side, side, K, device=dev, generator=gen) * 2).permute(0, 3, 1, 2)
    y = torch.randint(0, K, (n, side, side), device=dev, generator=gen)
    dev_index = ops.mix_index(index, n, dev)
    npix = n * side * side

    def kl_torch():
        oh = torch.nn.functional.one_hot(y, K).movedim(-1, 1).float()
        target = LAM * oh + (1 - LAM) * oh[idx, :]
        return (-target * torch.log((z.softmax(1) + EPS) / (target + EPS))).sum(1).mean()

    def mse_torch():
        p = t.softmax(1)
        target = LAM * p + (1 - LAM) * p[idx, :]
        return torch.nn.functional.mse_loss(z.softmax(1), target, reduction="none").mean()

    return {
        "images": ({"fused": lambda: ops.mix_images(image, dev_index, w_self, w_other),
                    "torch": lambda: LAM * image + (1 - LAM) * image[idx, :]}, None, (12 * npix, 0)),
        "mixkl": ({"fused": lambda: MixupKLFn.apply(z, y, dev_index, w_self, w_other, EPS), "torch": kl_torch}, z,
                  (npix * (4 * K + 16), npix * (8 * K + 16))),
        "mixmse": ({"fused": lambda: MixSoftmaxMSEFn.apply(z, t, dev_index, w_self, w_other), "torch": mse_torch}, z,
                   (npix * 12 * K, npix * 16 * K)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
    dev = "cuda"
    print(f"{'load':>4s} {'group':>7s} {'npix':>8s} {'K':>2s} | {'fused fwd':>9s} {'torch fwd':>9s} | {'fused bwd':>9s} "
          f"{'torch bwd':>9s} (ms) | fused MB fwd, bwd | fused GB/s fwd, bwd | peak MB fused, torch")
    for load, n, side, K in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(K + side)
        for group, (fns, leaf, nbytes) in groups(n, side, K, dev, gen).items():
            keep, res = {}, {}

            def fwd(v):
                keep[v] = fns[v]()

            def bwd(v):
                if leaf is not None:
                    leaf.grad = None
                    keep[v].backward(retain_graph=True)

            for v in fns:  # warm-up, and the comparison
                for _ in range(2):
                    fwd(v)
                    bwd(v)
                res[v] = (keep[v].detach().clone(), None if leaf is None else leaf.grad.clone())
            if leaf is None:
                note = "   bit-equal" if torch.equal(res["fused"][0], res["torch"][0]) else "   NOT bit-equal"
            else:
                rel = float((res["fused"][1] - res["torch"][1]).abs().max() / res["torch"][1].abs().max())
                note = (f"   loss {float(res['fused'][0]):.7f} vs {float(res['torch'][0]):.7f}, "
                        f"gradients differ by {rel:.1e}")
            peak = {}
            for v in fns:
                keep.clear()
                if leaf is not None:
                    leaf.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                fwd(v)
                bwd(v)
                torch.cuda.synchronize()
                peak[v] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            t = {(v, k): [] for v in fns for k in ("f", "b")}
            for _ in range(a.rounds):
                for v in fns:
                    t[(v, "f")].append(events(lambda: fwd(v), a.iters))
                    t[(v, "b")].append(events(lambda: bwd(v), a.iters) if leaf is not None else 0.0)
            m = {k: statistics.median(v) for k, v in t.items()}
            gbs = [b / (m[("fused", k)] * 1e-3) / 1e9 if b else 0.0 for b, k in zip(nbytes, ("f", "b"))]
            print(f"{load:>4s} {group:>7s} {n * side * side:8d} {K:2d} | {m[('fused', 'f')]:9.3f} "
                  f"{m[('torch', 'f')]:9.3f} | {m[('fused', 'b')]:9.3f} {m[('torch', 'b')]:9.3f}      | "
                  f"{nbytes[0] / 2 ** 20:7.1f}, {nbytes[1] / 2 ** 20:7.1f} | {gbs[0]:8.0f}, {gbs[1]:8.0f} | "
                  f"{peak['fused']:8.1f}, {peak['torch']:8.1f}{note}", flush=True)
            del keep, res
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
