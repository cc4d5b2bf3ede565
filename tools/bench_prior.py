#!/usr/bin/env python3
"""Time of the DAE-prior loss (csrc/cy_prior.hip: DAELossFn) forward + backward against the unfused composition of the
same formula from torch ops on the same tensors -- F.mse_loss(sigmoid(F.conv2d(logits, w, b)), image), the baseline,
since before these kernels the project had neither method -- at the workloads' own shapes: N = 16 and 32 slices at 224^2
with K = 4 (C2) and at 256^2 with K = 16; and of the orthogonality loss (OrthoLossFn) against its composition
(normalise, matmul, eye, subtract, square, mean) at K = 16 and K = 64 prototypes of C = 16.

    python tools/bench_prior.py [--rounds 7] [--iters 50]        (on the GPU box, one process)

The two versions alternate round by round in one process; a figure is the median over the rounds of the mean of
`iters` back-to-back calls between two device events, after two warm-up calls of each: the time of a call as Python
issues it, not a kernel time.  The table gives the algorithmic bytes of the fused form (forward: logits + image;
backward: logits twice + image + the gradient), those bytes over the call time, and the peak of device memory above
the inputs during one forward + backward.  The two versions' results are compared once per shape before anything is
timed."""
import argparse
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "contrast-you_amd"))
from cyhip.functions import DAELossFn, OrthoLossFn  # noqa: E402

DAE_SHAPES = ((16, 224, 4), (32, 224, 4), (16, 256, 16), (32, 256, 16))  # slices, side, K
ORTHO_SHAPES = ((16, 16), (64, 16))                                       # K, C


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def dae_group(n, side, K, dev, gen):
    z = (torch.randn(n, side, side, K, device=dev, generator=gen) * 2).permute(0, 3, 1, 2).requires_grad_(True)
    w = (torch.randn(1, K, 1, 1, device=dev, generator=gen) * 0.5).requires_grad_(True)
    b = torch.zeros(1, device=dev).requires_grad_(True)
    image = torch.rand(n, 1, side, side, device=dev, generator=gen)
    npix = n * side * side
    fns = {"fused": lambda: DAELossFn.apply(z, w, b, image, "sigmoid"),
           "torch": lambda: F.mse_loss(torch.sigmoid(F.conv2d(z, w, b)), image)}
    return fns, (z, w, b), (npix * (4 * K + 4), npix * (12 * K + 4))


def ortho_group(K, Cc, dev, gen):
    v = torch.randn(K, Cc, 1, 1, device=dev, generator=gen).requires_grad_(True)

    def composed():
        n = F.normalize(v, p=2, dim=1).squeeze()
        m = n @ n.t()
        return (m - torch.eye(K, device=dev, dtype=m.dtype)).pow(2).mean()

    return {"fused": lambda: OrthoLossFn.apply(v), "torch": composed}, (v,), (4 * K * Cc, 8 * K * Cc)


def measure(label, fns, leaves, nbytes, a):
    keep, res = {}, {}

    def fwd(v):
        keep[v] = fns[v]()

    def bwd(v):
        for leaf in leaves:
            leaf.grad = None
        keep[v].backward(retain_graph=True)

    for v in fns:  # warm-up, and the comparison
        for _ in range(2):
            fwd(v)
            bwd(v)
        res[v] = (keep[v].detach().clone(), [leaf.grad.clone() for leaf in leaves])
    rel = max(float((f - t).abs().max() / t.abs().max()) for f, t in zip(res["fused"][1], res["torch"][1]))
    note = f"   loss {float(res['fused'][0]):.7f} vs {float(res['torch'][0]):.7f}, gradients differ by {rel:.1e}"
    peak = {}
    for v in fns:
        keep.clear()
        for leaf in leaves:
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
            t[(v, "b")].append(events(lambda: bwd(v), a.iters))
    m = {k: statistics.median(v) for k, v in t.items()}
    gbs = [b / (m[("fused", k)] * 1e-3) / 1e9 for b, k in zip(nbytes, ("f", "b"))]
    print(f"{label} | {m[('fused', 'f')]:9.3f} {m[('torch', 'f')]:9.3f} | {m[('fused', 'b')]:9.3f} "
          f"{m[('torch', 'b')]:9.3f} | {m[('fused', 'f')] + m[('fused', 'b')]:9.3f} "
          f"{m[('torch', 'f')] + m[('torch', 'b')]:9.3f} (ms) | {nbytes[0] / 2 ** 20:7.2f}, {nbytes[1] / 2 ** 20:7.2f} | "
          f"{gbs[0]:6.0f}, {gbs[1]:6.0f} | {peak['fused']:8.2f}, {peak['torch']:8.2f}{note}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
    dev = "cuda"
    print(f"{'group':>5s} {'shape':>14s} | {'fused fwd':>9s} {'torch fwd':>9s} | {'fused bwd':>9s} {'torch bwd':>9s} | "
          f"{'fused f+b':>9s} {'torch f+b':>9s}      | fused MB fwd, bwd | MB over call time, GB/s | peak MB fused, torch")
    for n, side, K in DAE_SHAPES:
        gen = torch.Generator(device=dev).manual_seed(K + side + n)
        fns, leaves, nbytes = dae_group(n, side, K, dev, gen)
        measure(f"{'dae':>5s} {f'{n}x{K}x{side}x{side}':>14s}", fns, leaves, nbytes, a)
        del fns, leaves
        torch.cuda.empty_cache()
    for K, Cc in ORTHO_SHAPES:
        gen = torch.Generator(device=dev).manual_seed(K + Cc)
        fns, leaves, nbytes = ortho_group(K, Cc, dev, gen)
        measure(f"{'ortho':>5s} {f'{K}x{Cc}':>14s}", fns, leaves, nbytes, a)


if __name__ == "__main__":
    main()
