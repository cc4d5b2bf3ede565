#!/usr/bin/env python3
"""Forward and backward time of the four wide-K regularisers (csrc/cy_wide_reg.hip: SoftmaxEntropyFn, SoftmaxSelfMSEFn,
UAMTLossFn soft and hard, MixSoftmaxMSEFn at 16 < K <= 64) against the unfused composition of the same formulas from
torch ops on the same tensors -- the baseline, since before these kernels that was the only way the losses could run on
multi-prototype logits -- at the shape a user runs: the segmentation output of 16 slices of 224^2 with K = 20, 40, 64
outputs (5 classes x 4 prototypes, 4 x 10, 4 x 16).

    python tools/bench_wide_reg.py [--rounds 5] [--iters 20]        (on the GPU box, one process)

The two versions alternate round by round in one process; a figure is the median over the rounds of the mean of
`iters` back-to-back calls between two device events, after two warm-up calls of each.  Per family the table gives the
algorithmic bytes of the fused pass (4 bytes per logit read or gradient written: `reads` logit tensors forward,
`reads` + 1 backward; ICT reads the teacher twice), the achieved bytes/s and their share of the HBM peak, and the lanes
of a 16-lane row that hold a channel at that K.  The two versions' results are compared once per shape before anything
is timed.  The times are whole calls (autograd function, allocation, both launches of a forward), not kernel times."""
import argparse
import math
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "contrast-you_amd"))
from cyhip.functions import MixSoftmaxMSEFn, SoftmaxEntropyFn, SoftmaxSelfMSEFn, UAMTLossFn  # noqa: E402

EPS = 1e-16
HBM_PEAK = 8.0e12  # bytes/s, MI355X
N, SIDE = 16, 224
KS = (20, 40, 64)
# family -> logit tensors the fused forward reads (the backward reads the same and writes one gradient)
READS = {"entropy": 1, "selfmse": 1, "uamt_soft": 2, "uamt_hard": 2, "mixmse": 3}


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def entropy_of(p):
    return -(p * (p + EPS).log()).sum(1)


def versions(family, zs, zt, thr, index, w):
    """-> {version: forward() -> loss} on the student leaf zs"""
    K = zs.shape[1]
    if family == "entropy":
        return {"fused": lambda: SoftmaxEntropyFn.apply(zs, EPS), "torch": lambda: entropy_of(zs.softmax(1)).mean()}
    if family == "selfmse":
        def composed():
            p = zs.softmax(1)
            return F.mse_loss(p, F.one_hot(p.max(1)[1], K).movedim(-1, 1).float())
        return {"fused": lambda: SoftmaxSelfMSEFn.apply(zs), "torch": composed}
    if family == "mixmse":
        def composed():
            p = zt.softmax(1)
            mixed = w[0] * p + w[1] * p[index.long()]
            return F.mse_loss(zs.softmax(1), mixed, reduction="none").mean()
        return {"fused": lambda: MixSoftmaxMSEFn.apply(zs, zt, index, *w), "torch": composed}
    hard = family == "uamt_hard"

    def composed():
        t = zt.softmax(1)
        mask = (entropy_of(t) < thr).float()
        tau = F.one_hot(t.argmax(1), K).movedim(-1, 1).float() if hard else t
        e = F.mse_loss(tau, zs.softmax(1), reduction="none").mean(1)
        return (e * mask).mean() / (mask.mean() + 1e-2)
    return {"fused": lambda: UAMTLossFn.apply(zt, zs, thr, hard)[0], "torch": composed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default=None, help="one family of " + ", ".join(READS))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
    dev = "cuda"
    npix = N * SIDE * SIDE
    print(f"{npix} pixels ({N} x {SIDE}^2); times in ms, median of {a.rounds} rounds of {a.iters} calls")
    print(f"{'family':>10s} {'K':>3s} {'lanes':>6s} | {'fused fwd':>9s} {'torch fwd':>9s} {'x':>5s} | {'fused bwd':>9s} "
          f"{'torch bwd':>9s} {'x':>5s} | MB moved fwd, bwd | fused GB/s (share of HBM peak) fwd, bwd")
    for family in ([a.only] if a.only else READS):
        for K in KS:
            g = torch.Generator(device=dev).manual_seed(K)
            scale = torch.rand(N, SIDE, SIDE, 1, device=dev, generator=g) * 3
            zs = (torch.randn(N, SIDE, SIDE, K, device=dev, generator=g) * scale).permute(0, 3, 1, 2)
            zt = (torch.randn(N, SIDE, SIDE, K, device=dev, generator=g) * scale).permute(0, 3, 1, 2)
            zs.requires_grad_(True)
            index = torch.randperm(N, device=dev, generator=g).to(torch.int32)
            fns = versions(family, zs, zt, 0.85 * math.log(K), index, (0.3, 0.7))
            keep, res = {}, {}

            def fwd(v):
                keep[v] = fns[v]()

            def bwd(v):
                zs.grad = None
                keep[v].backward(retain_graph=True)

            for v in fns:  # warm-up, and the comparison
                for _ in range(2):
                    fwd(v)
                    bwd(v)
                res[v] = (float(keep[v].detach()), zs.grad.clone())
            rel = float((res["fused"][1] - res["torch"][1]).abs().max() / res["torch"][1].abs().max())
            note = f"   loss {res['fused'][0]:.7f} vs {res['torch'][0]:.7f}, gradients differ by {rel:.1e}"
            t = {(v, k): [] for v in fns for k in ("f", "b")}
            for _ in range(a.rounds):
                for v in fns:
                    t[(v, "f")].append(events(lambda: fwd(v), a.iters))
                    t[(v, "b")].append(events(lambda: bwd(v), a.iters))
            m = {k: statistics.median(v) for k, v in t.items()}
            spread = max((max(v) - min(v)) / statistics.median(v) for v in t.values())
            moved = [4.0 * npix * K * READS[family], 4.0 * npix * K * (READS[family] + 1)]
            rate = [moved[0] / (m[("fused", "f")] * 1e-3), moved[1] / (m[("fused", "b")] * 1e-3)]
            lanes = f"{-(-K // 4)}/16"
            print(f"{family:>10s} {K:3d} {lanes:>6s} | {m[('fused', 'f')]:9.3f} {m[('torch', 'f')]:9.3f} "
                  f"{m[('torch', 'f')] / m[('fused', 'f')]:5.1f} | {m[('fused', 'b')]:9.3f} {m[('torch', 'b')]:9.3f} "
                  f"{m[('torch', 'b')] / m[('fused', 'b')]:5.1f} | {moved[0] / 1e6:7.1f}, {moved[1] / 1e6:7.1f} | "
                  f"{rate[0] / 1e9:6.0f} ({100 * rate[0] / HBM_PEAK:4.1f} %), {rate[1] / 1e9:6.0f} "
                  f"({100 * rate[1] / HBM_PEAK:4.1f} %)   spread {spread * 100:.0f} %{note}", flush=True)
            del keep, res, zs, zt, fns
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
