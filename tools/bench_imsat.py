#!/usr/bin/env python3
"""Forward and backward time of the three IMSAT forms (csrc/cy_imsat.hip: IMSATFn, IMSATPairFn, SoftmaxIMSATFn) against
the unfused composition of the same formulas from torch ops on the same tensors -- the baseline, since before these
kernels the project had no IMSAT at all -- at the shapes a user runs: the `Up_conv2` (224^2) and `Up_conv3` (112^2) taps
of C2 with 2 x 16 unlabeled slices through a DenseClusterHead of K = 20 / 40 clusters, and the segmentation output of
16 slices at K = 4.

    python tools/bench_imsat.py [--rounds 5] [--iters 5]        (on the GPU box, one process)

The two versions alternate round by round in one process; a figure is the median over the rounds of the mean of
`iters` back-to-back calls between two device events, after two warm-up calls of each.  Per kernel form the table
gives the achieved bytes/s from the algorithmic bytes (4 R K forward, 8 R K backward; the pair twice that), the device
kernels of one forward + backward (counted once with torch.profiler, outside the timed loops), and the peak of device
memory above the inputs during one forward + backward (temporaries, saved tensors and the gradient itself).  The two
versions' results are compared once per shape before anything is timed."""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "contrast-you_amd"))
from cyhip.functions import IMSATFn, IMSATPairFn, softmax_imsat  # noqa: E402

EPS = 1e-8
# (form, name, slices, side, K)
SHAPES = (("rows", "Up_conv2", 32, 224, 20), ("rows", "Up_conv2", 32, 224, 40), ("rows", "Up_conv3", 32, 112, 20),
          ("rows", "Up_conv3", 32, 112, 40), ("pair", "Up_conv2", 16, 224, 20), ("pair", "Up_conv2", 16, 224, 40),
          ("pair", "Up_conv3", 16, 112, 20), ("pair", "Up_conv3", 16, 112, 40), ("logits", "output", 16, 224, 4))


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def torch_entropies(p):
    cond = -(p * torch.log(p + EPS)).sum(1).mean()
    m = p.mean(0)
    return -(m * torch.log(m + EPS)).sum(), cond


def versions(form, x, y):
    """-> {version: (forward() -> loss, leaves)}; the loss is 0.5 * sum of imsat_loss (+ the MSE for the pair)"""
    if form == "rows":
        def fused():
            marg, cond = IMSATFn.apply(x)
            return cond - marg

        def composed():
            marg, cond = torch_entropies(x)
            return cond - marg
        return {"fused": fused, "torch": composed}, (x,)
    if form == "pair":
        def fused():
            m1, c1, m2, c2, mse = IMSATPairFn.apply(x, y)
            return 0.5 * ((c1 - m1) + (c2 - m2)) + mse

        def composed():
            (m1, c1), (m2, c2) = torch_entropies(x), torch_entropies(y)
            return 0.5 * ((c1 - m1) + (c2 - m2)) + torch.nn.functional.mse_loss(x, y)
        return {"fused": fused, "torch": composed}, (x, y)

    def fused():
        marg, cond = softmax_imsat(x)
        return cond - marg

    def composed():
        p = x.softmax(1).permute(0, 2, 3, 1).reshape(-1, x.shape[1])
        marg, cond = torch_entropies(p)
        return cond - marg
    return {"fused": fused, "torch": composed}, (x,)


def kernels_of(fn):
    """device kernels launched by fn(), or None where the profiler is not available"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                   and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception:  # noqa: BLE001
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", type=int, default=None, help="index into SHAPES: that shape alone")
    ap.add_argument("--no-profiler", action="store_true", help="leave the kernel counts out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
    dev = "cuda"
    print(f"{'form':>6s} {'tap':>8s} {'rows':>8s} {'K':>3s} | {'fused fwd':>9s} {'torch fwd':>9s} | {'fused bwd':>9s} "
          f"{'torch bwd':>9s} (ms) | fused GB/s fwd, bwd | kernels fused, torch | peak MB fused, torch")
    for form, name, n, side, K in (SHAPES if a.only is None else SHAPES[a.only:a.only + 1]):
        R = n * side * side
        g = torch.Generator(device=dev).manual_seed(K + side)
        if form == "logits":
            x = (torch.randn(n, side, side, K, device=dev, generator=g) * 2).permute(0, 3, 1, 2).requires_grad_(True)
            y = None
        else:
            both = (torch.randn(2 * R if form == "pair" else R, K, device=dev, generator=g) * 2).softmax(1)
            x, y = (both[:R], both[R:]) if form == "pair" else (both, None)
            x = x.detach().requires_grad_(True)
            y = None if y is None else y.detach().requires_grad_(True)
        fns, leaves = versions(form, x, y)
        keep, res = {}, {}

        def fwd(v):
            keep[v] = fns[v]()

        def bwd(v):
            for t in leaves:
                t.grad = None
            keep[v].backward(retain_graph=True)

        for v in fns:  # warm-up, and the comparison
            for _ in range(2):
                fwd(v)
                bwd(v)
            res[v] = (float(keep[v]), [t.grad.clone() for t in leaves])
        rel = max(float((u - w).abs().max() / w.abs().max()) for u, w in zip(res["fused"][1], res["torch"][1]))
        note = f"   loss {res['fused'][0]:.7f} vs {res['torch'][0]:.7f}, gradients differ by {rel:.1e}"
        stats = {}
        for v in fns:
            keep.clear()
            for t in leaves:
                t.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fwd(v)
            bwd(v)
            torch.cuda.synchronize()
            peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            count = None if a.no_profiler else kernels_of(lambda: (fwd(v), bwd(v)))
            stats[v] = (peak, count)
        t = {(v, k): [] for v in fns for k in ("f", "b")}
        for _ in range(a.rounds):
            for v in fns:
                t[(v, "f")].append(events(lambda: fwd(v), a.iters))
                t[(v, "b")].append(events(lambda: bwd(v), a.iters))
        m = {k: statistics.median(v) for k, v in t.items()}
        spread = max((max(v) - min(v)) / statistics.median(v) for v in t.values())
        inputs = 2 if form == "pair" else 1
        gbs = [inputs * c * R * K / (m[("fused", k)] * 1e-3) / 1e9 for c, k in ((4, "f"), (8, "b"))]
        counts = ", ".join("not measured" if stats[v][1] is None else str(stats[v][1]) for v in fns)
        print(f"{form:>6s} {name:>8s} {R:8d} {K:3d} | {m[('fused', 'f')]:9.3f} {m[('torch', 'f')]:9.3f} | "
              f"{m[('fused', 'b')]:9.3f} {m[('torch', 'b')]:9.3f}      | {gbs[0]:8.0f}, {gbs[1]:8.0f} | {counts:>14s} "
              f"| {stats['fused'][0]:8.1f}, {stats['torch'][0]:8.1f}   spread {spread * 100:.0f} %{note}", flush=True)
        del keep, res, x, y, fns, leaves
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
