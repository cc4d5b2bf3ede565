#!/usr/bin/env python3
"""Forward and forward+backward time of the patch-wise IIC loss (IIDSegmentationSmallPathLoss: the batched patch kernels
of csrc/cy_mi.hip) against the loop a user would write without it: IIDSegmentationLoss called on every contiguous patch
slice and averaged -- at the workload's own shape, 16 x 20 x 224^2 f32, patch 32 (169 patches), padding 7 (225
displacements) and padding 1.

    python tools/bench_patch_iic.py [--rounds 3] [--iters 2] [--pads 7 1]        (on the GPU box, one process)

The two versions alternate round by round in one process; a figure is the median over the rounds of the mean of
back-to-back calls between two device events (`iters` of them, or as many as fill 200 ms), after warm-up calls of each.
The three kernels of the batched path are then timed one by one the same way and set against their algorithmic HBM
bytes: the joints read the two maps once and write J; the loss reads J and writes the final joints and dJ; the adjoint
reads the two maps and dJ and writes the two gradients.  The two versions' results are compared once per padding before anything is timed."""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "contrast-you_amd"))
from contrastyou.losses.discreteMI import (IIDSegmentationLoss, IIDSegmentationSmallPathLoss,  # noqa: E402
                                           patch_generator)
from cyhip import ops  # noqa: E402

N, K, SIDE, PATCH = 16, 20, 224, 32
EPS = sys.float_info.epsilon


def events(fn, iters, window_ms=200.0):
    """mean time of a call over one window between two device events: `iters` calls, or as many as fill window_ms
    (a pilot call decides), whichever is more -- a window of a few milliseconds measures the clock"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    iters = max(iters, min(1000, int(window_ms / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--pads", type=int, nargs="+", default=[7, 1])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(224)
    x = (torch.randn(N, K, SIDE, SIDE, device=dev, generator=g) * 2).softmax(1).requires_grad_(True)
    y = (torch.randn(N, K, SIDE, SIDE, device=dev, generator=g) * 2).softmax(1).requires_grad_(True)
    size, step = (PATCH, PATCH), (PATCH // 2, PATCH // 2)
    for pad in a.pads:
        batched = IIDSegmentationSmallPathLoss(padding=pad, patch_size=PATCH)
        single = IIDSegmentationLoss(padding=pad, eps=EPS)

        def loop():
            losses = [single(p.contiguous(), q.contiguous())
                      for p, q in zip(patch_generator(x, size, step), patch_generator(y, size, step))]
            return sum(losses) / len(losses)

        fns = {"batched": lambda: batched(x, y), "loop": loop}
        keep, res = {}, {}

        def fwd(v):
            keep[v] = fns[v]()

        def both(v):
            x.grad = y.grad = None
            fns[v]().backward()

        for v in fns:  # warm-up, and the comparison
            both(v)
            fwd(v)
            res[v] = (float(keep[v]), x.grad.clone(), y.grad.clone())
        rel = max(float((u - w).abs().max() / w.abs().max()) for u, w in zip(res["batched"][1:], res["loop"][1:]))
        print(f"padding {pad}: loss {res['batched'][0]:.7f} (batched) vs {res['loop'][0]:.7f} (loop), gradients differ "
              f"by {rel:.1e} of their largest element", flush=True)
        t = {(v, k): [] for v in fns for k in ("fwd", "fwd+bwd")}
        for _ in range(a.rounds):
            for v in fns:
                t[(v, "fwd")].append(events(lambda: fwd(v), a.iters))
                t[(v, "fwd+bwd")].append(events(lambda: both(v), a.iters))
        m = {k: statistics.median(v) for k, v in t.items()}
        spread = max((max(v) - min(v)) / statistics.median(v) for v in t.values())
        for k in ("fwd", "fwd+bwd"):
            print(f"  {k:8s} batched {m[('batched', k)]:9.2f} ms   loop {m[('loop', k)]:9.2f} ms   "
                  f"loop / batched {m[('loop', k)] / m[('batched', k)]:6.2f}", flush=True)
        print(f"  spread over the rounds {spread * 100:.0f} %", flush=True)
        # the kernels of the batched path, one by one
        x1, x2 = (t_.detach().permute(0, 2, 3, 1).contiguous() for t_ in (x, y))
        plan = ops.joint_patch_plan(N, SIDE, SIDE, K, pad, PATCH)
        T = 2 * pad + 1
        jb, mb = 4 * plan["P"] * T * T * K * K, 4 * x1.numel()
        J = ops.joint_patch_fwd(x1, x2, pad, PATCH, pad == 0)
        _, _, _, dJ = ops.iid_patch_loss(J, 0 if pad == 0 else 1, 1.0, EPS)
        one = torch.ones(1, device=dev)
        parts = (("joint_patch_fwd", lambda: ops.joint_patch_fwd(x1, x2, pad, PATCH, pad == 0), 2 * mb + jb),
                 ("iid_patch_loss", lambda: ops.iid_patch_loss(J, 0 if pad == 0 else 1, 1.0, EPS), 3 * jb),
                 ("joint_patch_bwd", lambda: ops.joint_patch_bwd(x1, x2, dJ, one, pad, PATCH, pad == 0), 4 * mb + jb))
        print(f"  plan: {plan}", flush=True)
        for name, fn, nbytes in parts:
            fn()
            ms = statistics.median(events(fn, a.iters) for _ in range(a.rounds))
            print(f"  {name:16s} {ms:9.3f} ms   {nbytes / 2 ** 20:8.1f} MiB algorithmic   {nbytes / ms / 1e6:8.1f} GB/s",
                  flush=True)
        del J, dJ, x1, x2, keep, res
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
