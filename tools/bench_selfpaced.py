#!/usr/bin/env python3
"""Time of SelfPacedSupConLoss forward + backward on the fused kernels (csrc/cy_contrast.hip: SelfPacedSupConFn, deferred
checks, as the training hook runs it) against the composition the criterion keeps for the widths the kernels refuse
(`SelfPacedSupConLoss._composition`: the similarity GEMM on the f32 MFMA kernel, then torch elementwise ops on 2n x 2n
tensors with autograd history and the reference's three host reads) -- what every call ran before these kernels -- on
the same tensors, at R = 2n = 36 and 64 rows (the reference's pre-training batches) and R = 4096 (C5), D = 256.

    python tools/bench_selfpaced.py [--rounds 7] [--window-ms 200] [--mode soft]        (on the GPU box, one process)

The two versions alternate round by round in one process; a figure is the median over the rounds of the mean of a window
of back-to-back forward + backward calls between two device events -- as many calls as fill `window-ms` at the pace of
ten trial calls, at least ten -- after two warm-up calls of each: the time of a call as Python issues it, host reads
included, not a kernel time.  `spread` is the lowest and the highest round.  The table
also gives the peak of device memory above the inputs during one forward + backward.  The two versions' results are
compared once per shape before anything is timed."""
import argparse
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "contrast-you_amd"))
from contrastyou.losses import SelfPacedSupConLoss  # noqa: E402

SHAPES = ((18, 256), (32, 256), (2048, 256))   # n, D
GAMMA = 8.0


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(n, D, a, dev):
    gen = torch.Generator(device=dev).manual_seed(n + D)
    z = F.normalize(torch.randn(2 * n, D, device=dev, generator=gen), dim=1).requires_grad_(True)
    z1, z2 = torch.chunk(z, 2)   # the two halves of one tensor, as the hook hands the projector's output over
    target = [i % 6 for i in range(n)]
    crit = SelfPacedSupConLoss(weight_update=a.mode, correct_grad=False)
    crit.set_gamma(GAMMA)
    crit.defer_checks = True
    up = torch.full((), 0.7, device=dev)

    def step(v):
        z.grad = None
        loss = crit(z1, z2, target=target) if v == "fused" else crit._composition(z1, z2, target)
        loss.backward(up)
        return loss

    res = {}
    for v in ("fused", "torch"):
        for _ in range(2):
            loss = step(v)
        assert (crit._last is not None) == (v == "fused"), "which path ran"
        res[v] = (loss.item(), float(crit.downgrade_ratio), z.grad.clone())
        crit.validate()
    rel = float((res["fused"][2] - res["torch"][2]).abs().max() / res["torch"][2].abs().max())
    note = (f"   loss {res['fused'][0]:.7f} vs {res['torch'][0]:.7f}, ratio {res['fused'][1]:.6f} vs {res['torch'][1]:.6f}, "
            f"gradients differ by {rel:.1e}")
    peak = {}
    for v in ("fused", "torch"):
        z.grad = None
        crit._last = crit._mats = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(v)
        torch.cuda.synchronize()
        peak[v] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        crit.validate()
    t = {"fused": [], "torch": []}
    iters = {v: max(10, int(a.window_ms / events(lambda: step(v), 10)) + 1) for v in t}
    crit.validate()
    for _ in range(a.rounds):
        for v in t:
            t[v].append(events(lambda: step(v), iters[v]))
            crit.validate()
    m = {v: statistics.median(x) for v, x in t.items()}
    print(f"{2 * n:5d} {D:4d} | {m['fused']:9.3f} ({min(t['fused']):.3f} .. {max(t['fused']):.3f}) | {m['torch']:9.3f} "
          f"({min(t['torch']):.3f} .. {max(t['torch']):.3f}) | {m['torch'] / m['fused']:6.2f}x | {peak['fused']:8.2f}, "
          f"{peak['torch']:8.2f} | {iters['fused']}, {iters['torch']}{note}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--mode", choices=("hard", "soft"), default="soft")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
    print(f"{'R':>5s} {'D':>4s} | fused f+b ms (spread) | composition f+b ms (spread) | ratio | peak MiB fused, composition | calls per window")
    for n, D in SHAPES:
        measure(n, D, a, "cuda")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
