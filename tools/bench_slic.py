#!/usr/bin/env python3
"""Time of the on-device SLIC superpixels (csrc/cy_slic.hip) at the reference's parameters (n_segments 40, sigma 5,
compactness 0.1, 10 rounds) on 16 and on 512 slices of 224^2: each stage alone (blur + quantisation, the clustering
rounds, the connected components) and `ops.slic`, the three through one workspace.

    python tools/bench_slic.py [--rounds 7] [--iters 20] [--slices 16 512]        (on the GPU box, one process)

A figure is the median over the rounds of the mean of `iters` back-to-back calls between two device events, after two
warm-up calls: the time of a call as Python issues it (its launches included), not a kernel time.  The stages are fed
each other's real outputs.  The images are soft blobs plus noise in 0..1, the same kind for every slice; the time of
the components depends on the label map (its union-find walks longer on longer components), so the table also gives
the mean number of superpixels per slice.  Compare the total with the step it would join: `bench.py --workload c2` and
`--workload c5` on the same box (DESIGN.md "On-device superpixels" keeps the figures)."""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "contrast-you_amd"))
from cyhip import ops  # noqa: E402

PARAMS = dict(n_segments=40, sigma=5.0, compactness=0.1)  # script/create_superpixel.py:27


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def images(n, side, dev, gen):
    """soft discs on a ramp plus noise, in 0..1"""
    yy, xx = torch.meshgrid(torch.arange(side, device=dev), torch.arange(side, device=dev), indexing="ij")
    out = 0.2 + 0.2 * xx / side + 0.1 * yy / side + torch.zeros(n, 1, 1, device=dev)
    for _ in range(6):
        cy, cx = (torch.rand(n, 1, 1, device=dev, generator=gen) * side for _ in range(2))
        rad = (0.08 + 0.22 * torch.rand(n, 1, 1, device=dev, generator=gen)) * side
        amp = torch.rand(n, 1, 1, device=dev, generator=gen) * 0.8 - 0.3
        out = out + amp * torch.sigmoid((rad - torch.hypot(yy - cy, xx - cx)) / 1.5)
    return (out + 0.03 * torch.randn(n, side, side, device=dev, generator=gen)).clamp_(0, 1).unsqueeze(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--slices", type=int, nargs="+", default=[16, 512])
    ap.add_argument("--side", type=int, default=224)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
    dev = "cuda"
    plan = ops.slic_plan(1, a.side, a.side, **PARAMS)
    print(f"{a.side}x{a.side}, {PARAMS}: S {plan['S']}, K {plan['K']}, r {plan['r']}, {plan['launches']} launches")
    print(f"{'slices':>6s} | {'blur+q':>8s} {'cluster':>8s} {'connect':>8s} | {'sum':>8s} {'ops.slic':>8s} (ms) | "
          f"{'us/slice':>8s} | superpixels per slice")
    for n in a.slices:
        x = images(n, a.side, dev, torch.Generator(device=dev).manual_seed(n))
        q = ops.slic_blur_q(x, PARAMS["sigma"])
        labels, _ = ops.slic_cluster(q, PARAMS["n_segments"], PARAMS["compactness"])
        fns = {"blur": lambda: ops.slic_blur_q(x, PARAMS["sigma"]),
               "cluster": lambda: ops.slic_cluster(q, PARAMS["n_segments"], PARAMS["compactness"]),
               "connect": lambda: ops.slic_connect(labels, PARAMS["n_segments"]),
               "all": lambda: ops.slic(x, **PARAMS)}
        for fn in fns.values():
            fn(), fn()
        count = ops.slic(x, **PARAMS)[1].float().mean().item()
        t = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                t[k].append(events(fn, a.iters))
        m = {k: statistics.median(v) for k, v in t.items()}
        print(f"{n:6d} | {m['blur']:8.3f} {m['cluster']:8.3f} {m['connect']:8.3f} | "
              f"{m['blur'] + m['cluster'] + m['connect']:8.3f} {m['all']:8.3f}      | {1e3 * m['all'] / n:8.2f} | "
              f"{count:.1f}", flush=True)


if __name__ == "__main__":
    main()
