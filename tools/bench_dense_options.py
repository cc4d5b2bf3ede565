#!/usr/bin/env python3
"""Forward and backward time of the per-row projector (PixelMLPFn's kernels, csrc/cy_pixel_mlp.hip) against the unfused
composition from the existing entry points -- cy_linear_fwd x2 + cy_l2norm_fwd, and cy_l2norm_bwd + cy_linear_bwd x2,
with the [rows, 256] f32 hidden and output tensors in memory (what DenseProjectionHead._rows_max composes) -- on the
rows of the C2 decoder taps at 64 views: 64 x 14^2 x 256 ch, 64 x 56^2 x 64 ch, 64 x 224^2 x 32 ch; hid = out = 256,
normalised, bf16 and f32 rows.

    python tools/bench_dense_options.py [--rounds 3] [--iters 3]        (on the GPU box, one process)

The two forms alternate round by round in one process; a figure is the median over the rounds of the mean of `iters`
back-to-back calls between two device events (ms).  The unfused form reads f32 rows, so for bf16 rows its forward
includes the conversion of x and its backward the conversion of dx, as in _rows_max.  Both backward passes produce dx
and all four parameter gradients.  The two forms' outputs are compared once per shape before anything is timed."""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "contrast-you_amd"))
from cyhip import ops  # noqa: E402

SHAPES = ((64, 14, 256), (64, 56, 64), (64, 224, 32))  # (views, side, channels)
HID = OUT = 256
SLOPE = 0.01


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--only", type=int, default=None, help="index into SHAPES: that shape alone")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
    dev = "cuda"
    print(f"{'rows':>9s} {'C':>4s} {'dtype':>5s} | {'fused fwd':>10s} {'unfused fwd':>11s} | {'fused bwd':>10s} {'unfused bwd':>11s}  (ms)")
    for n, side, Cc in (SHAPES if a.only is None else SHAPES[a.only:a.only + 1]):
        M = n * side * side
        for dt in (torch.bfloat16, torch.float32):
            g = torch.Generator().manual_seed(1)
            x = torch.randn(M, Cc, device=dev).to(dt)
            w1, b1 = (torch.randn(HID, Cc, generator=g) / Cc ** 0.5).to(dev), (torch.randn(HID, generator=g) * 0.1).to(dev)
            w2, b2 = (torch.randn(OUT, HID, generator=g) / 16).to(dev), (torch.randn(OUT, generator=g) * 0.1).to(dev)
            dz = torch.randn(M, OUT, device=dev)
            keep = {}

            def fused_fwd():
                keep["y"], keep["inv"] = ops.pixel_mlp_fwd(x, None, w1, b1, w2, b2, SLOPE, True)

            def fused_bwd():
                keep["fg"] = ops.pixel_mlp_bwd(x, None, w1, b1, w2, keep["y"], keep["inv"], dz, SLOPE, True, True, True)

            def unfused_fwd():
                xf = x.float()
                h = ops.linear_fwd(xf, w1, b1, 1, SLOPE)
                y2 = ops.linear_fwd(h, w2, b2, 0, 0.0)
                z, norms = ops.l2norm_fwd(y2)
                keep["u"] = (xf, h, y2, z, norms)

            def unfused_bwd():
                xf, h, y2, z, norms = keep["u"]
                dy2 = ops.l2norm_bwd(y2, norms, dz)
                dh, dw2, db2 = ops.linear_bwd(h, w2, y2, dy2, 0, 0.0, True, True)
                dx, dw1, db1 = ops.linear_bwd(xf, w1, h, dh, 1, SLOPE, True, True)
                keep["ug"] = (dx.to(dt), dw1, db1, dw2, db2)

            for fn in (fused_fwd, fused_bwd, unfused_fwd, unfused_bwd):  # warm-up, and the comparison
                fn()
                fn()
            torch.cuda.synchronize()
            # largest difference between the two forms relative to the tensor's largest magnitude: y, then the worst
            # gradient (f32 rows: summation order; bf16 rows: the fused form's rounding points, tests/test_gpu_dense_options.py)
            rel = lambda u, v: float((u.float() - v.float()).abs().max() / v.float().abs().max())  # noqa: E731
            note = (f"   forms differ by {rel(keep['y'], keep['u'][3]):.1e} (y), "
                    f"{max(rel(u, v) for u, v in zip(keep['fg'], keep['ug'])):.1e} (gradients)")
            # a third opinion on ~570 rows spread over the problem (the last 64 among them): float64 torch on the device
            sel = torch.unique(torch.cat([torch.arange(0, M, max(1, M // 509)), torch.arange(max(0, M - 64), M)])).to(dev)
            hs = torch.nn.functional.leaky_relu(x[sel].double() @ w1.double().t() + b1.double(), SLOPE)
            ref = torch.nn.functional.normalize(hs @ w2.double().t() + b2.double(), dim=1)
            note += (f"; y of the sampled rows against float64: fused {rel(keep['y'][sel], ref):.1e}, "
                     f"unfused {rel(keep['u'][3][sel], ref):.1e}")
            t = {k: [] for k in ("ff", "uf", "fb", "ub")}
            for _ in range(a.rounds):
                t["ff"].append(events(fused_fwd, a.iters))
                t["uf"].append(events(unfused_fwd, a.iters))
                t["fb"].append(events(fused_bwd, a.iters))
                t["ub"].append(events(unfused_bwd, a.iters))
            m = {k: statistics.median(v) for k, v in t.items()}
            spread = max((max(v) - min(v)) / statistics.median(v) for v in t.values())
            print(f"{M:9d} {Cc:4d} {str(dt)[6:]:>5s} | {m['ff']:10.3f} {m['uf']:11.3f} | {m['fb']:10.3f} {m['ub']:11.3f}"
                  f"   spread {spread * 100:.0f} %{note}", flush=True)
            del keep, x, dz
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
