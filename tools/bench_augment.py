#!/usr/bin/env python3
"""Time of the on-device loader augmentation (csrc/cy_augment.hip): the ACDC `pretrain` pipeline of augment_zoo on a
resident store of 256 x 256 slices, at the batches the C2 and the C4 benchmark steps consume.

    python tools/bench_augment.py [--rounds 7] [--iters 200] [--pillow-views 64]        (on the GPU box, one process)

C2: one step takes 16 labeled and 16 unlabeled slices, each transformed twice: 64 image views and 64 label views of
224 x 224 (two loaders, 32 views each: timed both as two calls of 32 and as one of 64).  C4: the same count at 256 x 256
(the pipeline's crop set to 256, so the crop window is the canvas).

Per size: `draw` is the host time of drawing the records of a batch (NumPy, no GPU work); `batch` is what a
`DeviceLoader` batch costs end to end, draws and uploads included -- the median over the rounds of the mean of `iters`
back-to-back batches between two device events, after warm-up batches, with the host clock around the same window
beside it (the larger of the two is what a step would wait for if nothing overlapped); `kernels` is
`ops.augment_views` alone on records drawn beforehand, between device events: the wrapper's issue time and its two
uploads are in it, so it bounds the two kernels from above.  Their own time is a kernel trace's, taken in a run of
its own (`rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_augment.py --rounds 1 --iters 50`).  views/s counts image views; every image view comes with its
label view.

Where Pillow can be imported, the same pipeline in Pillow on one core (rotate, two flips, crop, three ImageEnhance
steps, ToTensor's division, and the nearest twin for the label; decoding, seeding and collation excluded), and that
rate times 16, the CPUs a job has.  Compare with the step the batch feeds: `bench.py --workload c2` / `c4` on the same
box (DESIGN.md section 3 keeps the figures)."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "contrast-you_amd"))
from contrastyou.augment import DevicePipeline  # noqa: E402
from cyhip import ops  # noqa: E402
from semi_seg.augment import augment_zoo  # noqa: E402
from semi_seg.data import DeviceLoader, DeviceSliceStore  # noqa: E402

SLICES, SIDE = 512, 256


def slices(n, side, seed):
    """soft discs on a dark background, 8-bit, with a 4-class label: the statistics of a cardiac slice, roughly"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:side, 0:side]
    out = []
    for _ in range(n):
        img, lab = np.zeros((side, side)), np.zeros((side, side), np.uint8)
        for k in range(1, 4):
            cy, cx, r = rs.uniform(0.3, 0.7, 2).tolist() + [rs.uniform(0.08, 0.25)]
            d = np.hypot(yy - cy * side, xx - cx * side) < r * side
            img[d], lab[d] = rs.uniform(60, 220), k
        out.append(((img + rs.normal(0, 8, img.shape)).clip(0, 255).astype(np.uint8), lab))
    return out


def pipeline(crop):
    p = augment_zoo["acdc"]().pretrain
    if crop != 224:
        p = DevicePipeline(**{**{k: getattr(p, k) for k in ("rotation", "vflip", "hflip", "jitter", "total_freedom")},
                              "crop": crop})
    return p


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, 1e3 * (time.perf_counter() - t0) / iters


def pillow_rate(pairs, p, views):
    from PIL import Image, ImageEnhance
    rs = np.random.RandomState(0)
    crop = p.crop[0]
    ims = [(Image.fromarray(a), Image.fromarray(b)) for a, b in pairs[:16]]
    t0 = time.perf_counter()
    for v in range(views):
        img, lab = ims[v % len(ims)]
        ang, fv, fh = rs.uniform(-p.rotation, p.rotation), rs.uniform() < 0.5, rs.uniform() < 0.5
        y, x = (int(rs.uniform() * (SIDE - crop + 1)) for _ in range(2))
        for im, mode in ((img, Image.BILINEAR), (lab, Image.NEAREST)):
            im = im.rotate(ang, mode)
            if fv:
                im = im.transpose(Image.FLIP_TOP_BOTTOM)
            if fh:
                im = im.transpose(Image.FLIP_LEFT_RIGHT)
            im = im.crop((x, y, x + crop, y + crop))
            if mode == Image.BILINEAR:
                for enh in (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color):
                    im = enh(im).enhance(rs.uniform(0.5, 1.5))
                np.asarray(im, dtype=np.float32) / 255.0
            else:
                np.asarray(im).astype(np.int64)
    return views / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--pillow-views", type=int, default=64)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
    pairs = slices(SLICES, SIDE, 0)
    store = DeviceSliceStore.from_arrays([p[0] for p in pairs], [p[1] for p in pairs],
                                         [f"patient{i // 8:03d}_{i % 8:02d}" for i in range(SLICES)],
                                         group_re=r"patient\d+", device="cuda")
    print(f"store: {SLICES} slices of {SIDE}x{SIDE}, {2 * store.images.numel() / 2 ** 20:.0f} MiB; plan at 64 views of "
          f"224: {ops.augment_plan(64, 224, 224)}")
    print(f"{'workload':>8s} {'out':>4s} {'calls x views':>13s} | {'draw':>7s} {'batch':>7s} {'(host)':>7s} "
          f"{'kernels':>7s} (ms) | {'views/s':>9s}")
    rs = np.random.RandomState(1)
    for name, crop in (("c2", 224), ("c4", 256)):
        p = pipeline(crop)
        for calls, n in ((2, 16), (1, 32)):  # n slices, twice: 2n views per call
            index_lists = [[rs.randint(0, SLICES, size=n).tolist() for _ in range(calls)] for _ in range(a.iters + 2)]
            flat = [idx for step in index_lists for idx in step]
            loader = DeviceLoader(store, p, flat, twice=True, seed=3)
            it = iter(loader)
            for _ in range(2 * calls):
                next(it)  # warm-up: code objects, the pinned ring, the tables

            def one_step():
                for _ in range(calls):
                    next(it)

            t0 = time.perf_counter()
            for _ in range(a.iters):
                for idx in index_lists[0]:
                    p.draw_twice(n, 5, store.sizes(idx))
            draw_ms = 1e3 * (time.perf_counter() - t0) / a.iters
            pre = [np.concatenate([v.int_params for v in p.draw_twice(n, 5, store.sizes(index_lists[0][0]))]),
                   np.concatenate([v.f64_params for v in p.draw_twice(n, 5, store.sizes(index_lists[0][0]))])]
            pre[0][:, 0] = index_lists[0][0] * 2
            ip, fp = torch.from_numpy(pre[0]), torch.from_numpy(pre[1])

            def kernels():
                for _ in range(calls):
                    ops.augment_views(store.images, store.labels, store.table, ip, fp, None, (crop, crop))

            kernels()
            dev, host, ker = [], [], []
            for _ in range(a.rounds):
                it = iter(loader)
                d, h = timed(one_step, a.iters)
                dev.append(d), host.append(h)
                ker.append(timed(kernels, a.iters)[0])
            d, h, k = (statistics.median(v) for v in (dev, host, ker))
            views = calls * 2 * n
            print(f"{name:>8s} {crop:4d} {calls:>7d} x {2 * n:<3d} | {draw_ms:7.3f} {d:7.3f} {h:7.3f} {k:7.3f}      | "
                  f"{1e3 * views / max(d, h):9.0f}", flush=True)
        try:
            rate = pillow_rate(pairs, p, a.pillow_views)
            print(f"{name:>8s} {crop:4d} Pillow, one core: {rate:.0f} views/s; times 16: {16 * rate:.0f} views/s",
                  flush=True)
        except ImportError:
            print("Pillow is not installed here: no host figure", flush=True)


if __name__ == "__main__":
    main()
