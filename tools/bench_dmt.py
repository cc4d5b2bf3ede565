#!/usr/bin/env python3
"""Time of the differentiable mean teacher's bookkeeping and consistency term at the C2 shapes (U-Net with
max_channel = 512: 8.6 M parameters in about 70 tensors, 44 running statistics; 16 unlabeled slices of 224 x 224, K = 4),
fused against the unfused composition.  No network pass is timed.

    python tools/bench_dmt.py [--rounds 7] [--iters 20]        (on the GPU box, one process)

bookkeeping   what one step of the hooks does to the teacher's state besides running it:
    fused     FlatTeacher: ema_from (one cy_ema_update over the flat parameters, the student being FusedRAdam's, and one
              cy_ema_update_multi over the running statistics), snapshot, restore (three device copies each), adam_step
              (one cy_adam_step)
    torch     the per-tensor EMAUpdater(update_bn=True), deepcopy(state_dict()), load_state_dict, torch.optim.Adam
              (its default multi-tensor path on the GPU, and foreach=False: one launch group per tensor)
consistency   SoftmaxGatherMSEFn (cy_softmax_gathermse_*) forward + backward against softmax -> gather warp with zero
              padding -> MSELoss on the same logits and the same map (from AffineAugment through the index image)

The versions alternate round by round in one process; a figure is the median over the rounds of the mean of `iters`
back-to-back calls between two device events, after two warm-up calls of each: the time of a call as Python issues it,
not a kernel time.  The spread over the rounds is printed next to it.  Results of the two versions are compared once
before anything is timed."""
import argparse
import copy
import statistics
import sys
from pathlib import Path

import torch
from torch import nn

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "contrast-you_amd"))
from contrastyou.arch import UNet  # noqa: E402
from contrastyou.optim import FlatTeacher, RAdam  # noqa: E402
from cyhip import ops  # noqa: E402
from cyhip.functions import SoftmaxGatherMSEFn  # noqa: E402
from semi_seg.augment import AffineAugment  # noqa: E402
from semi_seg.hooks import EMAUpdater  # noqa: E402


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def table(title, fns, a):
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            t[k].append(events(fn, a.iters))
    print(title)
    for k, v in t.items():
        print(f"    {k:34s} median {statistics.median(v) * 1e3:9.1f} us   (min {min(v) * 1e3:9.1f}, max {max(v) * 1e3:9.1f})",
              flush=True)


def warp_by_map(x, m):
    N, C = x.shape[:2]
    idx = m.reshape(N, 1, -1)
    got = x.reshape(N, C, -1).gather(2, idx.clamp_min(0).long().expand(N, C, -1))
    return (got * (idx >= 0).to(x.dtype)).reshape(x.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--max-channel", type=int, default=512)
    ap.add_argument("--slices", type=int, default=16)
    ap.add_argument("--hw", type=int, default=224)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
    dev = "cuda"
    torch.manual_seed(1)
    student = UNet(input_dim=1, num_classes=4, max_channel=a.max_channel, momentum=0.01).to(dev)
    opt = RAdam(list(student.parameters()), lr=1e-3)
    opt.zero_grad()  # flattens the student's parameters
    n_par = sum(p.numel() for p in student.parameters())
    n_stat = sum(b.numel() for b in student.buffers() if b.is_floating_point())
    print(f"U-Net max_channel={a.max_channel}: {n_par} parameters in {len(list(student.parameters()))} tensors, "
          f"{n_stat} running statistics in {sum(b.is_floating_point() for b in student.buffers())} tensors")

    # ---- bookkeeping
    fused_model, plain_model = copy.deepcopy(student), copy.deepcopy(student)
    flat = FlatTeacher(fused_model)
    flat.flat.grad.normal_()
    for p in plain_model.parameters():
        p.grad = torch.randn_like(p)
    up_f, up_p = EMAUpdater(update_bn=True), EMAUpdater(update_bn=True)
    up_f._global_step = up_p._global_step = 10
    adam = {fe: torch.optim.Adam(plain_model.parameters(), lr=1e-3, weight_decay=1e-5, foreach=fe)
            for fe in (None, False)}
    keep = {}

    def plain_snapshot():
        keep["ckpt"] = copy.deepcopy(plain_model.state_dict())

    plain_snapshot()
    table("teacher bookkeeping, per call:", {
        "fused ema_from": lambda: flat.ema_from(student, up_f),
        "torch EMAUpdater (per tensor)": lambda: up_p(ema_model=plain_model, student_model=student),
        "fused snapshot": flat.snapshot,
        "torch deepcopy(state_dict())": plain_snapshot,
        "fused restore": flat.restore,
        "torch load_state_dict": lambda: plain_model.load_state_dict(keep["ckpt"]),
        "fused adam_step": lambda: flat.adam_step(1e-3, 1e-5),
        "torch Adam (multi-tensor)": adam[None].step,
        "torch Adam (foreach=False)": adam[False].step,
    }, a)

    def fused_all():
        flat.ema_from(student, up_f), flat.snapshot(), flat.restore(), flat.adam_step(1e-3, 1e-5)

    def torch_all():
        up_p(ema_model=plain_model, student_model=student), plain_snapshot()
        plain_model.load_state_dict(keep["ckpt"]), adam[None].step()

    table("teacher bookkeeping of one step (EMA + snapshot + restore + Adam):",
          {"fused": fused_all, "torch": torch_all}, a)

    # ---- consistency term
    N, K, H = a.slices, 4, a.hw
    gen = torch.Generator(device=dev).manual_seed(7)
    teacher = (torch.randn(N, H, H, K, device=dev, generator=gen) * 2).permute(0, 3, 1, 2)
    s = (torch.randn(N, H, H, K, device=dev, generator=gen) * 2).permute(0, 3, 1, 2).requires_grad_(True)
    aug = AffineAugment(scale=(0.8, 1.3), rotation=(-45, 45), translation=(-0.1, 0.1), mirror_p=0.9, gamma=(0.5, 2))
    smap = ops.source_map_from_warped(aug(ops.source_index_image(N, H, H, dev), mode="feature", seed=3))
    print(f"consistency term at {N}x{K}x{H}x{H}, {float((smap < 0).float().mean()) * 100:.1f} % of the pixels outside")
    mse = nn.MSELoss()
    fns = {"fused": lambda: SoftmaxGatherMSEFn.apply(teacher, smap, s),
           "torch": lambda: mse(warp_by_map(teacher.softmax(1), smap.view(N, -1)), s.softmax(1))}
    res = {}
    for k, fn in fns.items():
        s.grad = None
        v = fn()
        v.backward()
        res[k] = (float(v.detach()), s.grad.clone())
    rel = float((res["fused"][1] - res["torch"][1]).abs().max() / res["torch"][1].abs().max())
    print(f"    loss {res['fused'][0]:.8f} vs {res['torch'][0]:.8f}, gradients differ by {rel:.1e}")

    def fb(fn):
        def run():
            s.grad = None
            fn().backward()
        return run

    table("consistency term, forward + backward:", {k: fb(fn) for k, fn in fns.items()}, a)
    npix = N * H * H
    print(f"    algorithmic bytes of the fused form: forward {npix * (8 * K + 4) / 2 ** 20:.1f} MiB, "
          f"backward {npix * (12 * K + 4) / 2 ** 20:.1f} MiB")


if __name__ == "__main__":
    main()
