#!/usr/bin/env python3
"""Time of one optimizer step on the U-Net's own parameter list (UNet(max_channel=512), the C2 model: 8.6 M parameters
in about 70 tensors), fused flat-buffer optimizers against torch.optim's default (foreach) form on the same GPU, and of
each streaming kernel on the whole flat buffer with its bytes per second.  No network pass is timed.

    python tools/bench_optim.py [--rounds 7] [--iters 20]        (on the GPU box, one process)

kernels   one launch over the whole group (n = all parameters): cy_radam_step -- the yardstick, timed in the same run --,
          cy_sgd_step without and with momentum, cy_adam_step, cy_adamw_step without and with amsgrad.  GB/s is the
          algorithmic traffic over the time of a call: 12 B/element for SGD without momentum (read p, g; write p), 20 with
          it, 28 for RAdam and Adam(W), 36 with amsgrad.
steps     FusedSGD(momentum=0.9) / FusedAdam / FusedAdamW / FusedRAdam .step() with every parameter touched, against
          torch.optim.SGD / Adam / AdamW / RAdam .step() in their default form on per-tensor copies with the same
          gradients.

The versions alternate round by round in one process; a figure is the median over the rounds of the mean of `iters`
back-to-back calls between two device events, after two warm-up calls of each: the time of a call as Python issues it
(for the kernels: launches queued back to back, so the kernel time plus the gap between two launches), not a profiler's
kernel time.  The spread over the rounds is printed next to it.  The buffers of one call (35 MB each, 3 to 5 of them)
are the same in every call, so a part of them may be served by the last-level cache: compare the rates with each other
and with cy_radam_step's, not with the HBM peak."""
import argparse
import copy
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "contrast-you_amd"))
from contrastyou import optim  # noqa: E402
from contrastyou.arch import UNet  # noqa: E402
from cyhip import ops  # noqa: E402


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def table(title, fns, a, nbytes=None):
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
        med = statistics.median(v)
        rate = f"   {nbytes[k] / (med * 1e-3) / 1e9:7.0f} GB/s" if nbytes else ""
        print(f"    {k:34s} median {med * 1e3:9.1f} us   (min {min(v) * 1e3:9.1f}, max {max(v) * 1e3:9.1f}){rate}",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--max-channel", type=int, default=512)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
    dev = "cuda"
    torch.manual_seed(1)
    model = UNet(input_dim=1, num_classes=4, max_channel=a.max_channel, momentum=0.01).to(dev)
    n = sum(p.numel() for p in model.parameters())
    print(f"U-Net max_channel={a.max_channel}: {n} parameters in {len(list(model.parameters()))} tensors, "
          f"{4 * n / 2 ** 20:.1f} MiB per flat buffer")

    # ---- the kernels on one flat buffer
    p, g, m = (torch.randn(n, device=dev) * s for s in (1.0, 0.01, 0.01))
    v, vmax = torch.rand(n, device=dev) * 1e-4 + 1e-8, torch.rand(n, device=dev) * 1e-4 + 1e-8
    hyp = (1e-6, 0.9, 0.999, 1e-8, 1e-5)   # a small lr: the parameters stay put over the timed calls
    kernels = {
        "cy_radam_step (yardstick)": (28, lambda: ops.radam_step(p, g, m, v, *hyp, 1000)),
        "cy_sgd_step": (12, lambda: ops.sgd_step(p, g, None, 1e-6, 0.0, 0.0, 1e-5, False, False)),
        "cy_sgd_step momentum": (20, lambda: ops.sgd_step(p, g, m, 1e-6, 0.9, 0.0, 1e-5, False, False)),
        "cy_adam_step": (28, lambda: ops.adam_step(p, g, m, v, *hyp, 1000)),
        "cy_adamw_step": (28, lambda: ops.adamw_step(p, g, m, v, None, *hyp, True, 1000)),
        "cy_adamw_step amsgrad": (36, lambda: ops.adamw_step(p, g, m, v, vmax, *hyp, True, 1000)),
    }
    table("kernels, one launch over the whole buffer:", {k: fn for k, (_, fn) in kernels.items()}, a,
          nbytes={k: b * n for k, (b, _) in kernels.items()})
    del p, g, m, v, vmax

    # ---- the optimizers' step()
    grads = [torch.randn_like(q) * 0.01 for q in model.parameters()]
    pairs = (("SGD", dict(lr=1e-6, momentum=0.9, weight_decay=1e-5)), ("Adam", dict(lr=1e-6, weight_decay=1e-5)),
             ("AdamW", dict(lr=1e-6, weight_decay=1e-2)), ("RAdam", dict(lr=1e-6, weight_decay=1e-5)))
    fns = {}
    for name, kw in pairs:
        mine, theirs = copy.deepcopy(model), copy.deepcopy(model)
        fused = getattr(optim, name)(list(mine.parameters()), **kw)
        fused.zero_grad()   # flattens the parameters
        for q, gq in zip(mine.parameters(), grads):
            q.grad.copy_(gq)
            q.__dict__["_cy_touched"] = True   # what the kernels' accumulation (or autograd's hook) leaves
        plain = getattr(torch.optim, name)(list(theirs.parameters()), **kw)
        for q, gq in zip(theirs.parameters(), grads):
            q.grad = gq.clone()
        fns[f"Fused{name}.step()"] = fused.step
        fns[f"torch.optim.{name}.step()"] = plain.step
    table("optimizer step, every parameter updated:", fns, a)


if __name__ == "__main__":
    main()
