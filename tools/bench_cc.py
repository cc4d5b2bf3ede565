#!/usr/bin/env python3
"""Timings of the cross-correlation kernels (csrc/cy_cc.hip) and of one whole _CrossCorrelationHook call at the
production size, 16 x 224 x 224 with K = 10 and K = 20, windows 3 / 5 / 7 -- next to the same formulas evaluated
with torch-ROCm ops on the same GPU in the same process (what a user would otherwise run), the two alternating.

Two numbers per entry: `gpu` = device time of back-to-back executions (the host enqueues `iters` repetitions behind
a spin kernel, timing-only events around them), with the algorithmic bytes over it; `issue` = host wall time per
call when the host is the limit (what the eager section of a step pays).  Prints one line per entry.
"""
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "contrast-you_amd"))
from cyhip import _lib, ops  # noqa: E402

DEV = "cuda"


def gpu_us(fn, iters=20):
    """device time per call, the calls queued behind a 3 ms spin so that they run back to back"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    _lib.call("cy_debug_spin", 3000, ops._stream())
    e0, e1 = ops.TimingEvent().record(), None
    for _ in range(iters):
        fn()
    e1 = ops.TimingEvent().record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def issue_us(fn, iters=50):
    """host wall time per call with an empty queue in front (enqueue + execution, whichever is longer)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def line(name, hip, ref, nbytes=None):
    g, i = (min(gpu_us(hip), gpu_us(hip)), min(issue_us(hip), issue_us(hip)))
    txt = f"{name:46s} hip gpu {g:8.1f} us  issue {i:8.1f} us"
    if nbytes:
        txt += f"  {nbytes / g / 1e3:7.1f} GB/s"
    if ref is not None:
        # alternate: torch, hip, torch -- the HIP figure above is bracketed by the two torch runs
        rg = min(gpu_us(ref), gpu_us(ref))
        g2 = gpu_us(hip)
        ri = min(issue_us(ref), issue_us(ref))
        txt += f" | torch gpu {rg:8.1f} us  issue {ri:8.1f} us | hip again {g2:8.1f} us"
    print(txt, flush=True)


# ---- the same formulas on torch ops (ccblock.py:278-309, cross_correlation.py:22-74 restated)
def t_norm(x):
    lo, hi = x.amin(dim=(1, 2, 3), keepdim=True).detach(), x.amax(dim=(1, 2, 3), keepdim=True).detach()
    return (x - lo) / (hi - lo + 1e-6)


def t_edge(img, power):
    d = ((img - img.roll(1, 2)) ** 2 + (img - img.roll(1, 3)) ** 2).sqrt().mean(1, keepdim=True)
    return t_norm(d) ** power


def t_entropy(p):
    return t_norm(-(p * (p + 1e-16).log()).sum(1, keepdim=True))


def t_ccloss(I, J, filt, eps=1e-5):
    k = filt.shape[-1]
    n = float(k * k)
    sums = [F.conv2d(t, filt, padding=k // 2) for t in (I, J, I * I, J * J, I * J)]
    uI, uJ = sums[0] / n, sums[1] / n
    cross = (sums[4] - uJ * sums[0] - uI * sums[1] + uI * uJ * n).clamp_min(eps)
    ivar = (sums[2] - 2 * uI * sums[0] + uI * uI * n).clamp_min(eps)
    jvar = (sums[3] - 2 * uJ * sums[1] + uJ * uJ * n).clamp_min(eps)
    return -(cross * cross / (ivar * jvar)).mean()


def main():
    from semi_seg.hooks.ccblock import _CrossCorrelationHook
    torch.manual_seed(0)
    n, hw = 16, 224
    npix = n * hw * hw
    img = torch.rand(n, 1, hw, hw, device=DEV)
    img2 = torch.rand(n, 1, 2 * hw, 2 * hw, device=DEV)
    one = torch.ones(1, device=DEV)
    print(f"# {n} x {hw} x {hw}, f32; device {torch.cuda.get_device_name(0)}")
    line("edge_map (2 launches)", lambda: ops.cc_edge_map(img, 0.75), lambda: t_edge(img, 0.75), 3 * npix * 4)
    J = ops.cc_edge_map(img, 0.75)
    for K in (10, 20):
        prob = torch.randn(n, hw, hw, K, device=DEV).mul(3).softmax(-1).permute(0, 3, 1, 2)  # NHWC memory
        pc = prob.contiguous()  # what torch's ops get: NCHW
        line(f"entropy_map_fwd K={K} (2 launches)", lambda: ops.entropy_map_fwd(prob, True), lambda: t_entropy(pc),
             npix * (K + 3) * 4)
        I, mm = ops.entropy_map_fwd(prob, True)
        g = torch.rand_like(I)
        pl = pc.clone().requires_grad_(True)
        el = t_entropy(pl)
        line(f"entropy_map_bwd K={K}", lambda: ops.entropy_map_bwd(prob, mm, g),
             lambda: torch.autograd.grad(el, pl, g, retain_graph=True), npix * (2 * K + 1) * 4)
    for win in (3, 5, 7):
        filt = torch.ones(1, 1, win, win, device=DEV)
        line(f"ccloss_fwd win {win} (2 launches)", lambda: ops.ccloss_fwd(I, J, win, 1e-5),
             lambda: t_ccloss(I, J, filt), 2 * npix * 4)
        Il = I.clone().requires_grad_(True)
        ll = t_ccloss(Il, J, filt)
        line(f"ccloss_bwd win {win} (dI)", lambda: ops.ccloss_bwd(I, J, one, win, 1e-5, True, False),
             lambda: torch.autograd.grad(ll, Il, retain_graph=True), 3 * npix * 4)
        Jl = J.clone().requires_grad_(True)
        l2 = t_ccloss(Il, Jl, filt)
        line(f"ccloss_bwd win {win} (dI, dJ)", lambda: ops.ccloss_bwd(I, J, one, win, 1e-5, True, True),
             lambda: torch.autograd.grad(l2, (Il, Jl), retain_graph=True), 4 * npix * 4)
    # one whole hook call: two heads, forward + backward
    for K in (10, 20):
        p1 = torch.randn(n, hw, hw, K, device=DEV).mul(3).softmax(-1).permute(0, 3, 1, 2).requires_grad_(True)
        p2 = torch.randn(n, hw, hw, K, device=DEV).mul(3).softmax(-1).permute(0, 3, 1, 2).requires_grad_(True)
        c1, c2 = (p.detach().contiguous().requires_grad_(True) for p in (p1, p2))
        for win in (3, 5, 7):
            tiny = _CrossCorrelationHook(weight=1.0, kernel_size=win)
            filt = torch.ones(1, 1, win, win, device=DEV)

            def hip(image=img):
                p1.grad = p2.grad = None
                tiny._edges.clear()  # a new image every step
                tiny(image=image, input1=p1, input2=p2).backward()

            def ref(image=img):
                c1.grad = c2.grad = None
                if image.shape[-1] != hw:
                    image = F.interpolate(image, size=(hw, hw), mode="bilinear")
                e = t_edge(image, 0.75)
                (sum(t_ccloss(t_entropy(c), e, filt) for c in (c1, c2)) / 2).backward()

            line(f"hook call fwd+bwd K={K} win {win} (14 launches)", hip, ref)
        line(f"hook call fwd+bwd K={K} win 7, image 448 (15)", lambda: hip(img2), lambda: ref(img2))


if __name__ == "__main__":
    main()
