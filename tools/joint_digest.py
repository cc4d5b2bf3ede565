#!/usr/bin/env python3
"""One SHA-256 per output tensor of the joint kernels of csrc/cy_mi.hip (whole-image and patch-wise, forward and
backward) on inputs from fixed CPU seeds: two builds whose listings agree compute the same bytes.

    python tools/joint_digest.py [--lib path/to/libcontrastyou_hip.so]        (on the GPU box, a fresh process per build)

The cases are the test suite's own: every mi_cases.JOINT_CASES forward (normalise on where pad == 0), every
mi_cases.BWD_CASES backward (dx1 / dx2 as the case asks), and every patch_losses_fixture.PATCH_CASES entry plus
patch_losses_cases.MULTI_TRIP: the forward under kernel="staged" where the staged tile fits, the forward under
kernel="per_displacement", and joint_patch_bwd with a seeded dJ.  A digest is over the bytes of `.cpu().contiguous()`."""
import argparse
import hashlib
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "contrast-you_amd"), str(REPO / "tests")]
import mi_cases as mc  # noqa: E402
import patch_losses_cases as pc  # noqa: E402
import patch_losses_fixture as fx  # noqa: E402
from cyhip import _lib, ops  # noqa: E402

DEV = "cuda"
count = 0


def show(name, t):
    global count
    count += 1
    print(f"{hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()}  {name}", flush=True)


def maps(seed, shape, k, masked=False):
    """two softmaxed `randn * 2` maps [N,H,W,k] on the GPU; masked: a quarter of the pixels of both are zero"""
    g = torch.Generator().manual_seed(seed)
    n, h, w = shape
    x1, x2 = (torch.softmax(torch.randn(n, h, w, k, generator=g) * 2, -1) for _ in range(2))
    if masked:
        keep = (torch.rand(n, h, w, 1, generator=g) >= 0.25).float()
        x1, x2 = x1 * keep, x2 * keep
    return x1.to(DEV), x2.to(DEV), g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", type=Path, default=None, help="the build to load instead of contrast-you_amd/lib")
    a = ap.parse_args()
    if a.lib is not None:
        _lib.LIB_PATH = a.lib.resolve()
    assert torch.cuda.is_available(), "needs the GPU"
    for i, c in enumerate(mc.JOINT_CASES):
        x1, x2, _ = maps(1000 + i, c.shape, c.k, c.masked)
        show(f"joint_fwd {mc.case_id(c)}", ops.joint_fwd(x1, x2, *c.shape, c.k, c.pad, c.pad == 0))
    for i, c in enumerate(mc.BWD_CASES):
        x1, x2, g = maps(2000 + i, c.shape, c.k)
        T = 2 * c.pad + 1
        dJ = torch.randn(T * T, c.k, c.k, generator=g).to(DEV)
        gs = torch.tensor([c.gscale], device=DEV)
        d = ops.joint_bwd(x1, x2, dJ, gs, *c.shape, c.k, c.pad, c.normalise, "1" in c.need, "2" in c.need)
        for name, t in zip(("dx1", "dx2"), d):
            if t is not None:
                show(f"joint_bwd {mc.case_id(c)} {name}", t)
    npz = fx.load(REPO / "tests" / "golden")
    cases = dict(fx.PATCH_CASES, multi_trip=pc.MULTI_TRIP)
    for i, (tag, (n, k, H, W, patch, pad)) in enumerate(cases.items()):
        g = torch.Generator().manual_seed(3000 + i)
        if tag in fx.PATCH_CASES:
            x1, x2 = (p.permute(0, 2, 3, 1).contiguous().to(DEV) for p in fx.inputs(npz, tag))
        else:
            x1, x2 = (torch.softmax(torch.randn(n, H, W, k, generator=g) * 2, -1).to(DEV) for _ in range(2))
        if ops.joint_patch_plan(n, H, W, k, pad, patch)["staged_fits"]:
            show(f"joint_patch_fwd {tag} staged", ops.joint_patch_fwd(x1, x2, pad, patch, pad == 0, kernel="staged"))
        J = ops.joint_patch_fwd(x1, x2, pad, patch, pad == 0, kernel="per_displacement")
        show(f"joint_patch_fwd {tag} per_displacement", J)
        dJ = torch.randn(J.shape, generator=g).to(DEV)
        d1, d2 = ops.joint_patch_bwd(x1, x2, dJ, torch.tensor([0.75], device=DEV), pad, patch, pad == 0)
        show(f"joint_patch_bwd {tag} dx1", d1)
        show(f"joint_patch_bwd {tag} dx2", d2)
    torch.cuda.synchronize()
    print(f"{count} tensors")


if __name__ == "__main__":
    main()
