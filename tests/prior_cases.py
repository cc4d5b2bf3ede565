"""The cases of the DAE-prior and orthogonality kernels (csrc/cy_prior.hip), the float64 restatement of their two
formulas, the reference's composition in f32 (what the kernels' bounds are measured from) and the layout of
tests/golden/prior.npz.  Shared by tests/golden/gen_goldens_prior.py, tests/test_prior_host.py and
tests/test_gpu_prior.py.

DAE cases: the smallest shapes at which each thing can go wrong.
    K        2, 4, 8 compiled on aligned rows; 3, 5, 16, 17, 40, 64 run-time (1, 2, 3 and 4 pieces of 16 floats; 16, 40
             and 64 read four floats at a time); 2, 4, 8, 16 on a base that is only 4-byte aligned (a slice that starts
             one float into its buffer): the run-time form, one float at a time
    npix     1; 70 = 2 x 5 x 7 (two images in one block); 257 (a one-pixel last block); 513 x 512 (1026 blocks' worth:
             a second trip past the 1024-block cap, forward and backward)
    layout   "nchw" (the binding makes the NHWC copy), "cl" (channels-last, read in place), "slice"
    Cimg     1..4, act sigmoid / tanh
    reach    what the largest |pre-activation| is scaled to; 30 saturates the sigmoid (its f32 gradient underflows to 0)
Orthogonality cases: (K, C) with both tensor ranks; "zero": row 1 is all zeros (forward only).

Bounds (`bounds`): for each kind the reference's composition is evaluated in f32 with torch on the CPU over the same
cases; its largest distance from float64 is e_ref, and a kernel may be 4 e_ref away (the kernels sum in f64 and should
sit below the reference; the device's expf and tanhf differ from the host's by a couple of ulp; a dropped term, a wrong
divisor or a missing act' moves a result by 1e-3 or more).  A loss's bound is floored at 1.2e-6.  Measured on an
MI355X (DESIGN.md section 3 has the table):
    kind            e_ref     bound     kernel (largest over the cases)
    dae loss        1.57e-7   1.20e-6   5.0e-8
    dae grad2       2.31e-6   9.26e-6   1.43e-6
    dae gradmax     2.31e-6   9.26e-6   1.43e-6
    ortho loss      4.05e-7   1.62e-6   1.14e-7
    ortho grad2     4.83e-7   1.93e-6   1.97e-7
    ortho gradmax   6.35e-7   2.54e-6   3.67e-7
The DAE gradient figures are set by db of k17_70, a sum of per-pixel terms that nearly cancels (its own norm is small);
every other case is within 6e-7 in the kernels.
"""
from collections import namedtuple
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

MARGIN = 4.0
LOSS_FLOOR = 1.2e-6
KINDS = ("loss", "grad2", "gradmax")

Dae = namedtuple("Dae", "tag K N H W Cimg act layout reach")
DAE_CASES = (
    Dae("k2_1px", 2, 1, 1, 1, 1, "sigmoid", "nchw", 3.0),
    Dae("k3_70_c3", 3, 2, 5, 7, 3, "tanh", "nchw", 3.0),
    Dae("k4_70_cl", 4, 2, 5, 7, 1, "sigmoid", "cl", 3.0),
    Dae("k5_70_c2", 5, 2, 5, 7, 2, "sigmoid", "cl", 3.0),
    Dae("k8_257_c2", 8, 1, 1, 257, 2, "sigmoid", "cl", 3.0),
    Dae("k16_257_c4", 16, 1, 257, 1, 4, "tanh", "nchw", 3.0),
    Dae("k17_70", 17, 2, 5, 7, 1, "sigmoid", "nchw", 3.0),
    Dae("k40_70_c2", 40, 2, 5, 7, 2, "tanh", "cl", 3.0),
    Dae("k64_257", 64, 1, 1, 257, 1, "sigmoid", "cl", 3.0),
    Dae("k2_70_slice", 2, 2, 5, 7, 1, "tanh", "slice", 3.0),
    Dae("k4_257_slice", 4, 1, 1, 257, 1, "sigmoid", "slice", 3.0),
    Dae("k8_70_slice", 8, 2, 5, 7, 3, "sigmoid", "slice", 3.0),
    Dae("k16_70_slice", 16, 2, 5, 7, 1, "tanh", "slice", 3.0),
    Dae("k3_257", 3, 1, 257, 1, 1, "sigmoid", "cl", 3.0),
    Dae("k4_70_sat", 4, 2, 5, 7, 1, "sigmoid", "cl", 30.0),
    Dae("k4_70_sat_tanh", 4, 2, 5, 7, 2, "tanh", "nchw", 30.0),
    Dae("k2_past_cap", 2, 1, 513, 512, 1, "sigmoid", "cl", 3.0),
)
DAE_BY_TAG = {c.tag: c for c in DAE_CASES}

Ortho = namedtuple("Ortho", "tag K C rank zero")
ORTHO_CASES = (
    Ortho("k2_c1", 2, 1, 2, False),
    Ortho("k4_c16", 4, 16, 4, False),
    Ortho("k12_c16", 12, 16, 4, False),
    Ortho("k64_c16", 64, 16, 2, False),
    Ortho("k64_c256", 64, 256, 4, False),
    Ortho("k3_c5461", 3, 5461, 2, False),
    Ortho("k17_c64", 17, 64, 2, False),
    Ortho("k4_c16_zero", 4, 16, 4, True),
)
ORTHO_BY_TAG = {c.tag: c for c in ORTHO_CASES}

# what tests/golden/prior.npz holds of the reference's own hooks (tests/golden/gen_goldens_prior.py)
AUX_INIT = ((2, 11), (4, 12), (5, 13))  # (K, torch.manual_seed) of the recorded AuxiliaryLayer state dicts
HOOK_DAE = (dict(tag="dae_a", K=4, N=2, H=9, W=7, Cimg=1, weight=0.3, seed=12),
            dict(tag="dae_b", K=5, N=1, H=6, W=5, Cimg=3, weight=0.7, seed=13))
HOOK_ORTHO = (dict(tag="ortho_a", K=4, C=16, weight=0.3), dict(tag="ortho_b", K=12, C=16, weight=0.7))
# the steps of tests/test_gpu_prior.py
STEP_DAE = dict(weight=0.1, K=4)
STEP_ORTHO = dict(weight=0.05, true_classes=2, multiplier=2)


def _rng(tag: str) -> np.random.RandomState:
    return np.random.RandomState(sum(ord(c) * (i + 1) for i, c in enumerate(tag)) % (2 ** 31))


def load(golden_dir):
    return dict(np.load(Path(golden_dir) / "prior.npz"))


def dae_inputs(case: Dae):
    """(logits f32 [N,K,H,W], weight f32 [K], bias f32 [1], image f32 [N,Cimg,H,W]), contiguous CPU tensors.  Logits
    on the 1/8 grid with a per-image spread; the weight is scaled so that max |b + w . z| is the case's reach"""
    r = _rng(case.tag)
    z = r.standard_normal((case.N, case.K, case.H, case.W)) * (0.25 + 2.0 * r.random_sample((case.N, 1, 1, 1)))
    z = (np.clip(np.round(z * 8), -48, 48) / 8).astype(np.float32)
    w = r.standard_normal(case.K)
    b = 0.25 * r.standard_normal(1)
    pre = np.abs(b + np.einsum("nkhw,k->nhw", z.astype(np.float64), w)).max()
    w, b = w * (case.reach / pre), b * (case.reach / pre)
    img = r.random_sample((case.N, case.Cimg, case.H, case.W))
    if case.act == "tanh":
        img = 2 * img - 1
    return (torch.from_numpy(z), torch.from_numpy(w.astype(np.float32)), torch.from_numpy(b.astype(np.float32)),
            torch.from_numpy(img.astype(np.float32)))


def ortho_inputs(case: Ortho):
    """prototypes f32 [K,C] or [K,C,1,1]: rows of very different lengths; "zero": row 1 is all zeros"""
    r = _rng(case.tag)
    v = r.standard_normal((case.K, case.C)) * np.exp(r.uniform(-3, 3, (case.K, 1)))
    if case.zero:
        v[1] = 0.0
    v = torch.from_numpy(v.astype(np.float32))
    return v.view(case.K, case.C, 1, 1) if case.rank == 4 else v


# ---- the two formulas in float64 ---------------------------------------------------------------------------------------
def dae64(logits, weight, bias, image, act: str):
    """mean over N Cimg H W of (act(b + sum_k w_k z_k) - image)^2"""
    z, w, b, img = (t.double() for t in (logits, weight, bias, image))
    s = b.reshape(1, 1, 1, 1) + (z * w.reshape(1, -1, 1, 1)).sum(1, keepdim=True)
    r = torch.tanh(s) if act == "tanh" else torch.sigmoid(s)
    return ((r - img) ** 2).sum() / img.numel()


def ortho64(prototypes):
    """mean over K^2 of (n n^T - I)^2, n_i = v_i / max(|v_i|, 1e-12)"""
    v = prototypes.double().reshape(prototypes.shape[0], prototypes.shape[1])
    n = v / v.pow(2).sum(1, keepdim=True).sqrt().clamp_min(1e-12)
    g = n @ n.t() - torch.eye(v.shape[0], dtype=torch.float64)
    return g.pow(2).sum() / g.numel()


# ---- the reference's composition, in the dtype of its inputs (f32: what e_ref is measured on) ---------------------------
def dae_composed(logits, weight, bias, image, act: str):
    r = F.conv2d(logits, weight.reshape(1, -1, 1, 1), bias.reshape(1))
    r = torch.tanh(r) if act == "tanh" else torch.sigmoid(r)
    return F.mse_loss(r.expand_as(image), image)  # (F.mse_loss's own broadcast over the channels, without its warning)


def ortho_composed(prototypes):
    n = F.normalize(prototypes, p=2, dim=1)
    n = n.squeeze() if n.dim() == 4 else n
    m = n @ n.t()
    return (m - torch.eye(m.shape[0], device=m.device, dtype=m.dtype)).pow(2).mean()


def grads_of(fn, *tensors, wrt):
    """(value, [gradients of the tensors at the positions `wrt`]), all detached"""
    leaves = [t.detach().clone().requires_grad_(i in wrt) for i, t in enumerate(tensors)]
    v = fn(*leaves)
    v.backward()
    return v.detach(), [leaves[i].grad.detach() for i in wrt]


# ---- distances ---------------------------------------------------------------------------------------------------------
def rel_scalar(v, ref) -> float:
    v, ref = float(v), float(ref)
    return abs(v - ref) / max(abs(ref), 1e-300)


def rel_grad(g, ref):
    """(2-norm, max-norm) of g - ref, each relative to the same norm of the float64 gradient"""
    g, ref = g.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    d = g - ref
    return (float(d.norm() / ref.norm().clamp_min(1e-300)), float(d.abs().max() / ref.abs().max().clamp_min(1e-300)))


def errors(value, grads, value64, grads64):
    """[loss, grad2, gradmax]: the gradients' distances are the largest over the tensors"""
    pairs = [rel_grad(g, r) for g, r in zip(grads, grads64)]
    return [rel_scalar(value, value64), max(p[0] for p in pairs), max(p[1] for p in pairs)]


def dae_reference(case: Dae):
    """(f64 value, f64 gradients [dlogits, dw, db], the f32 composition's errors) of a DAE case"""
    z, w, b, img = dae_inputs(case)
    v64, g64 = grads_of(lambda a, c, d, e: dae64(a, c, d, e, case.act), z, w, b, img, wrt=(0, 1, 2))
    v32, g32 = grads_of(lambda a, c, d, e: dae_composed(a, c, d, e, case.act), z, w, b, img, wrt=(0, 1, 2))
    return v64, g64, errors(v32, g32, v64, g64)


def ortho_reference(case: Ortho):
    """(f64 value, [f64 gradient], the f32 composition's errors); a zero row's gradient is not compared: None"""
    v = ortho_inputs(case)
    if case.zero:
        v64 = ortho64(v)
        return v64, None, [rel_scalar(ortho_composed(v), v64), 0.0, 0.0]
    v64, g64 = grads_of(ortho64, v, wrt=(0,))
    v32, g32 = grads_of(ortho_composed, v, wrt=(0,))
    return v64, g64, errors(v32, g32, v64, g64)


def bounds(refs):
    """{kind: (e_ref, bound)} from the third items of the references of a family's cases"""
    out = {}
    for i, kind in enumerate(KINDS):
        e_ref = max(r[2][i] for r in refs)
        out[kind] = (e_ref, max(MARGIN * e_ref, LOSS_FLOOR) if kind == "loss" else MARGIN * e_ref)
    return out
