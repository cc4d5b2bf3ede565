"""Layout and decoding of tests/golden/imsat.npz (written by tests/golden/gen_goldens_imsat.py): the reference's IMSAT
family -- `imsat_with_entropy`, `imsat_loss`, `IMSATLoss`, `IMSATDynamicWeight` (contrastyou/losses/discreteMI.py:20-87,
275-297) and the `_call_implementation` of `_IMSATEpochHook` (semi_seg/hooks/midl.py:71-90) and
`_DiscreteIMSATEpochHook` (semi_seg/hooks/discretemi.py:136-167) -- evaluated on the CPU in f32 and in f64.

Inputs are stored as int8 logits on a 1/8 grid (`*_i8d8`), exact in f32: `decode` rebuilds them, `probs` takes the
f32 softmax, and the f64 runs read those f32 probabilities cast up, so both precisions (and the kernels) read the same
numbers.  The one-hot case is built directly (`onehot_rows`), not through a softmax.

Per row case `<tag>` (K clusters, R rows):
    <tag>_z_i8d8 [R,K]      (4-D cases: [b,K,H,W]); pair cases also <tag>_z2_i8d8
    <tag>_marg64, _cond64   imsat_with_entropy in f64
    <tag>_loss64            imsat_loss(p, LAMDA) in f64 = IMSATLoss(LAMDA)(p)
    <tag>_g64               d loss / d p in f64, rounded to f32
    <tag>_e_ref             the reference's own f32-to-f64 distances [scalars, gradient 2-norm, gradient max-norm]
pair cases: <tag>_pair_loss64, _pair_g1_64, _pair_g2_64, _pair_e_ref of IMSATLoss(LAMDA)(p, p2).
Dynamic weight: dyn_off_loss64, dyn_off_w64; dyn_loss64 [3], dyn_w64 [3] (after each call), dyn_g64 (first call),
dyn_e_ref.  Hooks: out_* (output hook), mid_* (intermediate hook): value64, gradients, meters, e_ref.

Distances are relative.  The two entropies are compared as one vector (marg, cond): |d|_2 / |(marg64, cond64)|_2 --
one-hot rows have cond64 = -1e-8 while f32 gives exactly 0, which no relative error of cond alone can express.  A
composite value a*marg + b*cond is held to tol * (|a marg64| + |b cond64|).  Gradients: 2-norm and max-norm over all
elements, relative to the f64 gradient's.  The tolerance of a kind is max(4 * the largest stored e_ref of that kind,
1e-6) (`tolerances`), taken over two groups so that neither widens the other's bound: the intermediate hook, whose
gradients run back through the cluster head (its own e_ref is some 40 times the others'), and everything else.
"""
from pathlib import Path

import numpy as np
import torch

LAMDA = 0.7
EPS = 1e-8

# every K of {2, 3, 5, 20, 40, 63, 64} and every R of {1, 255, 257, 3*19*19}; not the full product, which would not fit
# the size limit of a committed file with its gradients
ROW_SHAPES = ((2, 1), (2, 255), (2, 257), (2, 1083), (3, 257), (3, 1083), (5, 1), (5, 255), (20, 1083), (40, 255),
              (63, 1), (63, 255), (64, 1), (64, 257))
ROW_CASES = {f"k{K}_r{R}": (K, R) for K, R in ROW_SHAPES}
MAP_CASES = {"map_nchw": (3, 5, 19, 19), "map_nhwc": (3, 5, 19, 19)}  # R = 3*19*19, one per memory format
ONEHOT = ("onehot", 6, 37)  # K, R: column 5 is zero in every row
PAIR_CASES = ("k3_r257", "k5_r255", "k40_r255", "k2_r1")
DYN_CASE, DYN_LAMDA, DYN_CALLS = "k40_r255", 1.5, 3
HOOK_OUT = dict(n=2, K=4, H=19, W=19, weight=0.1)
HOOK_MID = dict(n_unl=2, C=16, H=11, W=11, subheads=3, clusters=5, weight=0.5, cons_weight=2.0, seed=13)
KINDS = ("scalar", "grad2", "gradmax")


def load(golden_dir):
    return dict(np.load(Path(golden_dir) / "imsat.npz"))


def decode(arr) -> torch.Tensor:
    return torch.from_numpy(np.asarray(arr).astype(np.float32) / 8.0)


def probs(z: torch.Tensor) -> torch.Tensor:
    return torch.softmax(z.float(), 1)


def onehot_rows() -> torch.Tensor:
    _, K, R = ONEHOT
    p = torch.zeros(R, K)
    p[torch.arange(R), (torch.arange(R) * 3) % (K - 1)] = 1.0
    return p


def case_probs(npz, tag) -> torch.Tensor:
    """the f32 probabilities of a row, map or one-hot case ([R,K], or [b,K,H,W] in the case's memory format)"""
    if tag == ONEHOT[0]:
        return onehot_rows()
    p = probs(decode(npz[f"{tag}_z_i8d8"]))
    if tag == "map_nhwc":
        p = p.contiguous(memory_format=torch.channels_last)
    return p


def all_cases():
    return list(ROW_CASES) + list(MAP_CASES) + [ONEHOT[0]]


def entropies64(p: torch.Tensor):
    """(marg, cond) of f64 rows [R,K] or maps [b,K,...] by the formulas of the issue, differentiable"""
    rows = p.movedim(1, -1).reshape(-1, p.shape[1])
    cond = -(rows * torch.log(rows + EPS)).sum(1).mean()
    m = rows.mean(0)
    return -(m * torch.log(m + EPS)).sum(), cond


def rel_vec(a, a64) -> float:
    a64 = torch.as_tensor(a64, dtype=torch.float64).flatten()
    d = torch.as_tensor(a, dtype=torch.float64).flatten() - a64
    return float(d.norm() / a64.norm())


def rel_grad(g, g64):
    """[2-norm, max-norm] distance of g from g64, relative, over all elements"""
    g64 = torch.as_tensor(g64, dtype=torch.float64).flatten()
    d = torch.as_tensor(g, dtype=torch.float64).flatten() - g64
    return [float(d.norm() / g64.norm()), float(d.abs().max() / g64.abs().max())]


def tolerances(npz, mid: bool = False) -> dict:
    """mid: the bounds of the intermediate hook (mid_e_ref alone); otherwise of every other case"""
    worst = np.max(np.stack([v for k, v in npz.items() if k.endswith("e_ref") and (k == "mid_e_ref") == mid]), axis=0)
    return {kind: max(4.0 * float(w), 1e-6) for kind, w in zip(KINDS, worst)}
