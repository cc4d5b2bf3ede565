"""Encoding and layout of tests/golden/multicore_adaptive.npz and multicore_adaptive_gz.npz, shared by their generator
(tests/golden/gen_goldens_adaptive.py) and their readers (tests/test_gpu_multicore_adaptive.py).  The logit gradients
(`_gz64`, 0.9 MB of incompressible f32) are a file of their own so that neither file exceeds the size limit of a
committed file; `load(golden_dir)` reads both as one mapping.  Logits lie on a 1/8 grid
in [-6, 6], translation matrices on a 1/8 grid in [-2, 2]; both are stored as int8 = 8 * value (suffix `_i8d8`, as in
multicore_fixture): exact in f32 and in f64.

Cases `(kind, K, C)`, key `{kind}_k{K}c{C}`; kind is
    adaptive   AdaptiveOverSegmentedLoss(K, C)                      parameter [K, C]
    stricter   StricterAdaptiveOverSegmentedLoss(K, C)              parameter [K - C, C] (empty at K = C)
    mi         StricterAdaptiveOverSegmentedLossWithMI(K, C, mi_weight=MI_WEIGHT)
    member     MultiCoreKL(interleaved_groups(K, C)): no parameter; the kernels take the 0/1 membership matrix as `mix`
Keys per case:
    _z_i8d8 [N,K,H,W]   _t [N,H,W] uint8   _T_i8d8 (the parameter; not for `member`)   _loss64
    _gz64 (f64 gradient w.r.t. the logits, rounded to f32)   _gT64 (w.r.t. the parameter; only where it has elements)
    _argmax [N,H,W] uint8 (reduced arg-max)
    _e_ref = the reference's f32-to-f64 distances [gz 2-norm, gz max, gT 2-norm, gT max, loss], relative (nan: no gT)
Class C - 1 is absent from the labels of image 0 (it is relabelled 0 there).
The large case BIG stores no inputs -- `big_inputs()` draws them from a fixed numpy RandomState stream -- and its logit
gradient only at the 512 pixels BIG_ROWS; the test compares every pixel with an f64 evaluation of the formulas.
"""
import numpy as np
import torch

from multicore_fixture import MARGIN, SHAPE, decode, pixel_rows  # noqa: F401  (re-exported)

FILES = ("multicore_adaptive.npz", "multicore_adaptive_gz.npz")

MI_WEIGHT = 0.1
CASES = (("adaptive", 4, 4), ("adaptive", 15, 3), ("adaptive", 16, 4), ("adaptive", 20, 4), ("adaptive", 21, 3),
         ("adaptive", 32, 4), ("adaptive", 34, 2), ("adaptive", 40, 5), ("adaptive", 64, 16),
         ("stricter", 4, 4), ("stricter", 16, 4), ("stricter", 32, 4), ("stricter", 40, 5),
         ("mi", 32, 4),
         ("member", 32, 4))
BIG = ("adaptive", 32, 4, (2, 96, 96))  # 18 432 pixels = 1152 rows of 16 > the 1024-block cap
BIG_KEY = "adaptive_big"
BIG_SEED = 20260  # (a seed whose draw has no near tie: the least relative gap is 6.6e-5; the generator asserts it)


def _big_rows():
    n = BIG[3][0] * BIG[3][1] * BIG[3][2]
    cut = 1024 * 16  # first pixel of the second grid-stride iteration of the sixteen-lanes-per-pixel kernels
    return np.concatenate([np.arange(0, 128), np.arange(cut - 128, cut + 128), np.arange(n - 128, n)])


BIG_ROWS = _big_rows()
E_GZ, E_GT, E_LOSS = slice(0, 2), slice(2, 4), 4  # where the three kinds sit in `_e_ref`


def load(golden_dir) -> dict:
    out = {}
    for name in FILES:
        with np.load(golden_dir / name) as data:
            out.update({k: data[k] for k in data.files})
    return out


def tag(kind: str, K: int, C: int) -> str:
    return f"{kind}_k{K}c{C}"


def interleaved_groups(K: int, C: int):
    """class c owns the prototypes c, c + C, c + 2C, ..."""
    return [list(range(c, K, C)) for c in range(C)]


def membership(K: int, C: int) -> torch.Tensor:
    """[K, C] 0/1 matrix of interleaved_groups"""
    M = torch.zeros(K, C)
    for c, g in enumerate(interleaved_groups(K, C)):
        M[g, c] = 1.0
    return M


def param_shape(kind: str, K: int, C: int):
    return {"adaptive": (K, C), "stricter": (K - C, C), "mi": (K - C, C), "member": None}[kind]


def drop_last_class_in_image0(t: np.ndarray, C: int) -> np.ndarray:
    t = t.copy()
    t[0][t[0] == C - 1] = 0
    return t


def big_inputs():
    """(int8 logits * 8 [N,K,H,W], labels uint8 [N,H,W], int8 parameter * 8 [K,C]) of the large case"""
    _, K, C, (N, H, W) = BIG
    rs = np.random.RandomState(BIG_SEED)
    z = rs.randint(-48, 49, size=(N, K, H, W)).astype(np.int8)
    t = drop_last_class_in_image0(rs.randint(0, C, size=(N, H, W)).astype(np.uint8), C)
    T = rs.randint(-16, 17, size=(K, C)).astype(np.int8)
    return z, t, T


def mix_of(kind: str, K: int, C: int, T: torch.Tensor = None) -> torch.Tensor:
    """the [K, C] matrix the criterion mixes with, from its parameter T, in T's dtype"""
    if kind == "member":
        return membership(K, C)
    if kind == "adaptive":
        return T.softmax(1)
    return torch.cat([30 * torch.eye(C, dtype=T.dtype), T], dim=0).softmax(1)
