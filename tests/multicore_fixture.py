"""Encoding and layout of tests/golden/multicore.npz, shared by its generator (tests/golden/gen_goldens_multicore.py)
and its readers (tests/test_gpu_multicore.py).  Logits lie on a 1/8 grid in [-6, 6] and are stored as int8 = 8 * logit
(suffix `_i8d8`, as in semi_fixture): exact in f32 and in f64.

Keys, per multi-prototype case `kl_c{C}m{m}` (C true classes, m prototypes each, K = C * m logits):
    _z_i8d8 [N,K,H,W]   _t [N,H,W] uint8   _loss64   _g64 (f64 gradient rounded to f32)   _argmax [N,H,W] uint8
    _e_ref = the reference's f32-to-f64 distances [gradient 2-norm, gradient max, loss], relative
The large case `kl_big` (BIG) stores no inputs -- `big_inputs()` draws them from a fixed numpy RandomState stream, whose
values are guaranteed stable -- and its gradient only at the pixels BIG_ROWS (the whole gradient would be 2.4 MB);
the test compares every pixel with an f64 evaluation of the formula and these rows with the reference.
Per consistency case `cons_K{K}`: _a_i8d8, _b_i8d8 [N,K,H,W] (plain view warped, transformed view), _loss64,
_g64 (gradient with respect to b), _e_ref.
"""
import numpy as np
import torch

CASES = ((4, 1), (3, 5), (4, 4), (5, 4), (3, 7), (2, 17), (4, 8), (8, 8))  # (C, m)
SHAPE = (2, 13, 22)          # N, H, W: 572 pixels, no multiple of 256, 16 or 4
BIG = (4, 8, (2, 96, 96))    # C, m, (N, H, W): 18 432 pixels = 1152 rows of 16 > the 1024-block cap
BIG_SEED = 20241
CONS_KS = (20, 21, 32, 64)
CONS_SHAPE = (2, 13, 11)     # 286 pixels
MARGIN = 1e-5                # least relative gap between the two largest reduced probabilities of a pixel


def _big_rows():
    n = BIG[2][0] * BIG[2][1] * BIG[2][2]
    cut = 1024 * 16  # first pixel of the second grid-stride iteration
    return np.concatenate([np.arange(0, 256), np.arange(cut - 256, cut + 256), np.arange(n - 256, n)])


BIG_ROWS = _big_rows()


def tag(C: int, m: int) -> str:
    return f"kl_c{C}m{m}"


def groups_of(C: int, m: int):
    """the contiguous equal partition of range(C * m): class c owns [c*m, (c+1)*m)"""
    return [list(range(c * m, (c + 1) * m)) for c in range(C)]


def decode(name: str, arr: np.ndarray) -> torch.Tensor:
    assert name.endswith("_i8d8"), name
    return torch.from_numpy(np.asarray(arr)).float() / 8.0


def big_inputs():
    """(int8 logits * 8 [N,K,H,W], labels uint8 [N,H,W]) of the large case"""
    C, m, (N, H, W) = BIG
    rs = np.random.RandomState(BIG_SEED)
    z = rs.randint(-48, 49, size=(N, C * m, H, W)).astype(np.int8)
    t = rs.randint(0, C, size=(N, H, W)).astype(np.uint8)
    return z, t


def pixel_rows(g: torch.Tensor, rows) -> torch.Tensor:
    """[N,K,H,W] -> [len(rows), K]: the gradient at the pixels `rows` (index n*H*W + h*W + w)"""
    K = g.shape[1]
    return g.permute(0, 2, 3, 1).reshape(-1, K)[torch.as_tensor(rows)]
