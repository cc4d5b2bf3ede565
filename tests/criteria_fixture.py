"""Layout and decoding of tests/golden/criteria.npz (inputs and the weighted-KL cases) and
tests/golden/criteria_dice.npz (the Dice cases: one file of both would pass the size limit of a committed file),
shared by their generator (tests/golden/gen_goldens_criteria.py) and their reader (tests/test_gpu_criteria.py).
Logits lie on a 1/8 grid in [-6, 6] and are stored as int8 = 8 * logit (suffix `_i8d8`, as in semi_fixture): exact in
f32 and in f64.  Labels are stored as uint8; upstream gradients as f32.

Per class count K: `K{K}_z_i8d8` [N, K, H, W], `K{K}_y` [N, H, W], `K{K}_upmap` [N, H, W] and `K{K}_upvec` [N] (the
upstream gradients of the "none" reductions).  Image ABSENT_IMAGE holds no pixel of class ABSENT_CLASS.
Per case `key`: `{key}_loss64` the reference's f64 loss (for a "none" reduction the f64 sum of output * upstream, and
`{key}_out64` the output itself), `{key}_g64` its f64 gradient with respect to the logits rounded to f32, and
`{key}_e_ref` = the reference's own f32-to-f64 distances [gradient 2-norm, gradient element-wise max, loss], relative.
"""
import numpy as np
import torch

KS = (2, 4, 5, 16)          # class counts of the fixture
SHAPE = (3, 19, 19)         # N, H, W: 361 pixels per image = one full block of 256 plus a tail; square (see the generator)
ABSENT_IMAGE, ABSENT_CLASS = 2, 1
REDUCTIONS = ("mean", "sum", "none")
FILES = {"kl": "criteria.npz", "dice": "criteria_dice.npz"}


def decode(name: str, arr: np.ndarray) -> torch.Tensor:
    assert name.endswith("_i8d8"), name
    return torch.from_numpy(np.asarray(arr)).float() / 8.0


def kl_weight(K: int, tag: str):
    """the weight list handed to KL_div: "ramp" [1, 2, ..., K]; "zero": the ramp with entry K // 2 set to 0"""
    w = [float(k + 1) for k in range(K)]
    if tag == "zero":
        w[K // 2] = 0.0
    return w


def kl_cases():
    """(key, K, weight tag, reduction) of every weighted-KL case"""
    return [(f"kl_K{K}_{tag}_{red}", K, tag, red) for K in KS for tag in ("ramp", "zero") for red in REDUCTIONS]


def dice_cases():
    """(key, K, DiceLoss keywords) of every Dice case: the three reductions, then one case each of ignore_index 0,
    ignore_index K - 1, p = 1 and smooth = 1e-5 at the mean reduction"""
    out = []
    for K in KS:
        out += [(f"dice_K{K}_{red}", K, dict(reduction=red)) for red in REDUCTIONS]
        out += [(f"dice_K{K}_ign0", K, dict(ignore_index=0)), (f"dice_K{K}_ignL", K, dict(ignore_index=K - 1)),
                (f"dice_K{K}_p1", K, dict(p=1)), (f"dice_K{K}_smooth", K, dict(smooth=1e-5))]
    return out
