"""Layout and decoding of tests/golden/patch_losses.npz (written by tests/golden/gen_goldens_patch_losses.py): the
reference's `IIDSegmentationSmallPathLoss` / `patch_generator` (contrastyou/losses/discreteMI.py:173-198,264-272),
`PUILoss` / `PUISegLoss` (contrastyou/losses/pica_loss.py) and `JSD_div` / `EntropyPrior` (contrastyou/losses/kl.py:63-78,
142-174), evaluated on the CPU in f32 and in f64.

Inputs are stored as int8 logits on a 1/8 grid (`*_i8d8`), exact in f32: `decode` rebuilds them, `probs` takes the f32
softmax over dim 1, and the f64 runs read those f32 probabilities cast up, so both precisions (and the kernels) read the
same numbers.

Per case `<tag>`:
    <tag>_z<i>_i8d8         the logits of input i (1-based); `A-mask_mask` the 0/1 mask [n,1,H,W] (its maps are A's)
    <tag>_loss64            the f64 value (JSD "none": the f64 map, rounded to f32)
    <tag>_g<i>_64           d loss / d input i in f64, rounded to f32 (JSD "none": of sum(out * none_weights(out)))
    <tag>_e_ref             the reference's own f32-to-f64 distances [value, gradient 2-norm, gradient max-norm]
    prior_given_prior       the prior row [1,C] of the EntropyPrior case with a given prior (f32 probabilities)
    origins_<L>_<p>_<s>     the origins of the reference's patch_generator along an axis, read off its views

Distances are relative: values |d|_2 / |v64|_2 (a scalar is a vector of one), gradients 2-norm and max-norm over all
elements relative to the f64 gradient's.  The tolerance of a kind is max(4 * the largest stored e_ref of that kind, 1e-6)
(`tolerances`), read from the npz, never from the code under test.
"""
from pathlib import Path

import numpy as np
import torch

LAMDA = 1.5  # every patch case
KINDS = ("scalar", "grad2", "gradmax")

# (n, k, H, W, patch, pad)
PATCH_CASES = {
    "A": (2, 5, 24, 20, 16, 1),   # k % 4 != 0; 4 patches with uneven overlap (origins h {0,8}, w {0,4})
    "B": (2, 4, 24, 20, 16, 2),   # vector branches; T*T = 25: three displacement groups, the last of 7
    "C": (2, 8, 24, 20, 16, 0),   # the padding-0 mode
    "D": (1, 3, 12, 10, 16, 1),   # map smaller than the patch: one clipped patch = IIDSegmentationLoss on the map
    "E": (2, 5, 40, 33, 16, 3),   # 16 patches; w origins {0,8,16,17}: three patches over a pixel on one axis; T*T = 49
    "F": (2, 20, 24, 20, 16, 7),  # the reference's default padding and the hooks' k = 20; T*T = 225
    "G": (2, 5, 24, 40, 32, 2),   # clipped in h only; two patches
}
MASK_CASE, MASK_OF = "A-mask", "A"
ORIGIN_CASES = ((224, 32, 16), (24, 16, 8), (20, 16, 8), (33, 16, 8), (12, 16, 8), (40, 32, 16), (32, 32, 16))

PUISEG_CASES = {"puiseg_p3": ((2, 5, 13, 11), 3), "puiseg_p1": ((2, 5, 13, 11), 1)}  # shape, padding; lamda 2.0
PUI_CASES = {"pui_37x6": (37, 6), "pui_257x20": (257, 20)}
PUI_LAMDA = 2.0
# (number of maps, shape, reduction)
JSD_CASES = {f"jsd{m}_{red}": (m, (2, 5, 13, 11), red) for m in (2, 3) for red in ("mean", "sum", "none")}
JSD_CASES["jsd_rows"] = (2, (255, 40), "mean")
PRIOR_CASES = {"prior_default": ((37, 6), False), "prior_given": ((37, 6), True)}
EPS = 1e-16  # JSD_div, EntropyPrior


def load(golden_dir):
    return dict(np.load(Path(golden_dir) / "patch_losses.npz"))


def decode(arr) -> torch.Tensor:
    return torch.from_numpy(np.asarray(arr).astype(np.float32) / 8.0)


def probs(z: torch.Tensor) -> torch.Tensor:
    return torch.softmax(z.float(), 1)


def inputs(npz, tag, count=2):
    """the f32 probabilities of a case's inputs (CPU, contiguous)"""
    tag = MASK_OF if tag == MASK_CASE else tag
    return [probs(decode(npz[f"{tag}_z{i}_i8d8"])) for i in range(1, count + 1)]


def none_weights(out: torch.Tensor) -> torch.Tensor:
    """the upstream gradient of an unreduced output: a fixed ramp over its elements"""
    return torch.linspace(-1.0, 1.0, out.numel(), dtype=out.dtype, device=out.device).view_as(out)


def rel_vec(a, a64) -> float:
    a64 = torch.as_tensor(a64, dtype=torch.float64).flatten()
    d = torch.as_tensor(a, dtype=torch.float64).flatten() - a64
    return float(d.norm() / a64.norm())


def rel_grad(g, g64):
    """[2-norm, max-norm] distance of g from g64, relative, over all elements"""
    g64 = torch.as_tensor(g64, dtype=torch.float64).flatten()
    d = torch.as_tensor(g, dtype=torch.float64).flatten() - g64
    return [float(d.norm() / g64.norm()), float(d.abs().max() / g64.abs().max())]


def tolerances(npz) -> dict:
    worst = np.max(np.stack([v for k, v in npz.items() if k.endswith("_e_ref")]), axis=0)
    return {kind: max(4.0 * float(w), 1e-6) for kind, w in zip(KINDS, worst)}
