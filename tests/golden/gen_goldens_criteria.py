#!/usr/bin/env python3
"""Generate tests/golden/criteria.npz and tests/golden/criteria_dice.npz: the REFERENCE's supervised criteria
`KL_div(weight=..., reduction=...)` (contrastyou/losses/kl.py:81-125) and `DiceLoss` (contrastyou/losses/dice_loss.py:
31-105) on softmax(logits) against one-hot labels, evaluated on the CPU in f32 and in f64 on seeded logits.

    python tests/golden/gen_goldens_criteria.py

Needs the reference checkout (see gen_goldens.py); nothing of it is copied into the repository, only numbers.
Layout and encoding: tests/criteria_fixture.py.  Stored per case: the f64 loss, the f64 gradient with respect to the
logits (rounded to f32) and the reference's own f32-to-f64 distances `e_ref` = [2-norm, element-wise max, loss],
relative as in the tolerance rule of tests/test_gpu_cc.py.  A "none" reduction is differentiated under a stored random
upstream gradient, and its loss figure is the sum of output * upstream.

Images are square.  The reference's weighted KL_div builds its weight map as `weight.expand(b, H, W, c).transpose(-1, 1)`
(kl.py:117), which is [b, c, W, H]: H and W are swapped, and at 17 x 19 the multiplication raises.  The kernels and this
project's `KL_div.forward` take any shape; only the comparison with the reference needs H = W.
The f64 evaluation multiplies by the same f32-rounded normalised weights (kl.py:104-108 keeps them `.float()`).
Image ABSENT_IMAGE has no pixel of class ABSENT_CLASS (T = 0 in its Dice denominator).
No pixel is left out of any comparison: these losses have no arg-max and no threshold, so there are no ties.
"""
import sys
import types
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import gen_goldens as gg  # noqa: E402
import gen_goldens_cc  # noqa: E402,F401  (its loguru stub)
from criteria_fixture import (ABSENT_CLASS, ABSENT_IMAGE, FILES, KS, SHAPE, decode, dice_cases, kl_cases,  # noqa: E402
                              kl_weight)
from gen_goldens_semi import draw, f32, rel  # noqa: E402

HERE = Path(__file__).resolve().parent


def make_labels(gen, z, K):
    """half the pixels carry the arg-max of their logits, half a random class; image ABSENT_IMAGE never ABSENT_CLASS"""
    N, H, W = SHAPE
    y = torch.where(torch.rand(N, H, W, generator=gen) < 0.5, z.argmax(1), torch.randint(0, K, (N, H, W), generator=gen))
    other = (ABSENT_CLASS + 1 + torch.randint(0, K - 1, (H, W), generator=gen)) % K  # any class but the absent one
    y[ABSENT_IMAGE] = torch.where(y[ABSENT_IMAGE] == ABSENT_CLASS, other, y[ABSENT_IMAGE])
    for n in range(N):
        present = set(y[n].unique().tolist())
        want = set(range(K)) - ({ABSENT_CLASS} if n == ABSENT_IMAGE else set())
        assert present == want, (K, n, sorted(want - present))
    return y


def run_both(make_crit, z, y, K, up):
    """-> {dtype: (figure, dfigure/dz, output)}; figure = the loss, or sum(output * up) for a "none" reduction"""
    res = {}
    for dt in (torch.float32, torch.float64):
        zz = z.detach().to(dt).clone().requires_grad_(True)
        onehot = torch.nn.functional.one_hot(y, K).movedim(-1, 1).to(dt)
        out = make_crit()(zz.softmax(1), onehot)
        fig = out if out.dim() == 0 else (out * up.to(dt)).sum()
        fig.backward()
        res[dt] = (fig.detach(), zz.grad, out.detach())
    return res


def store(out, table, key, res):
    (l32, g32, _), (l64, g64, o64) = res[torch.float32], res[torch.float64]
    e = rel(g32, g64) + [float(abs(l32.double() - l64) / abs(l64))]
    out[f"{key}_loss64"], out[f"{key}_g64"], out[f"{key}_e_ref"] = np.float64(l64), f32(g64), np.array(e)
    if o64.dim():
        out[f"{key}_out64"] = o64.numpy()
    table.append((key, e))


def main():
    scratch = gg.setup_reference()
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = type("SummaryWriter", (), {})
    sys.modules["torch.utils.tensorboard"] = tb
    from contrastyou.losses.dice_loss import DiceLoss
    from contrastyou.losses.kl import KL_div

    N, H, W = SHAPE
    assert H == W, "the reference's weighted KL_div swaps H and W (see the docstring)"
    kl, dice, table = {}, {}, []
    gen = torch.Generator().manual_seed(1901)
    inputs = {}
    for K in KS:
        zq = draw(gen, N, K, H, W)
        kl[f"K{K}_z_i8d8"] = zq.numpy()
        z = decode("z_i8d8", kl[f"K{K}_z_i8d8"])
        y = make_labels(gen, z, K)
        upmap = (torch.rand(N, H, W, generator=gen) + 0.5).float()
        upvec = (torch.rand(N, generator=gen) + 0.5).float()
        kl[f"K{K}_y"], kl[f"K{K}_upmap"], kl[f"K{K}_upvec"] = y.numpy().astype(np.uint8), upmap.numpy(), upvec.numpy()
        inputs[K] = (z, y, upmap, upvec)

    for key, K, tag, red in kl_cases():
        z, y, upmap, _ = inputs[K]
        store(kl, table, key, run_both(lambda: KL_div(reduction=red, weight=kl_weight(K, tag)), z, y, K, upmap))
    for key, K, kw in dice_cases():
        z, y, _, upvec = inputs[K]
        store(dice, table, key, run_both(lambda: DiceLoss(**kw), z, y, K, upvec))

    for name, data in (("kl", kl), ("dice", dice)):
        path = HERE / FILES[name]
        np.savez_compressed(path, **data)
        print(f"{path}: {path.stat().st_size} bytes")
        assert path.stat().st_size < 1 << 20, "a committed file must stay under 1 MiB"
    print("reference f32 vs f64:  case | grad 2-norm | grad max | loss")
    for name, e in table:
        print(f"  {name:22s} | {e[0]:.2e} | {e[1]:.2e} | {e[2]:.2e}")
    for kind in ("kl", "dice"):
        rows = np.array([e for name, e in table if name.startswith(kind)])
        print(f"largest over the {kind} cases: {rows.max(0)}")
    del scratch


if __name__ == "__main__":
    main()
