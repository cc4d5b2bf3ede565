#!/usr/bin/env python3
"""Generate tests/golden/selfpaced.npz: the REFERENCE's SelfPacedSupConLoss (contrastyou/losses/contrastive.py:103-212)
evaluated on the CPU in f32 and in f64.

    python tests/golden/gen_goldens_selfpaced.py

Needs the reference checkout (see gen_goldens.py); nothing of it is copied into the repository, only numbers.

Inputs: z1, z2 (70 x 16 random unit rows) and the asymmetric masks b and d of tests/golden/supcon_masks.npz (d holds
pairs that are neither positive nor negative); positives = labels i % 3, mask b, mask d; hard and soft weights;
correct_grad off and on.  gamma per (positives, mode) by the rules of tests/selfpaced_cases.py for random rows -- hard:
the midpoint of the widest gap of the float64 positive-pair losses between their 25th and 75th percentile (asserted to
leave HARD_MARGIN on either side), soft: their median (asserted to put pairs on both branches of the clamp).

Per case `<positives>_<mode>_c<correct_grad>`: `_gamma`, `_loss` and `_ratio` of the f64 run (f64), `_dz1` / `_dz2` of
the f64 run under an upstream gradient of GSCALE (rounded to f32: 6e-8 of their size), `_loss32` / `_ratio32` of the f32
run.  The distance |ratio32 - ratio| is printed: tests/selfpaced_cases.py records it as the ratio's yardstick.
The archive is written with fixed member dates: running this again reproduces the committed file byte for byte.
"""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import gen_goldens as gg  # noqa: E402
from gen_goldens_supcon import write_npz  # noqa: E402
from tests import selfpaced_cases as sc  # noqa: E402

HERE = Path(__file__).resolve().parent
OUT = HERE / sc.GOLDEN_FILE


def main():
    src = np.load(HERE / sc.GOLDEN_INPUTS)
    z1, z2 = torch.from_numpy(src["z1"]), torch.from_numpy(src["z2"])
    assert z1.shape == (sc.GOLDEN_N, sc.GOLDEN_D) and z1.dtype == torch.float32 and float(src["t"]) == sc.T
    scratch = gg.setup_reference()
    from contrastyou.losses.contrastive import SelfPacedSupConLoss

    out, dist = {}, {}
    rand = sc.Problem("golden", sc.GOLDEN_N, sc.GOLDEN_D, "", "rand", 0)   # (the gamma rule of random rows)
    for positives in sc.GOLDEN_POSITIVES:
        target = None if positives != "mod3" else [i % 3 for i in range(sc.GOLDEN_N)]
        mask = None if positives == "mod3" else torch.from_numpy(src[f"{positives}_mask"])
        l = sc.positive_losses(z1, z2, target, mask)
        for mode in sc.MODES:
            gamma = sc.gamma_of(rand, mode, l)
            if mode == "hard":
                assert float((l - gamma).abs().min()) >= sc.HARD_MARGIN, (positives, float((l - gamma).abs().min()))
            else:
                assert bool((l > gamma).any()) and bool((l < gamma).any())
            for cg in (0, 1):
                tag = f"{positives}_{mode}_c{cg}"
                res = {}
                for dt in (torch.float32, torch.float64):
                    a, b = z1.to(dt).clone().requires_grad_(True), z2.to(dt).clone().requires_grad_(True)
                    crit = SelfPacedSupConLoss(temperature=sc.T, weight_update=mode, correct_grad=bool(cg))
                    crit.set_gamma(gamma)
                    loss = crit(a, b, target=target, mask=mask)
                    (loss * sc.GSCALE).backward()
                    res[dt] = (loss.item(), crit.downgrade_ratio, a.grad, b.grad)
                l64, r64, da, db = res[torch.float64]
                l32, r32, _, _ = res[torch.float32]
                out[f"{tag}_gamma"] = np.float64(gamma)
                out[f"{tag}_loss"], out[f"{tag}_ratio"] = np.float64(l64), np.float64(r64)
                out[f"{tag}_loss32"], out[f"{tag}_ratio32"] = np.float64(l32), np.float64(r32)
                out[f"{tag}_dz1"], out[f"{tag}_dz2"] = da.numpy().astype(np.float32), db.numpy().astype(np.float32)
                dist[tag] = abs(r32 - r64)
    write_npz(OUT, out)
    print(f"{OUT}: {OUT.stat().st_size} bytes")
    print("RATIO_F32_F64 = {")
    for tag in sc.GOLDEN_TAGS:
        print(f"    \"{tag}\": {dist[tag]:.1e},   # gamma {float(out[tag + '_gamma']):.6f}  loss {float(out[tag + '_loss']):.6f}"
              f"  ratio {float(out[tag + '_ratio']):.6f}")
    print("}")
    del scratch


if __name__ == "__main__":
    main()
