#!/usr/bin/env python3
"""Generate tests/golden/semi_wide.npz: the REFERENCE's entropy-minimisation, pseudo-label and UA-MT epocher hooks
(`_EntropyEpocherHook`, `_PLEpocherHook`, `_UAMeanTeacherEpocherHook`, soft and `hard_clip`, two epoch ratios) and its
ICT loss `MSELoss(reduction="none")(...).mean()` (semi_seg/hooks/mt.py:301-319) on multi-prototype logits,
K in (17, 20, 40, 63, 64), evaluated on the CPU in f32 and in f64.

    python tests/golden/gen_goldens_semi_wide.py

Needs the reference checkout (see gen_goldens.py); nothing of it is copied into the repository, only numbers.
Layout and encoding: tests/semi_wide_fixture.py; the way the hooks are driven and what is stored per case:
gen_goldens_semi.py, whose helpers this reuses.  Asserted here, on the reference alone:
  every f64 teacher entropy lies at least 1e-4 away from each threshold used (redrawn otherwise);
  the reference's f32 mask and f32 arg-max equal the f64 ones everywhere: no pixel is left out of any comparison;
  every K has a row (other than the all-zero ones) whose maximum is tied between two different lanes of the row
  kernels, in the student and in the mean teacher, and that row is inside the mask;
  every UA-MT case has 0 < count < P.
"""
import sys
import types
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import gen_goldens as gg  # noqa: E402
import gen_goldens_semi as gs  # noqa: E402  (and through it the import stubs the hook modules need)
import semi_wide_fixture as fx  # noqa: E402

OUT = Path(__file__).resolve().parent / "semi_wide.npz"


def make_inputs(gen, K):
    """gen_goldens_semi.make_inputs with the tied row put in before the entropies are looked at"""
    N, H, W = fx.SHAPE
    n, h, w = fx.TIE_PIXEL
    a, b = fx.tie_channels(K)

    def tie(z):  # z: [..., K, H, W] int8; the two channels at 6, every other one at most -1
        row = z[..., :, h, w].clamp(max=-8)
        row[..., a] = row[..., b] = 48
        z[..., :, h, w] = row

    zs, zt = gs.draw(gen, N, K, H, W), gs.draw(gen, fx.TEACHERS, N, K, H, W)
    zt[1:] = (zt[:1] + torch.randint(-6, 7, zt[1:].shape, generator=gen)).clamp(-48, 48).to(torch.int8)
    tie(zs[n])
    zt[1:, n, :, h, w] = zt[0, n, :, h, w]  # the five teachers agree here: their mean keeps the tie
    tie(zt[:, n])
    for _ in range(100):
        ent = gs.entropy64(zt)
        near = torch.zeros_like(ent, dtype=torch.bool)
        for thr in gs.thresholds(K, fx.EPOCHS):
            near |= (ent - thr).abs() < gs.MARGIN
        near[:, :fx.ZERO_ROWS] = False
        assert not near[n, h, w]
        if not near.any():
            break
        zt = torch.where(near[None, :, None], gs.draw(gen, fx.TEACHERS, N, K, H, W), zt)
    else:
        raise RuntimeError("could not move every pixel off the thresholds")
    zs[:, :, :fx.ZERO_ROWS] = 0
    zt[:, :, :, :fx.ZERO_ROWS] = 0
    return zs, zt


def main():
    scratch = gg.setup_reference()
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = type("SummaryWriter", (), {})
    sys.modules["torch.utils.tensorboard"] = tb
    from contrastyou.losses.kl import Entropy
    from semi_seg.hooks.entmin import _EntropyEpocherHook
    from semi_seg.hooks.mt import EMAUpdater, _UAMeanTeacherEpocherHook
    from semi_seg.hooks.pseudolabel import _PLEpocherHook
    gs.MAX_EPOCH = fx.MAX_EPOCH  # (the same number: gs.adopt and gs.thresholds read it)

    out, table = {}, []
    gen = torch.Generator().manual_seed(1720)
    for K in fx.KS:
        zs, zt = make_inputs(gen, K)
        out[f"K{K}_zs_i8d8"], out[f"K{K}_zt_i8d8"] = zs.numpy(), zt.numpy()
    inputs = {K: (fx.decode("zs_i8d8", out[f"K{K}_zs_i8d8"]), fx.decode("zt_i8d8", out[f"K{K}_zt_i8d8"]))
              for K in fx.KS}
    n, h, w = fx.TIE_PIXEL
    for K, (zs, zt) in inputs.items():
        for what, z in (("student", zs), ("mean teacher", zt.double().mean(0))):
            ties = fx.cross_lane_ties(z)
            assert ties[n, h, w] and ties[:, :fx.ZERO_ROWS].all(), (K, what)
            assert int(z[n, :, h, w].argmax()) == fx.tie_channels(K)[0], (K, what)

    # ------------------------------------------------------------------ entropy minimisation, pseudo-label
    for K in fx.KS:
        zs, _ = inputs[K]
        res = gs.run_both(lambda dt: gs.adopt(_EntropyEpocherHook(name="entropy", weight=1.0, criterion=Entropy())), zs)
        gs.store(out, table, f"ent_K{K}", res)
        res = gs.run_both(lambda dt: gs.adopt(_PLEpocherHook(name="plab", weight=1.0, criterion=torch.nn.MSELoss())),
                          zs)
        gs.store(out, table, f"pl_K{K}", res)
        assert torch.equal(zs.float().softmax(1).max(1)[1], zs.double().softmax(1).max(1)[1]), K

    # ------------------------------------------------------------------ UA-MT
    image = torch.zeros(fx.SHAPE[0], 1, *fx.SHAPE[1:])
    P = fx.SHAPE[0] * fx.SHAPE[1] * fx.SHAPE[2]

    def uamt_hook(dt, zt, cur_epoch, hard):
        teacher = fx.StoredTeacher([t.to(dt) for t in zt])
        hook = _UAMeanTeacherEpocherHook(
            name="mt", weight=1.0, criterion=torch.nn.MSELoss(reduction="none"), teacher_model=teacher,
            updater=EMAUpdater(), extra_teachers=torch.nn.ModuleList(), extra_updater=EMAUpdater(update_bn=True),
            hard_clip=hard)
        return gs.adopt(hook, cur_epoch)

    for key, K, ep, hard in fx.uamt_cases():
        zs, zt = inputs[K]
        res = gs.run_both(lambda dt: uamt_hook(dt, zt, ep, hard), zs, unlabeled_image=image, unlabeled_image_tf=image)
        gs.store(out, table, key, res)
        thr = gs.thresholds(K, (ep,))[0]
        seen = {}
        for dt in (torch.float32, torch.float64):
            hook = res[dt][2]
            assert hook._teacher_model.calls == fx.TEACHERS
            prob, ent = hook._aggregate_predictions(unlabeled_image=image.to(dt), N=4, affine_transformer=gs.identity,
                                                    seed=1)
            seen[dt] = (ent < thr, prob.argmax(1))
        assert torch.equal(seen[torch.float32][0], seen[torch.float64][0]), f"{key}: the f32 mask differs"
        assert torch.equal(seen[torch.float32][1], seen[torch.float64][1]), f"{key}: the f32 arg-max differs"
        mask = seen[torch.float64][0]
        assert mask[n, h, w], f"{key}: the tied row is outside the mask"
        assert 0 < int(mask.sum()) < P, (key, int(mask.sum()))
        out[f"{key}_count"] = np.int64(mask.sum())
        out[f"{key}_thr"] = np.float64(thr)

    # ------------------------------------------------------------------ ICT (the f64 run reads the f32 weights cast up)
    mse = torch.nn.MSELoss(reduction="none")
    index = torch.tensor(fx.ICT_INDEX)
    w_self, w_other = np.float32(fx.ICT_LAM), np.float32(1.0 - fx.ICT_LAM)
    for K in fx.KS:
        zs, zt = inputs[K]
        res = {}
        for dt in (torch.float32, torch.float64):
            z = zs.detach().to(dt).clone().requires_grad_(True)
            prob = zt[0].to(dt).softmax(1)
            mixed = float(w_self) * prob + float(w_other) * prob[index, :]
            loss = mse(z.softmax(1), mixed).mean()
            loss.backward()
            res[dt] = (loss.detach(), z.grad, None)
        gs.store(out, table, f"ict_K{K}", res)

    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {OUT.stat().st_size} bytes")
    print("reference f32 vs f64:  case | grad 2-norm | grad max | loss | mask count")
    for name, e in table:
        count = out.get(f"{name}_count", "")
        print(f"  {name:20s} | {e[0]:.2e} | {e[1]:.2e} | {e[2]:.2e} | {count}")
    del scratch


if __name__ == "__main__":
    main()
