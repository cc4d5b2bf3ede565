#!/usr/bin/env python3
"""Generate tests/golden/mixup.npz: the REFERENCE's `mixup_data` draws (semi_seg/hooks/utils.py:284-297), its MixUp loss
`KL_div()(softmax, mixed one-hot)` (semi_seg/hooks/mixup.py:49-58) and ICT loss `MSELoss(reduction="none")(...).mean()`
(semi_seg/hooks/mt.py:301-319) with their input gradients, and the `_call_implementation` of `_MixUpEpocherHook` and
`_ICTMeanTeacherEpocherHook`, evaluated on the CPU in f32 and in f64; and tests/golden/mixup_signatures.txt: parameter
names of `mixup_data`, both trainer hooks, `MixupEpocher._batch_update` and the constructor `MixUpTrainer` inherits.

    python tests/golden/gen_goldens_mixup.py

Needs the reference checkout (see gen_goldens.py); nothing of it is copied into the repository, only numbers and names.
Layout, decoding and the way distances are measured: tests/mixup_fixture.py; the cases: tests/mixup_cases.py.

The draws are what the reference's `mixup_data` does to the generators under its `fix_all_seed_within_context`: it is
called on a [batch, 1] tensor whose rows are their own numbers, so that lam and the index can be read off the result.
The losses are the reference's criteria on a mixed target formed in f32 by `mixup_data`'s expression with the recorded
weights; the f64 runs read that f32 target (MixUp) or the f32 weights (ICT) cast up, so both precisions and the kernels
read the same numbers.  The hooks run as they are, on a stand-in model (mixup_fixture.Conv1x1) and recording meters.
"""
import sys
import types
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import gen_goldens as gg  # noqa: E402
import gen_goldens_cc  # noqa: E402,F401  (the import stubs the hook modules need)
from gen_goldens_imsat import Rec, arg_names, f32, leaf  # noqa: E402
import mixup_cases as mc  # noqa: E402
import mixup_fixture as fx  # noqa: E402

OUT = Path(__file__).resolve().parent / "mixup.npz"
NAMES = Path(__file__).resolve().parent / "mixup_signatures.txt"


def image_i8(gen, *shape):
    return (torch.rand(*shape, generator=gen) * 8).round().to(torch.int8)  # [0, 1] on the 1/8 grid


def main():
    scratch = gg.setup_reference()
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = type("SummaryWriter", (), {})
    sys.modules["torch.utils.tensorboard"] = tb
    from contrastyou.losses.kl import KL_div
    from contrastyou.utils import class2one_hot, fix_all_seed_within_context
    from semi_seg.hooks import mixup as ref_mixup
    from semi_seg.hooks import mt as ref_mt
    from semi_seg.hooks.utils import mixup_data

    ref = scratch / "ref"
    ut, mx, mt = "semi_seg/hooks/utils.py", "semi_seg/hooks/mixup.py", "semi_seg/hooks/mt.py"
    ep, tr = "semi_seg/epochers/comparable.py", "semi_seg/trainers/trainer.py"
    lines = [f"{name}: " + " ".join(arg_names(ref / path, cls, fn)) for name, path, cls, fn in (
        ("mixup_data", ut, None, "mixup_data"),
        ("MixUpTrainHook", mx, "MixUpTrainHook", "__init__"),
        ("ICTMeanTeacherTrainerHook", mt, "ICTMeanTeacherTrainerHook", "__init__"),
        ("MixupEpocher._batch_update", ep, "MixupEpocher", "_batch_update"),
        ("MixUpTrainer", tr, "SemiTrainer", "__init__"))]  # MixUpTrainer defines none: it inherits SemiTrainer's
    NAMES.write_text("\n".join(lines) + "\n")

    out, table = {}, []
    # ---- draws
    lam = np.zeros((len(mc.SEEDS), len(mc.BATCHES), len(mc.ALPHAS)))
    for bi, batch in enumerate(mc.BATCHES):
        idx = np.zeros((len(mc.SEEDS), len(mc.ALPHAS), batch), dtype=np.int64)
        for si, seed in enumerate(mc.SEEDS):
            for ai, alpha in enumerate(mc.ALPHAS):
                # rows 2^n: mixed_x[n] = lam 2^n + (1 - lam) 2^index[n]
                rows = (2.0 ** torch.arange(batch, dtype=torch.float64)).unsqueeze(1)
                with fix_all_seed_within_context(seed):
                    state = np.random.get_state()
                    mixed, _ = mixup_data(rows, rows, alpha=alpha, device="cpu")
                    np.random.set_state(state)
                    lam[si, bi, ai] = np.random.beta(alpha, alpha)  # the very draw mixup_data made
                l_ = lam[si, bi, ai]
                got = ((mixed.squeeze(1) - l_ * rows.squeeze(1)) / (1 - l_)).log2().round().long()
                assert torch.allclose(l_ * rows + (1 - l_) * rows[got], mixed, rtol=1e-12, atol=0), (seed, batch, alpha)
                assert sorted(got.tolist()) == list(range(batch))
                idx[si, ai] = got.numpy()
        out[f"draw_index_b{batch}"] = idx
    out["draw_lam"] = lam

    # ---- the two losses
    kl, mse = KL_div(), torch.nn.MSELoss(reduction="none")
    for case in mc.LOSS_CASES:
        if not case.golden:
            continue
        tag = case.tag
        out[f"{tag}_s_i8d8"], out[f"{tag}_t_i8d8"] = mc.logits_i8(case, "s"), mc.logits_i8(case, "t")
        small = np.int8 if case.K < 128 else np.int64
        out[f"{tag}_y"] = mc.labels(case).astype(small)
        s, t, y, index, (w_self, w_other) = fx.case_inputs(out, case)
        onehot = class2one_hot(y, C=case.K).float()
        target32 = w_self * onehot + w_other * onehot[index, :]  # mixup_data's expression, f32
        res = {}
        for dt in (torch.float32, torch.float64):
            z = leaf(s, dt)
            v = kl(z.softmax(1), target32.to(dt))
            v.backward()
            zs = leaf(s, dt)
            prob = t.to(dt).softmax(1)
            mixed = fx.f32w(w_self) * prob + fx.f32w(w_other) * prob[index, :]
            u = mse(zs.softmax(1), mixed).mean()
            u.backward()
            res[dt] = (v.detach(), z.grad, u.detach(), zs.grad)
        (v32, g32, u32, h32), (v64, g64, u64, h64) = res[torch.float32], res[torch.float64]
        out[f"{tag}_kl64"], out[f"{tag}_mse64"] = np.float64(v64), np.float64(u64)
        out[f"{tag}_gkl64"], out[f"{tag}_gmse64"] = f32(g64), f32(h64)
        e_kl = [fx.rel_scalar(v32, v64)] + fx.rel_grad(g32, g64)
        e_mse = [fx.rel_scalar(u32, u64)] + fx.rel_grad(h32, h64)
        out[f"{tag}_kl_e_ref"], out[f"{tag}_mse_e_ref"] = np.array(e_kl), np.array(e_mse)
        table += [(f"{tag} kl", e_kl), (f"{tag} mse", e_mse)]

    gen = torch.Generator().manual_seed(2207)
    # ---- _MixUpEpocherHook
    h = mc.HOOK_MIXUP
    B, K = h["B"], h["K"]
    out["mixup_image_i8d8"] = image_i8(gen, B, 1, h["H"], h["W"]).numpy()
    out["mixup_image_tf_i8d8"] = image_i8(gen, B, 1, h["H"], h["W"]).numpy()
    out["mixup_y"] = torch.randint(0, K, (B, 1, h["H"], h["W"]), generator=gen).to(torch.int8).numpy()
    out["mixup_y_tf"] = torch.randint(0, K, (B, 1, h["H"], h["W"]), generator=gen).to(torch.int8).numpy()
    out["mixup_w"] = (torch.randn(K, generator=gen) * 2).numpy()
    out["mixup_b"] = torch.randn(K, generator=gen).numpy()
    res = {}
    for dt in (torch.float32, torch.float64):
        model = fx.Conv1x1(out["mixup_w"], out["mixup_b"], dt)
        hook = ref_mixup._MixUpEpocherHook(name="mix_reg", weight=h["weight"], criterion=KL_div(), enable_bn=True)
        hook._epocher = types.SimpleNamespace(_model=model, device="cpu", num_classes=K)
        hook._epocher_init = True
        hook.meters = {"loss": Rec()}
        value = hook._call_implementation(
            labeled_image=fx.decode(out["mixup_image_i8d8"]).to(dt),
            labeled_image_tf=fx.decode(out["mixup_image_tf_i8d8"]).to(dt),
            labeled_target=torch.from_numpy(out["mixup_y"]).long(),
            labeled_target_tf=torch.from_numpy(out["mixup_y_tf"]).to(dt), seed=h["seed"])
        value.backward()
        res[dt] = (value.detach(), torch.cat([model.w.grad.flatten(), model.b.grad.flatten()]), hook.meters["loss"].got)
    (v32, g32, _), (v64, g64, got) = res[torch.float32], res[torch.float64]
    out["mixup_value64"], out["mixup_g64"], out["mixup_meter64"] = np.float64(v64), g64.numpy(), np.array(got)
    e = [fx.rel_scalar(v32, v64)] + fx.rel_grad(g32, g64)
    out["mixup_e_ref"] = np.array(e)
    table.append(("mixup hook", e))

    # ---- _ICTMeanTeacherEpocherHook
    h = mc.HOOK_ICT
    B, K = h["B"], h["K"]
    out["ict_image_i8d8"] = image_i8(gen, B, 1, h["H"], h["W"]).numpy()
    out["ict_image_tf_i8d8"] = image_i8(gen, B, 1, h["H"], h["W"]).numpy()
    out["ict_w"], out["ict_b"] = (torch.randn(K, generator=gen) * 2).numpy(), torch.randn(K, generator=gen).numpy()
    out["ict_tw"], out["ict_tb"] = (torch.randn(K, generator=gen) * 2).numpy(), torch.randn(K, generator=gen).numpy()
    res = {}
    for dt in (torch.float32, torch.float64):
        model = fx.Conv1x1(out["ict_w"], out["ict_b"], dt)
        teacher = fx.Conv1x1(out["ict_tw"], out["ict_tb"], dt)
        hook = ref_mt._ICTMeanTeacherEpocherHook(
            name="ict", weight=h["weight"], criterion=torch.nn.MSELoss(reduction="none"), teacher_model=teacher,
            updater=ref_mt.EMAUpdater(), extra_teachers=torch.nn.ModuleList(),
            extra_updater=ref_mt.EMAUpdater(update_bn=True))
        hook._epocher = types.SimpleNamespace(_model=model)
        hook._epocher_init = True
        hook.meters = {"loss": Rec()}
        image = fx.decode(out["ict_image_i8d8"]).to(dt)
        image_tf = fx.decode(out["ict_image_tf_i8d8"]).to(dt)
        value = hook._call_implementation(unlabeled_tf_logits=None, unlabeled_image=image, unlabeled_image_tf=image_tf,
                                          seed=h["seed"])
        value.backward()
        res[dt] = (value.detach(), torch.cat([model.w.grad.flatten(), model.b.grad.flatten()]), hook.meters["loss"].got)
    (v32, g32, _), (v64, g64, got) = res[torch.float32], res[torch.float64]
    out["ict_value64"], out["ict_g64"], out["ict_meter64"] = np.float64(v64), g64.numpy(), np.array(got)
    e = [fx.rel_scalar(v32, v64)] + fx.rel_grad(g32, g64)
    out["ict_e_ref"] = np.array(e)
    table.append(("ict hook", e))

    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {OUT.stat().st_size} bytes; {NAMES}:\n{NAMES.read_text()}")
    print("reference f32 vs f64:  case | scalar | gradient 2-norm | gradient max-norm")
    for name, e in table:
        print(f"  {name:22s} | {e[0]:.2e} | {e[1]:.2e} | {e[2]:.2e}")
    print("tolerances", {k: f"{v:.2e}" for k, v in fx.tolerances(out).items()})
    del scratch


if __name__ == "__main__":
    main()
