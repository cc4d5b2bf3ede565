#!/usr/bin/env python3
"""Generate tests/golden/semi_baselines.npz: the REFERENCE's entropy-minimisation, pseudo-label and UA-MT epocher hooks
(`_EntropyEpocherHook`, `_PLEpocherHook`, `_UAMeanTeacherEpocherHook`), their `_call_implementation` evaluated on the
CPU in f32 and in f64 on seeded logits, and tests/golden/hook_factory_names.txt: the factory names the reference's
hook_creator.py imports from semi_seg.hooks.

    python tests/golden/gen_goldens_semi.py

Needs the reference checkout (see gen_goldens.py); nothing of it is copied into the repository, only numbers and names.
Layout and encoding: tests/semi_fixture.py.  The UA-MT teacher is a module that returns five stored logit tensors.
Stored per case: the f64 loss, the f64 gradient with respect to the student logits (rounded to f32), for UA-MT the
integer mask count, and the reference's own f32-to-f64 distances `e_ref` = [2-norm, element-wise max, loss], relative
as in the tolerance rule of tests/test_gpu_cc.py.
No pixel is ever left out of a comparison: a pixel whose f64 teacher entropy lies within 1e-4 of a threshold of its
cases is redrawn, and the reference's f32 mask and f32 arg-max are asserted to equal their f64 counterparts everywhere.
"""
import ast
import collections
import math
import sys
import types
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import gen_goldens as gg  # noqa: E402
import gen_goldens_cc  # noqa: E402,F401  (its loguru stub: `logger.contextualize` decorates mt.py:251)
from semi_fixture import (EPOCHS, EXTRA, KS, MAX_EPOCH, SHAPE, TEACHERS, ZERO_ROWS, StoredTeacher, decode,  # noqa: E402
                          uamt_cases)

OUT = Path(__file__).resolve().parent / "semi_baselines.npz"
NAMES = Path(__file__).resolve().parent / "hook_factory_names.txt"
MARGIN = 1e-4


def draw(gen, *shape):
    """logits on the 1/8 grid in [-6, 6]; a per-pixel scale spreads the entropies from 0 to ln K"""
    lead, (K, H, W) = shape[:-3], shape[-3:]
    u = torch.rand(*lead, K, H, W, generator=gen) * 12 - 6
    s = torch.rand(*lead[-1:], 1, H, W, generator=gen) ** 2
    return (u * s * 8).round().clamp(-48, 48).to(torch.int8)


def entropy64(zt_q):
    prob = (zt_q.double() / 8).mean(0).softmax(1)
    return -(prob * (prob + 1e-16).log()).sum(1)


def thresholds(K, epochs):
    return [3 / 4 * math.log(K) + 1 / 4 * math.log(K) * float(ep / MAX_EPOCH) for ep in epochs]


def make_inputs(gen, K, epochs, zero_rows):
    N, H, W = SHAPE
    zs, zt = draw(gen, N, K, H, W), draw(gen, TEACHERS, N, K, H, W)
    zt[1:] = (zt[:1] + torch.randint(-6, 7, zt[1:].shape, generator=gen)).clamp(-48, 48).to(torch.int8)
    for _ in range(100):
        h = entropy64(zt)
        near = torch.zeros_like(h, dtype=torch.bool)
        for thr in thresholds(K, epochs):
            near |= (h - thr).abs() < MARGIN
        if zero_rows:
            near[:, :zero_rows] = False
        if not near.any():
            break
        fresh = draw(gen, TEACHERS, N, K, H, W)
        zt = torch.where(near[None, :, None], fresh, zt)
    else:
        raise RuntimeError("could not move every pixel off the thresholds")
    if zero_rows:
        zs[:, :, :zero_rows] = 0
        zt[:, :, :, :zero_rows] = 0
    return zs, zt


def rel(a32, a64):
    d = (a32.double() - a64).flatten()
    return [float(d.norm() / a64.norm()), float(d.abs().max() / a64.abs().max())]


def f32(t):
    return t.detach().to(torch.float32).numpy()


def adopt(hook, cur_epoch=0):
    """what an epocher does to a hook, without an epocher: meters that swallow, cur_epoch and trainer._max_epoch"""
    hook.meters = collections.defaultdict(lambda: types.SimpleNamespace(add=lambda *a, **k: None))
    hook._epocher = types.SimpleNamespace(cur_epoch=cur_epoch, trainer=types.SimpleNamespace(_max_epoch=MAX_EPOCH))
    hook._epocher_init = True
    return hook


def identity(t, mode=None):
    return t


class one_hot_of:
    """the f64 evaluation only: pseudolabel.py:34 and mt.py:241 write `class2one_hot(...).float()`, an f32 target under
    an f64 prediction, which MSELoss cannot differentiate; inside the block `.float()` of that one-hot returns it in
    `dt` instead (0 and 1 are the same numbers in either format)"""

    def __init__(self, dt, *modules):
        self.dt, self.modules = dt, modules

    def __enter__(self):
        self.saved = [m.class2one_hot for m in self.modules]
        for m, real in zip(self.modules, self.saved):
            m.class2one_hot = lambda *a, _real=real, **k: types.SimpleNamespace(float=_real(*a, **k).to(self.dt).clone)

    def __exit__(self, *exc):
        for m, real in zip(self.modules, self.saved):
            m.class2one_hot = real
        return False


def run_both(make_hook, zs, **kwargs):
    """-> {dtype: (loss, dloss/dzs, hook)}"""
    from semi_seg.hooks import mt, pseudolabel
    res = {}
    for dt in (torch.float32, torch.float64):
        z = zs.detach().to(dt).clone().requires_grad_(True)
        hook = make_hook(dt)
        with one_hot_of(dt, mt, pseudolabel):
            loss = hook._call_implementation(unlabeled_tf_logits=z, unlabeled_logits_tf=z, seed=1,
                                             affine_transformer=identity, **kwargs)
        loss.backward()
        res[dt] = (loss.detach(), z.grad, hook)
    return res


def store(out, table, key, res):
    (l32, g32, _), (l64, g64, _) = res[torch.float32], res[torch.float64]
    e = rel(g32, g64) + [float(abs(l32.double() - l64) / abs(l64))]
    out[f"{key}_loss32"], out[f"{key}_loss64"], out[f"{key}_g64"] = np.float32(l32), np.float64(l64), f32(g64)
    out[f"{key}_e_ref"] = np.array(e)
    table.append((key, e))


def factory_names(path):
    """names of the `from semi_seg.hooks import ...` statement of hook_creator.py"""
    for node in ast.walk(ast.parse(path.read_text())):
        if isinstance(node, ast.ImportFrom) and node.module == "semi_seg.hooks":
            return sorted(a.name for a in node.names)
    raise RuntimeError("hook_creator.py does not import from semi_seg.hooks")


def main():
    scratch = gg.setup_reference()
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = type("SummaryWriter", (), {})
    sys.modules["torch.utils.tensorboard"] = tb
    from contrastyou.losses.kl import Entropy
    from semi_seg.hooks.entmin import _EntropyEpocherHook
    from semi_seg.hooks.mt import EMAUpdater, _UAMeanTeacherEpocherHook
    from semi_seg.hooks.pseudolabel import _PLEpocherHook

    NAMES.write_text("\n".join(factory_names(scratch / "ref" / "hook_creator.py")) + "\n")

    out, table = {}, []
    gen = torch.Generator().manual_seed(701)
    inputs = {f"K{K}": make_inputs(gen, K, EPOCHS, ZERO_ROWS) for K in KS}
    inputs[EXTRA[0]] = make_inputs(gen, EXTRA[1], (EXTRA[2],), 0)
    for tag, (zs, zt) in inputs.items():
        out[f"{tag}_zs_i8d8"], out[f"{tag}_zt_i8d8"] = zs.numpy(), zt.numpy()
    inputs = {tag: (decode("zs_i8d8", out[f"{tag}_zs_i8d8"]), decode("zt_i8d8", out[f"{tag}_zt_i8d8"]))
              for tag in inputs}

    # ------------------------------------------------------------------ entropy minimisation, pseudo-label
    for K in KS:
        zs, _ = inputs[f"K{K}"]
        res = run_both(lambda dt: adopt(_EntropyEpocherHook(name="entropy", weight=1.0, criterion=Entropy())), zs)
        store(out, table, f"ent_K{K}", res)
        res = run_both(lambda dt: adopt(_PLEpocherHook(name="plab", weight=1.0, criterion=torch.nn.MSELoss())), zs)
        store(out, table, f"pl_K{K}", res)
        assert torch.equal(zs.float().softmax(1).max(1)[1], zs.double().softmax(1).max(1)[1]), K

    # ------------------------------------------------------------------ UA-MT
    image = torch.zeros(SHAPE[0], 1, *SHAPE[1:])

    def uamt_hook(dt, zt, cur_epoch, hard):
        teacher = StoredTeacher([t.to(dt) for t in zt])
        hook = _UAMeanTeacherEpocherHook(
            name="mt", weight=1.0, criterion=torch.nn.MSELoss(reduction="none"), teacher_model=teacher,
            updater=EMAUpdater(), extra_teachers=torch.nn.ModuleList(), extra_updater=EMAUpdater(update_bn=True),
            hard_clip=hard)
        return adopt(hook, cur_epoch)

    for key, tag, K, ep, hard in uamt_cases():
        zs, zt = inputs[tag]
        res = run_both(lambda dt: uamt_hook(dt, zt, ep, hard), zs, unlabeled_image=image, unlabeled_image_tf=image)
        store(out, table, key, res)
        thr = thresholds(K, (ep,))[0]
        seen = {}
        for dt in (torch.float32, torch.float64):
            hook = res[dt][2]
            assert hook._teacher_model.calls == TEACHERS
            prob, ent = hook._aggregate_predictions(unlabeled_image=image.to(dt), N=4, affine_transformer=identity,
                                                    seed=1)
            seen[dt] = (ent < thr, prob.argmax(1))
        assert torch.equal(seen[torch.float32][0], seen[torch.float64][0]), f"{key}: the f32 mask differs"
        assert torch.equal(seen[torch.float32][1], seen[torch.float64][1]), f"{key}: the f32 arg-max differs"
        out[f"{key}_count"] = np.int64(seen[torch.float64][0].sum())
        out[f"{key}_thr"] = np.float64(thr)

    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {OUT.stat().st_size} bytes; {NAMES}: {len(NAMES.read_text().split())} names")
    print("reference f32 vs f64:  case | grad 2-norm | grad max | loss | mask count")
    for name, e in table:
        count = out.get(f"{name}_count", "")
        print(f"  {name:20s} | {e[0]:.2e} | {e[1]:.2e} | {e[2]:.2e} | {count}")
    del scratch


if __name__ == "__main__":
    main()
