#!/usr/bin/env python3
"""Generate tests/golden/multicore_adaptive.npz and multicore_adaptive_gz.npz (the logit gradients): the REFERENCE's
`AdaptiveOverSegmentedLoss`, `StricterAdaptiveOverSegmentedLoss`, `StricterAdaptiveOverSegmentedLossWithMI` (and
`MultiCoreKL` on interleaved groups) on `softmax(z)` and `class2one_hot(t, C)`, evaluated on the CPU in f32 and in f64
on seeded logits and translation matrices.

    python tests/golden/gen_goldens_adaptive.py

Needs the reference checkout (see gen_goldens.py); nothing of it is copied into the repository, only numbers.
Layout and encoding: tests/adaptive_fixture.py.  The translation matrix is written into `_translate_matrix` before the
evaluation (the constructor's randn is not reproduced).  The f64 evaluation casts the criterion with `.double()` (and
the plain-attribute diagonal of the stricter criteria with it): as written, an f32 parameter meets an f64 simplex.
No pixel is ever left out of a comparison: a pixel whose two largest f64 reduced probabilities lie within a relative
MARGIN of each other is redrawn, and the reference's f32 arg-max is asserted to equal its f64 arg-max everywhere.
"""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import gen_goldens as gg  # noqa: E402
import gen_goldens_cc  # noqa: E402,F401  (its loguru stub)
import gen_goldens_multicore as gm  # noqa: E402
from gen_goldens_semi import f32, rel  # noqa: E402
from adaptive_fixture import (BIG, BIG_KEY, BIG_ROWS, CASES, FILES, MARGIN, MI_WEIGHT, SHAPE, big_inputs,  # noqa: E402
                              decode, drop_last_class_in_image0, interleaved_groups, param_shape, pixel_rows, tag)

OUT, OUT_GZ = (Path(__file__).resolve().parent / name for name in FILES)
NAN = float("nan")


def reference_classes():
    """the reference's classes, imported the way gen_goldens_multicore.main() imports MultiCoreKL"""
    import types
    scratch = gg.setup_reference()
    writer = types.ModuleType("contrastyou.writer")
    writer.get_tb_writer = lambda *a, **k: None
    writer.SummaryWriter = type("SummaryWriter", (), {})
    sys.modules["contrastyou.writer"] = writer
    hooks_pkg = types.ModuleType("semi_seg.hooks")
    hooks_pkg.__path__ = [str(scratch / "ref" / "semi_seg" / "hooks")]
    sys.modules["semi_seg.hooks"] = hooks_pkg
    from contrastyou.losses import multicore_loss as ml
    from contrastyou.utils import class2one_hot
    return scratch, ml, class2one_hot


def make(ml, kind, K, C, T, dt):
    """the reference criterion of a case with its parameter set to T, in dtype dt"""
    if kind == "member":
        return ml.MultiCoreKL(groups=interleaved_groups(K, C))
    if kind == "adaptive":
        crit = ml.AdaptiveOverSegmentedLoss(K, C, "cpu")
    elif kind == "stricter":
        crit = ml.StricterAdaptiveOverSegmentedLoss(K, C, "cpu")
    else:
        crit = ml.StricterAdaptiveOverSegmentedLossWithMI(K, C, "cpu", mi_weight=MI_WEIGHT)
    assert list(crit.state_dict()) == ["_translate_matrix"]
    assert tuple(crit._translate_matrix.shape) == param_shape(kind, K, C)
    with torch.no_grad():
        crit._translate_matrix.copy_(T)
    if dt == torch.float64:
        crit = crit.double()
        if hasattr(crit, "_diagonal_matrix"):
            crit._diagonal_matrix = crit._diagonal_matrix.double()
    return crit


def draw_T(gen, shape):
    """a translation matrix on the 1/8 grid in [-2, 2], as int8 = 8 * value"""
    return torch.randint(-16, 17, shape, generator=gen).to(torch.int8)


def run(ml, class2one_hot, kind, K, C, T, z, t):
    res = {}
    for dt in (torch.float32, torch.float64):
        crit = make(ml, kind, K, C, T, dt)
        zz = z.detach().to(dt).clone().requires_grad_(True)
        loss = crit(zz.softmax(1), class2one_hot(t, C))
        loss.backward()
        with torch.no_grad():
            arg = crit.reduced_simplex(zz.softmax(1)).max(1)[1]
        gT = getattr(crit, "_translate_matrix", None)
        gT = gT.grad if gT is not None and gT.numel() > 0 else None
        res[dt] = (loss.detach(), zz.grad, gT, arg)
    return res


def store(out, table, key, res, rows=None):
    (l32, g32, T32, a32), (l64, g64, T64, a64) = res[torch.float32], res[torch.float64]
    assert torch.equal(a32, a64), f"{key}: the f32 reduced arg-max differs from the f64 one"
    e = rel(g32, g64) + (rel(T32, T64) if T64 is not None else [NAN, NAN]) + [float(abs(l32.double() - l64) / abs(l64))]
    out[f"{key}_loss32"], out[f"{key}_loss64"] = np.float32(l32), np.float64(l64)
    out[f"{key}_gz64"] = f32(g64) if rows is None else f32(pixel_rows(g64, rows))
    if T64 is not None:
        out[f"{key}_gT64"] = f32(T64)
    out[f"{key}_argmax"] = a64.numpy().astype(np.uint8)
    out[f"{key}_e_ref"] = np.array(e)
    table.append((key, e))


def main():
    scratch, ml, class2one_hot = reference_classes()
    out, table = {}, []
    gen = torch.Generator().manual_seed(1902)
    N, H, W = SHAPE
    redrawn = 0
    for kind, K, C in CASES:
        key = tag(kind, K, C)
        shape = param_shape(kind, K, C)
        T_q = draw_T(gen, shape) if shape is not None else None
        T = T_q.float() / 8 if T_q is not None else None
        probe = make(ml, kind, K, C, T, torch.float64)
        with torch.no_grad():
            z_q, n = gm.settle(probe, gm.draw(gen, N, K, H, W), lambda: gm.draw(gen, N, K, H, W))
        redrawn += n
        t = drop_last_class_in_image0(torch.randint(0, C, (N, H, W), generator=gen).numpy().astype(np.uint8), C)
        out[f"{key}_z_i8d8"], out[f"{key}_t"] = z_q.numpy(), t
        if T_q is not None:
            out[f"{key}_T_i8d8"] = T_q.numpy()
        store(out, table, key, run(ml, class2one_hot, kind, K, C, T, decode(f"{key}_z_i8d8", out[f"{key}_z_i8d8"]),
                                   torch.from_numpy(t).long()))

    kind, K, C, _ = BIG
    z_q, t, T_q = big_inputs()
    z_q, t, T = torch.from_numpy(z_q), torch.from_numpy(t).long(), torch.from_numpy(T_q).float() / 8
    with torch.no_grad():
        assert not gm.near_tie(make(ml, kind, K, C, T, torch.float64), z_q).any(), \
            "adaptive_fixture.BIG_SEED draws a near tie: pick another seed"
    store(out, table, BIG_KEY, run(ml, class2one_hot, kind, K, C, T, z_q.float() / 8, t), rows=BIG_ROWS)

    np.savez_compressed(OUT, **{k: v for k, v in out.items() if not k.endswith("_gz64")})
    np.savez_compressed(OUT_GZ, **{k: v for k, v in out.items() if k.endswith("_gz64")})
    print(f"{OUT}: {OUT.stat().st_size} bytes, {OUT_GZ.name}: {OUT_GZ.stat().st_size} bytes; "
          f"{redrawn} pixels redrawn off a near tie (MARGIN {MARGIN})")
    print("reference f32 vs f64:  case | dz 2-norm | dz max | dT 2-norm | dT max | loss")
    for name, e in table:
        print(f"  {name:18s} | " + " | ".join(f"{v:.2e}" for v in e))
    worst = np.nanmax(np.array([e for _, e in table]), axis=0)
    print("  largest            | " + " | ".join(f"{v:.2e}" for v in worst))
    del scratch


if __name__ == "__main__":
    main()
