#!/usr/bin/env python3
"""Generate tests/golden/multicore.npz: the REFERENCE's `MultiCoreKL(groups=list(grouper(range(K), C)))` on
`softmax(z)` and `class2one_hot(t, C)`, its `reduced_simplex` arg-max, and its `_ConsistencyEpocherHook` at
16 < K <= 64, evaluated on the CPU in f32 and in f64 on seeded logits.

    python tests/golden/gen_goldens_multicore.py

Needs the reference checkout (see gen_goldens.py); nothing of it is copied into the repository, only numbers.
Layout and encoding: tests/multicore_fixture.py.  Stored per case: the f64 loss, the f64 gradient (rounded to f32), the
reduced arg-max, and the reference's own f32-to-f64 distances `e_ref` = [2-norm, element-wise max, loss], relative as
in the tolerance rule of tests/test_gpu_cc.py.
No pixel is ever left out of a comparison: a pixel whose two largest f64 reduced probabilities lie within a relative
MARGIN of each other is redrawn, and the reference's f32 arg-max is asserted to equal its f64 arg-max everywhere.
"""
import ast
import sys
import types
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import gen_goldens as gg  # noqa: E402
import gen_goldens_cc  # noqa: E402,F401  (its loguru stub)
from gen_goldens_semi import adopt, f32, identity, rel  # noqa: E402
from multicore_fixture import (BIG, BIG_ROWS, CASES, CONS_KS, CONS_SHAPE, MARGIN, SHAPE, big_inputs, decode,  # noqa: E402
                               groups_of, pixel_rows, tag)

OUT = Path(__file__).resolve().parent / "multicore.npz"


def draw(gen, N, K, H, W):
    """logits on the 1/8 grid in [-6, 6], as int8 = 8 * logit"""
    return torch.randint(-48, 49, (N, K, H, W), generator=gen).to(torch.int8)


def near_tie(crit, z_q):
    """pixels whose two largest f64 reduced probabilities are closer than MARGIN (relative)"""
    top = crit.reduced_simplex((z_q.double() / 8).softmax(1)).topk(2, dim=1)[0]
    return (top[:, 0] - top[:, 1]) < MARGIN * top[:, 0]


def settle(crit, z_q, redraw):
    for _ in range(100):
        near = near_tie(crit, z_q)
        if not near.any():
            return z_q, int(near.sum())
        z_q = torch.where(near[:, None], redraw(), z_q)
    raise RuntimeError("could not move every pixel off a tie")


def run_kl(crit, class2one_hot, z, t, C):
    res = {}
    for dt in (torch.float32, torch.float64):
        zz = z.detach().to(dt).clone().requires_grad_(True)
        loss = crit(zz.softmax(1), class2one_hot(t, C))
        loss.backward()
        with torch.no_grad():
            arg = crit.reduced_simplex(zz.softmax(1)).max(1)[1]
        res[dt] = (loss.detach(), zz.grad, arg)
    return res


def store_kl(out, table, key, res, rows=None):
    (l32, g32, a32), (l64, g64, a64) = res[torch.float32], res[torch.float64]
    assert torch.equal(a32, a64), f"{key}: the f32 reduced arg-max differs from the f64 one"
    e = rel(g32, g64) + [float(abs(l32.double() - l64) / abs(l64))]
    out[f"{key}_loss32"], out[f"{key}_loss64"] = np.float32(l32), np.float64(l64)
    out[f"{key}_g64"] = f32(g64) if rows is None else f32(pixel_rows(g64, rows))
    out[f"{key}_argmax"] = a64.numpy().astype(np.uint8)
    out[f"{key}_e_ref"] = np.array(e)
    table.append((key, e))


def reference_function(path, name):
    """one top-level function of a reference module whose other imports (omegaconf, prettytable) are absent here: its
    definition alone is compiled from the checkout and run"""
    tree = ast.parse(path.read_text())
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
    scope = {}
    exec(compile(ast.Module(body=[node], type_ignores=[]), str(path), "exec"), scope)
    return scope[name]


def main():
    scratch = gg.setup_reference()
    # semi_seg/hooks/__init__.py pulls every hook and contrastyou.losses.discreteMI imports semi_seg.hooks.midl back:
    # the package is entered as a bare namespace with its real path, `contrastyou.writer` (tensorboard) is pre-seeded
    writer = types.ModuleType("contrastyou.writer")
    writer.get_tb_writer = lambda *a, **k: None
    writer.SummaryWriter = type("SummaryWriter", (), {})
    sys.modules["contrastyou.writer"] = writer
    hooks_pkg = types.ModuleType("semi_seg.hooks")
    hooks_pkg.__path__ = [str(scratch / "ref" / "semi_seg" / "hooks")]
    sys.modules["semi_seg.hooks"] = hooks_pkg
    from contrastyou.losses.multicore_loss import MultiCoreKL
    from contrastyou.utils import class2one_hot
    from semi_seg.hooks.consistency import _ConsistencyEpocherHook
    grouper = reference_function(scratch / "ref" / "utils.py", "grouper")  # (main_multicore.py:18,57)

    out, table = {}, []
    gen = torch.Generator().manual_seed(1801)

    # ------------------------------------------------------------------ MultiCoreKL
    N, H, W = SHAPE
    redrawn = 0
    for C, m in CASES:
        K, key = C * m, tag(C, m)
        groups = list(grouper(range(K), C))
        assert groups == groups_of(C, m), (C, m)
        crit = MultiCoreKL(groups=groups)
        z_q, n = settle(crit, draw(gen, N, K, H, W), lambda: draw(gen, N, K, H, W))
        redrawn += n
        t = torch.randint(0, C, (N, H, W), generator=gen)
        out[f"{key}_z_i8d8"], out[f"{key}_t"] = z_q.numpy(), t.numpy().astype(np.uint8)
        store_kl(out, table, key, run_kl(crit, class2one_hot, decode(f"{key}_z_i8d8", out[f"{key}_z_i8d8"]), t, C))

    C, m, _ = BIG
    crit = MultiCoreKL(groups=list(grouper(range(C * m), C)))
    z_q, t = big_inputs()
    z_q, t = torch.from_numpy(z_q), torch.from_numpy(t).long()
    assert not near_tie(crit, z_q).any(), "multicore_fixture.BIG_SEED draws a near tie: pick another seed"
    store_kl(out, table, "kl_big", run_kl(crit, class2one_hot, z_q.float() / 8, t, C), rows=BIG_ROWS)

    # ------------------------------------------------------------------ consistency at 16 < K <= 64
    N, H, W = CONS_SHAPE
    for K in CONS_KS:
        key = f"cons_K{K}"
        a_q = draw(gen, N, K, H, W)
        b_q = (a_q + torch.randint(-12, 13, a_q.shape, generator=gen)).clamp(-48, 48).to(torch.int8)
        out[f"{key}_a_i8d8"], out[f"{key}_b_i8d8"] = a_q.numpy(), b_q.numpy()
        a, b = decode(f"{key}_a_i8d8", out[f"{key}_a_i8d8"]), decode(f"{key}_b_i8d8", out[f"{key}_b_i8d8"])
        res = {}
        for dt in (torch.float32, torch.float64):
            bb = b.to(dt).clone().requires_grad_(True)
            hook = adopt(_ConsistencyEpocherHook(name="consistency", weight=1.0, criterion=torch.nn.MSELoss()))
            loss = hook._call_implementation(unlabeled_tf_logits=bb, unlabeled_logits_tf=a.to(dt), seed=1,
                                             affine_transformer=identity)
            loss.backward()
            res[dt] = (loss.detach(), bb.grad)
        (l32, g32), (l64, g64) = res[torch.float32], res[torch.float64]
        e = rel(g32, g64) + [float(abs(l32.double() - l64) / abs(l64))]
        out[f"{key}_loss32"], out[f"{key}_loss64"], out[f"{key}_g64"] = np.float32(l32), np.float64(l64), f32(g64)
        out[f"{key}_e_ref"] = np.array(e)
        table.append((key, e))

    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {OUT.stat().st_size} bytes; {redrawn} pixels redrawn off a near tie")
    print("reference f32 vs f64:  case | grad 2-norm | grad max | loss")
    for name, e in table:
        print(f"  {name:12s} | {e[0]:.2e} | {e[1]:.2e} | {e[2]:.2e}")
    del scratch


if __name__ == "__main__":
    main()
