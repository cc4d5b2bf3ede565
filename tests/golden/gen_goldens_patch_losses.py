#!/usr/bin/env python3
"""Generate tests/golden/patch_losses.npz: the REFERENCE's `IIDSegmentationSmallPathLoss` / `patch_generator`
(contrastyou/losses/discreteMI.py:173-198,264-272), `PUILoss` / `PUISegLoss` (contrastyou/losses/pica_loss.py) and
`JSD_div` / `EntropyPrior` (contrastyou/losses/kl.py:63-78,142-174), evaluated on the CPU in f32 and in f64; and
tests/golden/patch_losses_signatures.txt: the parameter names of these classes and of `patch_generator`.

    python tests/golden/gen_goldens_patch_losses.py

Needs the reference checkout (see gen_goldens.py); nothing of it is copied into the repository, only numbers and names.
Layout, decoding and the way distances are measured: tests/patch_losses_fixture.py.
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
import patch_losses_fixture as fx  # noqa: E402
from gen_goldens_imsat import arg_names, draw, f32, leaf  # noqa: E402

OUT = Path(__file__).resolve().parent / "patch_losses.npz"
NAMES = Path(__file__).resolve().parent / "patch_losses_signatures.txt"


def main():
    scratch = gg.setup_reference()
    from contrastyou.losses.kl import Entropy
    # discreteMI.py imports semi_seg.hooks.midl (-> tensorboard, absent) for one module attribute: the stand-in of
    # gen_goldens.py:77-85
    midl = types.ModuleType("semi_seg.hooks.midl")
    midl.entropy_criterion = Entropy(reduction="none", eps=1e-8)
    hooks_pkg = types.ModuleType("semi_seg.hooks")
    hooks_pkg.midl = midl
    hooks_pkg.__path__ = []
    sys.modules.setdefault("semi_seg.hooks", hooks_pkg)
    sys.modules.setdefault("semi_seg.hooks.midl", midl)
    from contrastyou.losses.discreteMI import IIDSegmentationSmallPathLoss, patch_generator
    from contrastyou.losses.kl import EntropyPrior, JSD_div
    from contrastyou.losses.pica_loss import PUILoss, PUISegLoss

    ref = scratch / "ref"
    mi, pica, kl = "contrastyou/losses/discreteMI.py", "contrastyou/losses/pica_loss.py", "contrastyou/losses/kl.py"
    lines = [f"{name}: " + " ".join(arg_names(ref / path, cls, fn)) for name, path, cls, fn in (
        ("IIDSegmentationSmallPathLoss", mi, "IIDSegmentationSmallPathLoss", "__init__"),
        ("IIDSegmentationSmallPathLoss.__call__", mi, "IIDSegmentationSmallPathLoss", "__call__"),
        ("patch_generator", mi, None, "patch_generator"),
        ("PUILoss", pica, "PUILoss", "__init__"), ("PUILoss.forward", pica, "PUILoss", "forward"),
        ("PUISegLoss", pica, "PUISegLoss", "__init__"), ("PUISegLoss.forward", pica, "PUISegLoss", "forward"),
        ("JSD_div", kl, "JSD_div", "__init__"), ("JSD_div.forward", kl, "JSD_div", "forward"),
        ("EntropyPrior", kl, "EntropyPrior", "__init__"), ("EntropyPrior.forward", kl, "EntropyPrior", "forward"))]
    NAMES.write_text("\n".join(lines) + "\n")

    out, table = {}, []
    gen = torch.Generator().manual_seed(1733)

    def record(tag, run, ps):
        """run(inputs as leaves of a dtype) -> (value to store, scalar to differentiate)"""
        res = {}
        for dt in (torch.float32, torch.float64):
            xs = [leaf(p, dt) for p in ps]
            value, scalar = run(xs)
            scalar.backward()
            assert bool(torch.isfinite(value).all()) and all(bool(torch.isfinite(x.grad).all()) for x in xs), tag
            res[dt] = (value.detach(), [x.grad for x in xs])
        (v32, g32), (v64, g64) = res[torch.float32], res[torch.float64]
        out[f"{tag}_loss64"] = np.float64(v64) if v64.dim() == 0 else f32(v64)
        rows = []
        for i, (a, b) in enumerate(zip(g32, g64), 1):
            out[f"{tag}_g{i}_64"] = f32(b)
            rows.append(fx.rel_grad(a, b))
        worst = np.max(np.array(rows), axis=0)
        e = [fx.rel_vec(v32, v64), float(worst[0]), float(worst[1])]
        out[f"{tag}_e_ref"] = np.array(e)
        table.append((tag, e))

    # patch-wise IIC.  The reference multiplies a mask into views of its inputs in place: the inputs handed to it are
    # copies inside the graph, never the leaves
    for tag, (n, k, H, W, patch, pad) in fx.PATCH_CASES.items():
        out[f"{tag}_z1_i8d8"] = draw(gen, n, k, H, W).numpy()
        out[f"{tag}_z2_i8d8"] = draw(gen, n, k, H, W).numpy()
    n, k, H, W, patch, pad = fx.PATCH_CASES[fx.MASK_OF]
    mask = (torch.rand(n, 1, H, W, generator=gen) > 0.3)
    out[f"{fx.MASK_CASE}_mask"] = mask.numpy().astype(np.uint8)
    for tag in list(fx.PATCH_CASES) + [fx.MASK_CASE]:
        n, k, H, W, patch, pad = fx.PATCH_CASES[fx.MASK_OF if tag == fx.MASK_CASE else tag]
        crit = IIDSegmentationSmallPathLoss(lamda=fx.LAMDA, padding=pad, patch_size=patch)

        def run(xs, crit=crit, tag=tag):
            if tag == fx.MASK_CASE:
                v = crit(xs[0] * 1.0, xs[1] * 1.0, mask.to(xs[0].dtype))
            else:
                v = crit(xs[0], xs[1])
            return v, v
        record(tag, run, fx.inputs(out, tag))

    # the origins of patch_generator, read off the views it yields
    for L, p, s in fx.ORIGIN_CASES:
        ramp = torch.arange(L, dtype=torch.float32).view(1, 1, L, 1).expand(1, 1, L, 2)
        views = list(patch_generator(ramp, (p, 2), (s, 1)))
        origins = sorted({int(v[0, 0, 0, 0]) for v in views})
        assert all(v.shape[2] == min(p, L) for v in views)
        out[f"origins_{L}_{p}_{s}"] = np.array(origins, dtype=np.int32)

    for tag, (shape, pad) in fx.PUISEG_CASES.items():
        out[f"{tag}_z1_i8d8"], out[f"{tag}_z2_i8d8"] = draw(gen, *shape).numpy(), draw(gen, *shape).numpy()
        crit = PUISegLoss(lamda=fx.PUI_LAMDA, padding=pad)

        def run(xs, crit=crit):
            v = crit(xs[0], xs[1])
            return v, v
        record(tag, run, fx.inputs(out, tag))

    for tag, shape in fx.PUI_CASES.items():
        out[f"{tag}_z1_i8d8"], out[f"{tag}_z2_i8d8"] = draw(gen, *shape).numpy(), draw(gen, *shape).numpy()
        crit = PUILoss(lamda=fx.PUI_LAMDA)

        def run(xs, crit=crit):
            v = crit(xs[0], xs[1])
            return v, v
        record(tag, run, fx.inputs(out, tag))

    for tag, (m, shape, red) in fx.JSD_CASES.items():
        for i in range(1, m + 1):
            out[f"{tag}_z{i}_i8d8"] = draw(gen, *shape).numpy()
        crit = JSD_div(reduction=red, eps=fx.EPS)

        def run(xs, crit=crit):
            v = crit(*xs)
            return v, (v if v.dim() == 0 else (v * fx.none_weights(v)).sum())
        record(tag, run, fx.inputs(out, tag, m))

    for tag, (shape, given) in fx.PRIOR_CASES.items():
        out[f"{tag}_z1_i8d8"] = draw(gen, *shape).numpy()
        prior = torch.softmax(torch.randn(1, shape[1], generator=gen), 1) if given else None
        if given:
            out[f"{tag}_prior"] = prior.numpy()
        crit = EntropyPrior(reduction="mean", eps=fx.EPS)

        def run(xs, crit=crit, prior=prior):
            v = crit(xs[0], None if prior is None else prior.to(xs[0].dtype))
            return v, v
        record(tag, run, fx.inputs(out, tag, 1))

    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {OUT.stat().st_size} bytes; {NAMES}:\n{NAMES.read_text()}")
    print("reference f32 vs f64:  case | value | gradient 2-norm | gradient max-norm")
    for name, e in table:
        print(f"  {name:14s} | {e[0]:.2e} | {e[1]:.2e} | {e[2]:.2e}")
    print("tolerances", {k: f"{v:.2e}" for k, v in fx.tolerances(out).items()})
    del scratch


if __name__ == "__main__":
    main()
