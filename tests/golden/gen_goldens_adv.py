#!/usr/bin/env python3
"""Generate tests/golden/adversarial.npz: the REFERENCE's `Discriminator` (contrastyou/arch/discriminator.py) under
`nn.BCELoss`, evaluated on the CPU in f32 and in f64 through the three discriminator forwards of one
`AdversarialEpocher` step (semi_seg/epochers/comparable.py:141-187), and tests/golden/adversarial_signatures.txt: the
constructor parameter names of the reference's `Discriminator`, `AdversarialEpocher` and `AdversarialTrainer`.

    python tests/golden/gen_goldens_adv.py

Needs the reference checkout (see gen_goldens.py); nothing of it is copied into the repository, only numbers and names.
Layout and encoding: tests/adversarial_fixture.py.
"""
import ast
import sys
from pathlib import Path

import numpy as np
import torch
from torch import nn

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import gen_goldens as gg  # noqa: E402
import gen_goldens_cc  # noqa: E402,F401  (the import stubs of gen_goldens_semi.py)
from adversarial_fixture import (ARMS, BUFFERS, CASES, HIDDEN, K, PARAMS, SEED, arm_tag, decode,  # noqa: E402
                                 generator_gradient64, pin)

OUT = Path(__file__).resolve().parent / "adversarial.npz"
NAMES = Path(__file__).resolve().parent / "adversarial_signatures.txt"


def draw_logits(gen, n, H, W):
    """logits on the 1/8 grid in [-6, 6]; a per-pixel scale spreads the confidences"""
    u = torch.rand(n, K, H, W, generator=gen) * 12 - 6
    s = torch.rand(n, 1, H, W, generator=gen) ** 2
    return (u * s * 8).round().clamp(-48, 48).to(torch.int8)


def rel(a32, a64):
    d = (a32.double() - a64).flatten()
    return [float(d.norm() / a64.norm()), float(d.abs().max() / a64.abs().max())]


def worst(rows):
    return np.max(np.array(rows), axis=0)


def f32(t):
    return t.detach().to(torch.float32).numpy()


def init_names(path, cls):
    """parameter names of `cls.__init__` in the source file `path` (self left out; **name for the catch-all)"""
    for node in ast.walk(ast.parse(path.read_text())):
        if isinstance(node, ast.ClassDef) and node.name == cls:
            for fn in node.body:
                if isinstance(fn, ast.FunctionDef) and fn.name == "__init__":
                    a = fn.args
                    names = [x.arg for x in a.posonlyargs + a.args if x.arg != "self"] + [x.arg for x in a.kwonlyargs]
                    return names + (["**" + a.kwarg.arg] if a.kwarg else [])
    raise RuntimeError(f"{cls}.__init__ not found in {path}")


def step(Discriminator, sd, dt, consider_image, image, lab, unl):
    """the three discriminator forwards of one step, in the step's order -> dict of results in `dt`"""
    dis = Discriminator(5 if consider_image else K, HIDDEN)
    dis.load_state_dict(sd, strict=True)
    dis = dis.to(dt).train()
    criterion = nn.BCELoss()
    image, lab = image.to(dt), lab.to(dt)

    def feed(z):
        return torch.cat([image, z.softmax(1)], dim=1) if consider_image else z.softmax(1)

    res = {}
    z = unl.to(dt).clone().requires_grad_(True)
    out = dis(feed(z))
    gen = criterion(out, torch.zeros_like(out).fill_(1.0))
    gen.backward()
    res["gen_loss"], res["gen_g"] = gen.detach(), z.grad
    dis.zero_grad()
    out_lab = dis(feed(lab.detach()))
    out_unl = dis(feed(unl.to(dt).detach()))
    loss = criterion(out_lab, torch.zeros_like(out_lab).fill_(1.0)) + \
        criterion(out_unl, torch.zeros_like(out_unl).fill_(0.0))
    loss.backward()
    res["out_lab"], res["out_unl"], res["dis_loss"] = out_lab.detach(), out_unl.detach(), loss.detach()
    res["dis_g"] = {n: p.grad for n, p in dis.named_parameters()}
    res["buf"] = {n: b.detach() for n, b in dis.named_buffers()}
    return res


def main():
    scratch = gg.setup_reference()
    from contrastyou.arch.discriminator import Discriminator

    ref = scratch / "ref"
    lines = [f"{cls}: " + " ".join(init_names(ref / rel_path, cls)) for cls, rel_path in (
        ("Discriminator", "contrastyou/arch/discriminator.py"),
        ("AdversarialEpocher", "semi_seg/epochers/comparable.py"),
        ("AdversarialTrainer", "semi_seg/trainers/trainer.py"))]
    NAMES.write_text("\n".join(lines) + "\n")

    out, table = {}, []
    torch.manual_seed(SEED)
    sd1 = {k: v.clone() for k, v in Discriminator(5, HIDDEN).state_dict().items()}
    assert [k for k in sd1 if "running" not in k and "tracked" not in k] == list(PARAMS)
    for k, v in sd1.items():
        out[f"sd_{k}"] = v.numpy()
    gen = torch.Generator().manual_seed(811)
    for tag, (n, ci, H, W) in CASES.items():
        out[f"{tag}_image_i8d32"] = torch.randint(0, 33, (n, ci, H, W), generator=gen).to(torch.int8).numpy()
        out[f"{tag}_lab_i8d8"] = draw_logits(gen, n, H, W).numpy()
        out[f"{tag}_unl_i8d8"] = draw_logits(gen, n, H, W).numpy()

    for tag in CASES:
        image, lab, unl = (decode(k, out[f"{tag}_{k}"]) for k in ("image_i8d32", "lab_i8d8", "unl_i8d8"))
        for arm in ARMS:
            sd = dict(sd1)
            if not arm:
                sd["_main.0.weight"] = sd1["_main.0.weight"][:, 1:].contiguous()
            r32 = step(Discriminator, sd, torch.float32, arm, image, lab, unl)
            r64 = step(Discriminator, sd, torch.float64, arm, image, lab, unl)
            key = f"{tag}_{arm_tag(arm)}"
            for o in ("out_lab", "out_unl"):
                out[f"{key}_{o}64"] = f32(r64[o])
            e_out = worst([rel(r32[o], r64[o]) + [0.0] for o in ("out_lab", "out_unl")])
            for kind in ("gen", "dis"):
                out[f"{key}_{kind}_loss32"] = np.float32(r32[f"{kind}_loss"])
                out[f"{key}_{kind}_loss64"] = np.float64(r64[f"{kind}_loss"])
            out[f"{key}_gen_g64_norm"], out[f"{key}_gen_g64_max"], out[f"{key}_gen_g64_proj"] = pin(r64["gen_g"])
            # what a reader recomputes (torch's layers under the same state dict) is the reference's gradient
            l64, g64 = generator_gradient64(sd, arm, image, unl)
            assert abs(float(l64) - float(r64["gen_loss"])) <= 1e-12 and \
                float((g64 - r64["gen_g"]).abs().max()) <= 1e-12 * float(r64["gen_g"].abs().max()), key
            e_gen = rel(r32["gen_g"], r64["gen_g"]) + [
                float(abs(r32["gen_loss"].double() - r64["gen_loss"]) / abs(r64["gen_loss"]))]
            e_loss = float(abs(r32["dis_loss"].double() - r64["dis_loss"]) / abs(r64["dis_loss"]))
            rows = []
            for name in PARAMS:
                out[f"{key}_dis_g64_{name}"] = f32(r64["dis_g"][name])
                rows.append(rel(r32["dis_g"][name], r64["dis_g"][name]) + [e_loss])
            e_dis = worst(rows)
            rows = []
            for name in BUFFERS:
                b32, b64 = r32["buf"][name], r64["buf"][name]
                if name.endswith("num_batches_tracked"):
                    assert int(b32) == int(b64) == 3
                    out[f"{key}_buf64_{name}"] = b64.numpy()
                else:
                    out[f"{key}_buf64_{name}"] = f32(b64)
                    rows.append(rel(b32, b64) + [0.0])
            e_buf = worst(rows)
            for kind, e in (("out", e_out), ("gen", e_gen), ("dis", e_dis), ("buf", e_buf)):
                out[f"{key}_{kind}_e_ref"] = np.array(e)
                table.append((f"{key}_{kind}", e))
            lo = min(float(r64[o].min()) for o in ("out_lab", "out_unl"))
            hi = max(float(r64[o].max()) for o in ("out_lab", "out_unl"))
            print(f"{key}: outputs in [{lo:.3f}, {hi:.3f}], gen {float(r64['gen_loss']):.6f}, "
                  f"dis {float(r64['dis_loss']):.6f}")

    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {OUT.stat().st_size} bytes; {NAMES}:\n{NAMES.read_text()}")
    print("reference f32 vs f64:  kind | 2-norm | max | loss")
    for name, e in table:
        print(f"  {name:16s} | {e[0]:.2e} | {e[1]:.2e} | {e[2]:.2e}")
    del scratch


if __name__ == "__main__":
    main()
