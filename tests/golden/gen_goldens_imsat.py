#!/usr/bin/env python3
"""Generate tests/golden/imsat.npz: the REFERENCE's IMSAT family -- `imsat_with_entropy`, `imsat_loss`, `IMSATLoss`
(one and two inputs), `IMSATDynamicWeight` (contrastyou/losses/discreteMI.py:20-87,275-297) and the
`_call_implementation` of `_IMSATEpochHook` (semi_seg/hooks/midl.py:71-90) and `_DiscreteIMSATEpochHook`
(semi_seg/hooks/discretemi.py:136-167) -- evaluated on the CPU in f32 and in f64; and
tests/golden/imsat_signatures.txt: the parameter names of the reference's four loss names and two trainer hooks.

    python tests/golden/gen_goldens_imsat.py

Needs the reference checkout (see gen_goldens.py); nothing of it is copied into the repository, only numbers and names.
Layout, decoding and the way distances are measured: tests/imsat_fixture.py.

The hook modules import under the stubs of gen_goldens_cc.py, so both `_call_implementation`s are the reference's own
methods: the output hook is built with the arguments its trainer hook passes; the intermediate hook gets a stand-in
for the feature extractor that returns the stored features, an identity `affine_transformer`, and the reference's
`DenseClusterHead` with 3 sub-heads loaded from `oracle.next_rows.init_cluster_sds`.  The meters are recording
stand-ins.
"""
import ast
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
import imsat_fixture as fx  # noqa: E402

OUT = Path(__file__).resolve().parent / "imsat.npz"
NAMES = Path(__file__).resolve().parent / "imsat_signatures.txt"


def draw(gen, *shape):
    """logits on the 1/8 grid; a per-row scale spreads the confidences"""
    u = torch.randn(*shape, generator=gen)
    s = 0.25 + 2.0 * torch.rand(shape[0], *([1] * (len(shape) - 1)), generator=gen)
    return (u * s * 8).round().clamp(-48, 48).to(torch.int8)


def f32(t):
    return t.detach().to(torch.float32).numpy()


def leaf(t, dt):
    return t.detach().to(dt).clone().requires_grad_(True)


def arg_names(path, cls, fn_name):
    """parameter names of `cls.fn_name` (or of the module-level function `fn_name` for cls None) in `path`"""
    tree = ast.parse(path.read_text())
    body = tree.body if cls is None else next(n for n in ast.walk(tree)
                                              if isinstance(n, ast.ClassDef) and n.name == cls).body
    fn = next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == fn_name)
    a = fn.args
    names = [x.arg for x in a.posonlyargs + a.args if x.arg != "self"] + [x.arg for x in a.kwonlyargs]
    return names + (["**" + a.kwarg.arg] if a.kwarg else [])


class Rec:
    def __init__(self):
        self.got = []

    def add(self, v):
        self.got.append(float(v))


def main():
    scratch = gg.setup_reference()
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = type("SummaryWriter", (), {})
    sys.modules["torch.utils.tensorboard"] = tb
    from oracle import next_rows as onr
    from semi_seg.hooks import discretemi as ref_dmi
    from semi_seg.hooks import midl as ref_midl
    from contrastyou.losses.discreteMI import IMSATDynamicWeight, IMSATLoss, imsat_loss, imsat_with_entropy
    from contrastyou.projectors.heads import DenseClusterHead

    ref = scratch / "ref"
    mi, md, dm = "contrastyou/losses/discreteMI.py", "semi_seg/hooks/midl.py", "semi_seg/hooks/discretemi.py"
    lines = [f"{name}: " + " ".join(arg_names(ref / path, cls, fn)) for name, path, cls, fn in (
        ("imsat_loss", mi, None, "imsat_loss"), ("imsat_with_entropy", mi, None, "imsat_with_entropy"),
        ("IMSATLoss", mi, "IMSATLoss", "__init__"), ("IMSATLoss.forward", mi, "IMSATLoss", "forward"),
        ("IMSATDynamicWeight", mi, "IMSATDynamicWeight", "__init__"),
        ("IMSATDynamicWeight.forward", mi, "IMSATDynamicWeight", "forward"),
        ("IMSATTrainHook", md, "IMSATTrainHook", "__init__"),
        ("DiscreteIMSATTrainHook", dm, "DiscreteIMSATTrainHook", "__init__"))]
    NAMES.write_text("\n".join(lines) + "\n")

    out, table = {}, []
    gen = torch.Generator().manual_seed(1207)
    for tag, (K, R) in fx.ROW_CASES.items():
        out[f"{tag}_z_i8d8"] = draw(gen, R, K).numpy()
    for tag, shape in fx.MAP_CASES.items():
        out[f"{tag}_z_i8d8"] = draw(gen, *shape).numpy()
    for tag in fx.PAIR_CASES:
        K, R = fx.ROW_CASES[tag]
        # the second view: the first one perturbed, as two augmentations of one image are
        z = fx.decode(out[f"{tag}_z_i8d8"]) * 8 + draw(gen, R, K).float() * 0.25
        out[f"{tag}_z2_i8d8"] = z.round().clamp(-48, 48).to(torch.int8).numpy()

    def scalars(p, dt):
        x = leaf(p, dt)
        marg, cond = imsat_with_entropy(x)
        loss = imsat_loss(x, lamda=fx.LAMDA)
        rows = x if x.dim() == 2 else None
        if rows is not None:  # the class is the function on 2-D inputs
            assert float((IMSATLoss(lamda=fx.LAMDA)(rows) - loss).detach().abs()) == 0.0
        loss.backward()
        return marg.detach(), cond.detach(), loss.detach(), x.grad

    for tag in fx.all_cases():
        p = fx.case_probs(out, tag)
        m32, c32, l32, g32 = scalars(p, torch.float32)
        m64, c64, l64, g64 = scalars(p, torch.float64)
        # what a reader recomputes from the formulas is the reference's value
        mm, cc = fx.entropies64(p.double())
        assert abs(float(mm - m64)) <= 1e-12 and abs(float(cc - c64)) <= 1e-12, tag
        out[f"{tag}_marg64"], out[f"{tag}_cond64"], out[f"{tag}_loss64"] = (np.float64(v) for v in (m64, c64, l64))
        out[f"{tag}_g64"] = f32(g64)
        e = [fx.rel_vec(torch.stack([m32, c32]), torch.stack([m64, c64]))] + fx.rel_grad(g32, g64)
        out[f"{tag}_e_ref"] = np.array(e)
        table.append((tag, e))

    for tag in fx.PAIR_CASES:
        p1, p2 = fx.probs(fx.decode(out[f"{tag}_z_i8d8"])), fx.probs(fx.decode(out[f"{tag}_z2_i8d8"]))
        res = {}
        for dt in (torch.float32, torch.float64):
            a, b = leaf(p1, dt), leaf(p2, dt)
            crit = IMSATLoss(lamda=fx.LAMDA)
            loss = crit(a, b)
            loss.backward()
            ents = torch.stack([*imsat_with_entropy(a.detach()), *imsat_with_entropy(b.detach())])
            res[dt] = (loss.detach(), a.grad, b.grad, ents, crit.get_joint_matrix())
        (l32, a32, b32, s32, _), (l64, a64, b64, s64, joint) = res[torch.float32], res[torch.float64]
        out[f"{tag}_pair_loss64"] = np.float64(l64)
        out[f"{tag}_pair_g1_64"], out[f"{tag}_pair_g2_64"] = f32(a64), f32(b64)
        out[f"{tag}_pair_joint64"] = np.asarray(joint, dtype=np.float32)
        e1, e2 = fx.rel_grad(a32, a64), fx.rel_grad(b32, b64)
        e = [fx.rel_vec(s32, s64), max(e1[0], e2[0]), max(e1[1], e2[1])]
        out[f"{tag}_pair_e_ref"] = np.array(e)
        table.append((f"{tag} pair", e))

    # IMSATDynamicWeight: without the update, and three consecutive calls with it
    p = fx.case_probs(out, fx.DYN_CASE)
    res = {}
    for dt in (torch.float32, torch.float64):
        off = IMSATDynamicWeight(lamda=fx.DYN_LAMDA, use_dynamic=False)
        l_off = off(p.to(dt)).detach()
        w_off = off.dynamic_weight.detach().clone()
        dyn = IMSATDynamicWeight(lamda=fx.DYN_LAMDA, use_dynamic=True)
        assert list(dyn.state_dict()) == ["dynamic_weight"]
        losses, ws, g = [], [], None
        for i in range(fx.DYN_CALLS):
            x = leaf(p, dt)
            loss = dyn(x)
            if i == 0:
                loss.backward()
                g = x.grad
            losses.append(loss.detach())
            ws.append(dyn.dynamic_weight.detach().clone())
        res[dt] = (l_off, w_off, torch.stack(losses), torch.stack(ws), g)
    (lo32, wo32, l32, w32, g32), (lo64, wo64, l64, w64, g64) = res[torch.float32], res[torch.float64]
    out["dyn_off_loss64"], out["dyn_off_w64"] = np.float64(lo64), np.float64(wo64)
    out["dyn_loss64"], out["dyn_w64"], out["dyn_g64"] = l64.numpy(), w64.numpy(), f32(g64)
    scale = float(out[f"{fx.DYN_CASE}_cond64"]) + fx.DYN_LAMDA * float(out[f"{fx.DYN_CASE}_marg64"])
    e = [max(float((l32.double() - l64).abs().max()) / scale, fx.rel_vec(w32, w64))] + fx.rel_grad(g32, g64)
    out["dyn_e_ref"] = np.array(e)
    table.append(("dynamic weight", e))

    # _IMSATEpochHook (built directly: the reference's trainer hooks register their names once per process)
    h = fx.HOOK_OUT
    out["out_tf_logits_i8d8"] = draw(gen, h["n"], h["K"], h["H"], h["W"]).numpy()
    out["out_logits_tf_i8d8"] = draw(gen, h["n"], h["K"], h["H"], h["W"]).numpy()
    res = {}
    for dt in (torch.float32, torch.float64):
        hook = ref_midl._IMSATEpochHook(name="imsat", weight=h["weight"])
        hook.meters = {"mi": Rec()}
        a, b = leaf(fx.decode(out["out_tf_logits_i8d8"]), dt), leaf(fx.decode(out["out_logits_tf_i8d8"]), dt)
        value = hook._call_implementation(unlabeled_tf_logits=a, unlabeled_logits_tf=b)
        value.backward()
        ents = [imsat_with_entropy(t.detach().softmax(1)) for t in (a, b)]
        scale = h["weight"] * 0.5 * sum(float(m.abs() + c.abs()) for m, c in ents)
        res[dt] = (value.detach(), a.grad, b.grad, hook.meters["mi"].got, scale)
    (v32, a32, b32, _, _), (v64, a64, b64, got, scale) = res[torch.float32], res[torch.float64]
    out["out_value64"], out["out_scale64"], out["out_meter_mi64"] = np.float64(v64), np.float64(scale), np.array(got)
    out["out_g_tf_logits64"], out["out_g_logits_tf64"] = f32(a64), f32(b64)
    e1, e2 = fx.rel_grad(a32, a64), fx.rel_grad(b32, b64)
    e = [float(abs(v32.double() - v64)) / scale, max(e1[0], e2[0]), max(e1[1], e2[1])]
    out["out_e_ref"] = np.array(e)
    table.append(("output hook", e))

    # _DiscreteIMSATEpochHook on stored features
    h = fx.HOOK_MID
    out["mid_feat_i8d8"] = draw(gen, 2 * h["n_unl"], h["C"], h["H"], h["W"]).numpy()
    sds = onr.init_cluster_sds(h["C"], h["clusters"], h["subheads"], True, seed=h["seed"])
    sd = {f"_headers.{i}.{k}": v for i, s in enumerate(sds) for k, v in s.items()}
    res = {}
    for dt in (torch.float32, torch.float64):
        head = DenseClusterHead(input_dim=h["C"], num_clusters=h["clusters"], num_subheads=h["subheads"],
                                head_type="linear", T=1, normalize=False)
        head.load_state_dict(sd, strict=True)
        head = head.to(dt)
        feat = leaf(fx.decode(out["mid_feat_i8d8"]), dt)
        extractor = types.SimpleNamespace(bind=lambda: None, remove=lambda: None, feature=lambda: feat)
        hook = ref_dmi._DiscreteIMSATEpochHook(
            name="imsat_mid", weight=h["weight"], extractor=extractor, projector=head,
            criterion=IMSATLoss(lamda=1.0), cons_criterion=torch.nn.MSELoss(), cons_weight=h["cons_weight"])
        hook.meters = {"mi": Rec(), "cons": Rec()}
        images = torch.zeros(h["n_unl"], 1, 8, 8)
        value = hook._call_implementation(unlabeled_image=images, unlabeled_image_tf=images,
                                          affine_transformer=lambda x: x)
        value.backward()
        with torch.no_grad():
            scale = 0.0
            for prob in head(feat):
                for half in torch.chunk(prob, 2, 0):
                    m, c = imsat_with_entropy(half)
                    scale += 0.5 * float(m.abs() + c.abs())
            scale = h["weight"] * scale / h["subheads"] + h["cons_weight"] * hook.meters["cons"].got[0]
        res[dt] = (value.detach(), feat.grad, {n: q.grad for n, q in head.named_parameters()},
                   hook.meters["mi"].got, hook.meters["cons"].got, scale)
    (v32, f32_, p32, _, _, _), (v64, f64_, p64, mi_got, cons_got, scale) = res[torch.float32], res[torch.float64]
    out["mid_value64"], out["mid_scale64"] = np.float64(v64), np.float64(scale)
    out["mid_meter_mi64"], out["mid_meter_cons64"] = np.array(mi_got), np.array(cons_got)
    out["mid_g_feat64"] = f32(f64_)
    rows = [fx.rel_grad(f32_, f64_)]
    for n in p64:
        out[f"mid_g_{n}64"] = f32(p64[n])
        rows.append(fx.rel_grad(p32[n], p64[n]))
    worst = np.max(np.array(rows), axis=0)
    e = [float(abs(v32.double() - v64)) / scale, float(worst[0]), float(worst[1])]
    out["mid_e_ref"] = np.array(e)
    table.append(("intermediate hook", e))

    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {OUT.stat().st_size} bytes; {NAMES}:\n{NAMES.read_text()}")
    print("reference f32 vs f64:  case | scalars | gradient 2-norm | gradient max-norm")
    for name, e in table:
        print(f"  {name:18s} | {e[0]:.2e} | {e[1]:.2e} | {e[2]:.2e}")
    for mid in (False, True):
        print("tolerances" + (" (intermediate hook)" if mid else ""),
              {k: f"{v:.2e}" for k, v in fx.tolerances(out, mid).items()})
    del scratch


if __name__ == "__main__":
    main()
