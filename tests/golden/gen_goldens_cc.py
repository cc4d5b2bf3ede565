#!/usr/bin/env python3
"""Generate tests/golden/cc.npz: the REFERENCE's cross-correlation family (CCLoss, the cc_loss_per_head of
ccblock.py and cc.py, CrossCorrelationProjector, one composed _ProjectorEpocherGeneralHook call) evaluated on the CPU
in f32 and in f64 on seeded inputs.

    python tests/golden/gen_goldens_cc.py

Needs the reference checkout (see gen_goldens.py); nothing of it is copied into the repository, only numbers.
Inputs are stored quantised (images as uint8 / 255, maps as uint16 / 65535, logits and features as int8 / scale):
exact in f32, a fraction of the size; `tests/cc_fixture.decode()` rebuilds them here and in tests/test_gpu_cc.py.
The f64 yardsticks are stored rounded to f32; the reference's own f32-to-f64 distances `e_ref` are computed here in
full precision: per case [2-norm, element-wise max, loss], relative as in the tolerance rule of the tests.
"""
import sys
import types
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import gen_goldens as gg  # noqa: E402
from cc_fixture import decode, softmax_f32  # noqa: E402

OUT = Path(__file__).resolve().parent / "cc.npz"

gg.STUBS = dict(gg.STUBS)
# the hooks use loguru's `logger.contextualize(...)` as a context manager (ccblock.py:85) and as a decorator (mt.py:251);
# the stub logger of gen_goldens.py returns itself from every call, which is neither: give it one that is both
gg.STUBS["loguru/__init__.py"] = (
    "import contextlib\n"
    "class _Ctx(contextlib.ContextDecorator):\n"
    "    def __enter__(self):\n"
    "        return self\n"
    "    def __exit__(self, *exc):\n"
    "        return False\n"
    "class _L:\n"
    "    def __getattr__(self, k):\n"
    "        return lambda *a, **k2: self\n"
    "    def catch(self, *a, **k):\n"
    "        return lambda fn: fn\n"
    "    def contextualize(self, *a, **k):\n"
    "        return _Ctx()\n"
    "    def __call__(self, fn=None, *a, **k):\n"
    "        return fn\n"
    "logger = _L()\n")


def smooth(gen, n, c, h, w, k=5):
    x = torch.rand(n, c, h + k - 1, w + k - 1, generator=gen)
    return torch.nn.functional.avg_pool2d(x, k, stride=1)


def unit(x):
    lo, hi = x.amin(dim=(1, 2, 3), keepdim=True), x.amax(dim=(1, 2, 3), keepdim=True)
    return (x - lo) / (hi - lo)


def rel(a32, a64):
    d = (a32.double() - a64).flatten()
    return [float(d.norm() / a64.norm()), float(d.abs().max() / a64.abs().max())]


def leaf(t, dt):
    return t.detach().to(dt).clone().requires_grad_(True)


def f32(t):
    return t.detach().to(torch.float32).numpy()


def main():
    scratch = gg.setup_reference()
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = type("SummaryWriter", (), {})
    sys.modules["torch.utils.tensorboard"] = tb
    from contrastyou.losses.cross_correlation import CCLoss
    from contrastyou.projectors.heads import CrossCorrelationProjector
    from semi_seg.hooks import cc as ref_cc
    from semi_seg.hooks import ccblock as ref_ccblock

    out = {}
    table = []

    # ------------------------------------------------------------------ (a) CCLoss alone
    gen = torch.Generator().manual_seed(301)
    I = unit(smooth(gen, 4, 1, 56, 56, 5))
    J = unit(0.6 * I + 0.4 * smooth(gen, 4, 1, 56, 56, 3)).pow(0.75)
    out["a_I_u16"] = (I * 65535).round().numpy().astype(np.uint16)
    out["a_J_u16"] = (J * 65535).round().numpy().astype(np.uint16)
    I, J = decode("a_I_u16", out["a_I_u16"]), decode("a_J_u16", out["a_J_u16"])
    for win in (3, 5, 7, 9):
        res = {}
        for dt in (torch.float32, torch.float64):
            crit = CCLoss(win=(win, win)).to(dt)
            i_, j_ = leaf(I, dt), leaf(J, dt)
            loss = crit(i_, j_)
            loss.backward()
            res[dt] = (loss.detach(), i_.grad, j_.grad)
        l32, gi32, gj32 = res[torch.float32]
        l64, gi64, gj64 = res[torch.float64]
        ei, ej = rel(gi32, gi64), rel(gj32, gj64)
        e = [max(ei[0], ej[0]), max(ei[1], ej[1]), float(abs(l32.double() - l64) / abs(l64))]
        out[f"a{win}_loss32"], out[f"a{win}_loss64"] = np.float32(l32), np.float64(l64)
        out[f"a{win}_gI64"], out[f"a{win}_gJ64"] = f32(gi64), f32(gj64)
        out[f"a{win}_e_ref"] = np.array(e)
        table.append((f"a win {win}", e))

    # ------------------------------------------------------------------ (b), (c) cc_loss_per_head
    gen = torch.Generator().manual_seed(302)
    K, n, S = 5, 2, 56
    logits = (smooth(gen, n, K, S, S, 7) - 0.5) * 60 + torch.randn(n, K, S, S, generator=gen) * 1.5
    lq = logits.mul(4).round().clamp(-128, 127).to(torch.int8)
    lq[0, :, 8:24, :] = -128  # a flat background band: saturated prediction ...
    lq[0, 0, 8:24, :] = 127
    out["bc_logits_i8d4"] = lq.numpy()
    img112 = unit(smooth(gen, n, 1, 112, 112, 5) + 0.3 * smooth(gen, n, 1, 112, 112, 2))
    img112[0, :, 16:48, :] = 0  # ... under a band of image 0 (56 x 56: rows 8..24)
    img56 = torch.nn.functional.avg_pool2d(img112, 2)
    out["bc_img112_u8"] = (img112 * 255).round().numpy().astype(np.uint8)
    out["bc_img56_u8"] = (img56 * 255).round().numpy().astype(np.uint8)
    prob = softmax_f32(decode("bc_logits_i8d4", out["bc_logits_i8d4"]))
    imgs = {56: decode("bc_img56_u8", out["bc_img56_u8"]), 112: decode("bc_img112_u8", out["bc_img112_u8"])}

    def block_head(power, win, dt):
        h = ref_ccblock._CrossCorrelationHook(weight=1.0, kernel_size=win, diff_power=power)
        h.criterion.to(dt)
        return h.cc_loss_per_head

    def logit_head(power, win, dt):
        h = ref_cc._CrossCorrelationLogitEpocherHook(
            cc_criterion=CCLoss(win=(win, win)).to(dt), mi_criterion=None, cc_weight=1.0, mi_weight=0.0,
            diff_power=power, saver=None)
        return h.cc_loss_per_head

    cases = [("b0", block_head, 0.75, 5, 56), ("b1", block_head, 1.0, 7, 112), ("c0", logit_head, 0.75, 5, 112)]
    out["bc_cases"] = np.array([[p, w, s] for _, _, p, w, s in cases])
    for tag, make, power, win, size in cases:
        res = {}
        for dt in (torch.float32, torch.float64):
            p_ = leaf(prob, dt)
            loss, diff_image, diff_pred = make(power, win, dt)(image=imgs[size].to(dt), predict_simplex=p_)
            loss.backward()
            res[dt] = (loss.detach(), p_.grad, diff_image.detach(), diff_pred.detach())
        l32, g32, _, _ = res[torch.float32]
        l64, g64, di64, dp64 = res[torch.float64]
        e = rel(g32, g64) + [float(abs(l32.double() - l64) / abs(l64))]
        out[f"{tag}_loss32"], out[f"{tag}_loss64"] = np.float32(l32), np.float64(l64)
        out[f"{tag}_g64"] = f32(g64)
        out[f"{tag}_e_ref"] = np.array(e)
        if tag == "b0":  # (the maps of one case: they are 25 KB each)
            out[f"{tag}_diff_image64"], out[f"{tag}_diff_pred64"] = f32(di64), f32(dp64)
        table.append((f"{tag} power {power} win {win} image {size}", e))

    # ------------------------------------------------------------------ (d) CrossCorrelationProjector
    gen = torch.Generator().manual_seed(303)
    feat = torch.randn(2, 16, 12, 10, generator=gen).mul(32).round().clamp(-128, 127).to(torch.int8)
    out["d_feat_i8d32"] = feat.numpy()
    x = decode("d_feat_i8d32", out["d_feat_i8d32"])
    for head_type in ("linear", "mlp"):
        head = CrossCorrelationProjector(input_dim=16, num_clusters=6, head_type=head_type, normalize=False,
                                         num_subheads=2, hidden_dim=24)
        sd = {k: torch.randn(v.shape, generator=gen) * 0.3 for k, v in head.state_dict().items()}
        head.load_state_dict(sd, strict=True)
        out[f"d_{head_type}_names"] = np.array(sorted(sd))
        coefs = [torch.randn(2, 6, 12, 10, generator=gen) for _ in range(2)]
        xi = x.clone().requires_grad_(True)
        probs = head(xi)
        sum((p * c).sum() for p, c in zip(probs, coefs)).backward()
        for k, v in sd.items():
            out[f"d_{head_type}_w_{k}"] = f32(v)
        for i in range(2):
            out[f"d_{head_type}_prob{i}"], out[f"d_{head_type}_coef{i}"] = f32(probs[i]), f32(coefs[i])
        out[f"d_{head_type}_dx"] = f32(xi.grad)
        for k, p in head.named_parameters():
            out[f"d_{head_type}_g_{k}"] = f32(p.grad)

    # ------------------------------------------------------------------ (e) composed epocher hook: cc + mi + rr
    gen = torch.Generator().manual_seed(304)
    n_unl, C, hw = 2, 16, 12
    feats = smooth(gen, 2 * n_unl, C, hw, hw, 3).sub(0.5).mul(6).add(torch.randn(2 * n_unl, C, hw, hw, generator=gen))
    out["e_feat_i8d32"] = feats.mul(32).round().clamp(-128, 127).to(torch.int8).numpy()
    eimg = unit(smooth(gen, n_unl, 1, 24, 24, 3))
    out["e_img_u8"] = (eimg * 255).round().numpy().astype(np.uint8)
    feats, eimg = decode("e_feat_i8d32", out["e_feat_i8d32"]), decode("e_img_u8", out["e_img_u8"])
    proj = CrossCorrelationProjector(input_dim=C, num_clusters=6, head_type="linear", normalize=False, num_subheads=2)
    sd = {k: torch.randn(v.shape, generator=gen) * 0.5 for k, v in proj.state_dict().items()}
    for k, v in sd.items():
        out[f"e_w_{k}"] = f32(v)
    params = {"cc": dict(weight=1.0, kernel_size=3, diff_power=0.75), "mi": dict(weight=0.1, lamda=1.5, padding=0),
              "rr": dict(weight=0.1, alpha=0.5)}
    out["e_params"] = np.array([1.0, 3, 0.75, 0.1, 1.5, 0, 0.1, 0.5])

    class Tap:
        def __init__(self, f):
            self.f = f

        def bind(self):
            pass

        def feature(self):
            return self.f

    res = {}
    for dt in (torch.float32, torch.float64):
        proj.load_state_dict(sd, strict=True)
        p_ = proj.to(dt)
        for q in p_.parameters():
            q.grad = None
        f_ = leaf(feats, dt)
        cch = ref_ccblock._CrossCorrelationHook(**params["cc"])
        cch.criterion.to(dt)
        tiny = [ref_ccblock._MIHook(**params["mi"]), cch, ref_ccblock._RedundancyReduction(**params["rr"])]
        hook = ref_ccblock._ProjectorEpocherGeneralHook(name="e", extractor=Tap(f_), projector=p_, dist_hooks=tiny)
        hook._epocher, hook._epocher_init = types.SimpleNamespace(cur_epoch=1, cur_batch_num=1), True
        loss = hook._call_implementation(
            unlabeled_image_tf=eimg.to(dt), unlabeled_logits_tf=torch.zeros(n_unl, 1), affine_transformer=lambda t: t,
            unlabeled_image=eimg.to(dt), seed=1)
        loss.backward()
        res[dt] = (loss.detach(), f_.grad, {k: q.grad.clone() for k, q in p_.named_parameters()})
    l32, g32, pg32 = res[torch.float32]
    l64, g64, pg64 = res[torch.float64]
    e = rel(g32, g64)
    for k in pg64:
        ek = rel(pg32[k], pg64[k])
        e = [max(e[0], ek[0]), max(e[1], ek[1])]
        out[f"e_g64_{k}"] = f32(pg64[k])
    e.append(float(abs(l32.double() - l64) / abs(l64)))
    out["e_loss32"], out["e_loss64"], out["e_gfeat64"], out["e_e_ref"] = np.float32(l32), np.float64(l64), f32(g64), \
        np.array(e)
    table.append(("e cc+mi+rr", e))

    # the parameter names create_cross_correlation_hooks2 must reproduce (Up_conv2, linear, 2 sub-heads)
    out["names_linear_2"] = np.array(sorted(
        CrossCorrelationProjector(input_dim=16, num_clusters=10, head_type="linear", normalize=False,
                                  num_subheads=2, hidden_dim=64).state_dict()))
    out["names_mlp_2"] = np.array(sorted(
        CrossCorrelationProjector(input_dim=16, num_clusters=10, head_type="mlp", normalize=False,
                                  num_subheads=2, hidden_dim=64).state_dict()))

    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {OUT.stat().st_size} bytes")
    print("reference f32 vs f64:  case | grad 2-norm | grad max | loss")
    for name, e in table:
        print(f"  {name:34s} | {e[0]:.2e} | {e[1]:.2e} | {e[2]:.2e}")
    del scratch


if __name__ == "__main__":
    main()
