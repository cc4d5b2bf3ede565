"""The supervised criteria on the GPU (csrc/cy_seg_loss.hip: class-weighted KL_div with any reduction, soft DiceLoss)
against tests/golden/criteria.npz / criteria_dice.npz (the reference's KL_div and DiceLoss in f32 and f64,
tests/golden/gen_goldens_criteria.py) and against f64 CPU evaluations written here from the formulas.

Tolerance rule (the one of tests/test_gpu_semi_baselines.py).  The yardstick is the reference's own f32-to-f64 distance
on the fixture's inputs:
    e(x) = |x - x64| relative: 2-norm for gradients, element-wise maximum over max|grad64|, |.| / |loss64| for the loss
    require e_hip <= max(4 * e_ref, 1e-6), e_ref = the largest value over the fixture's cases of the same family
The bound comes from the fixture, never from the code under test.  No pixel is left out of any comparison: these losses
have no arg-max and no threshold.  A "none" reduction is differentiated under an upstream gradient, and its loss figure
is the f64 sum of output * upstream; its output is also compared element-wise, relative to the largest element, under
the loss bound.  Every figure is printed before it is asserted.
"""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from criteria_fixture import ABSENT_CLASS, ABSENT_IMAGE, FILES, SHAPE, decode, dice_cases, kl_cases, kl_weight
from test_gpu_hooks_dice import Loader, blob_batch
from test_gpu_semi_baselines import bound, check, cpu64, gpu_leaf

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-16


@pytest.fixture(scope="module")
def fx(golden_dir):
    data = {}
    for name in FILES.values():
        with np.load(golden_dir / name) as f:
            data.update({k: f[k] for k in f.files})

    class Fx:
        def __getitem__(self, k):
            return data[k]

        def t(self, k):
            return torch.from_numpy(data[k])

        def inputs(self, K):
            """-> logits f32 [N, K, H, W], labels int64 [N, H, W], upstream map [N, H, W], upstream vector [N]"""
            return (decode(f"K{K}_z_i8d8", data[f"K{K}_z_i8d8"]), torch.from_numpy(data[f"K{K}_y"]).long(),
                    self.t(f"K{K}_upmap"), self.t(f"K{K}_upvec"))

        def e_ref(self, family):
            """[2-norm, max, loss]: the largest over the fixture's cases of this family ("kl", "dice")"""
            rows = [data[k] for k in data if k.endswith("_e_ref") and k.startswith(family)]
            assert rows, family
            return np.max(np.stack(rows), axis=0)

    return Fx()


# ---------------------------------------------------------------------------------------------- f64 formulas (CPU)
def kl64(z, y, w, reduction, eps=EPS):
    """l = -w[y] log((p_y + eps) / (1 + eps)); w: the normalised weights as the kernels read them (f32), or None"""
    p = z.softmax(1)
    py = p.gather(1, y[:, None])[:, 0]
    wy = 1.0 if w is None else w.double()[y]
    l = -wy * torch.log((py + eps) / (1 + eps))
    return {"mean": l.mean, "sum": l.sum, "none": lambda: l}[reduction]()


def dice64(z, y, *, smooth=1.0, p=2, ignore_index=None, reduction="mean"):
    """per image n and class c: A = sum p_c [y = c], B = sum p_c^P, T = #[y = c]; L = 1 - (A + s) / (B + T + s);
    (1 / K) sum_{c != ignore} red_n L_nc"""
    K = z.shape[1]
    pr = z.softmax(1)
    onehot = F.one_hot(y, K).movedim(-1, 1).to(z.dtype)
    A, B, T = (pr * onehot).flatten(2).sum(2), (pr ** p).flatten(2).sum(2), onehot.flatten(2).sum(2)
    L = 1 - (A + smooth) / (B + T + smooth)
    keep = [c for c in range(K) if c != ignore_index]
    Ln = L[:, keep].sum(1) / K
    return {"mean": Ln.mean, "sum": Ln.sum, "none": lambda: Ln}[reduction]()


def eval64(fn, z, up=None):
    """-> (figure, dfigure/dz, output) of an f64 formula; figure = the loss, or sum(output * up)"""
    z = z.double().requires_grad_(True)
    out = fn(z)
    fig = out if out.dim() == 0 else (out * up.double()).sum()
    fig.backward()
    return fig.detach(), z.grad, out.detach()


def normalised(w):
    """kl.py:104-108, in f32"""
    w = torch.tensor(w).float()
    return w / w.sum() * len(w)


def figure(out, up):
    """the loss figure of a device output, in f64 on the CPU"""
    out = cpu64(out)
    return out if out.dim() == 0 else (out * up.double()).sum()


def check_output(what, out, out64, e_ref_loss):
    """a "none" output element-wise: each element is one f32 evaluation of the loss formula"""
    got, want = cpu64(out), cpu64(out64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    e = float((got - want).abs().max() / want.abs().max())
    print(f"{what}: output e_max {e:.2e} (bound {bound(e_ref_loss):.2e})")
    assert e <= bound(e_ref_loss), (what, e)


# --------------------------------------------------------------------------------- 0. the restatement, on the fixture
def test_the_f64_restatement_equals_the_reference(fx):
    """kl64 / dice64 above are what the shapes outside the fixture are compared with: on the fixture they give the
    reference's f64 numbers (the gradient is stored rounded to f32: half an ulp of its largest entry per element)"""
    worst = [0.0, 0.0]
    for key, K, tag, red in kl_cases():
        z, y, upmap, _ = fx.inputs(K)
        l, g, _ = eval64(lambda t: kl64(t, y, normalised(kl_weight(K, tag)), red), z, upmap)
        worst = _held(key, l, g, fx, worst)
    for key, K, kw in dice_cases():
        z, y, _, upvec = fx.inputs(K)
        l, g, _ = eval64(lambda t: dice64(t, y, **kw), z, upvec)
        worst = _held(key, l, g, fx, worst)
    print(f"restatement vs reference f64: loss {worst[0]:.2e}, gradient {worst[1]:.2e} of its largest entry")


def _held(key, l, g, fx, worst):
    e_l = abs(float(l) - float(fx[f"{key}_loss64"])) / abs(float(fx[f"{key}_loss64"]))
    g64 = fx.t(f"{key}_g64").double()
    e_g = float((g - g64).abs().max() / g64.abs().max())
    assert e_l <= 1e-13, (key, e_l)          # the same f64 operations in another order
    assert e_g <= 2.0 ** -24, (key, e_g)     # f32 rounding of the stored gradient
    return [max(worst[0], e_l), max(worst[1], e_g)]


# ---------------------------------------------------------------------------------------------- 1. the fixture
def _kl_through_ops(z, y, w, red, up):
    from cyhip import ops
    zd, yd = ops.to_nhwc(z.to(DEV)), y.to(DEV)
    wd = None if w is None else w.to(DEV)
    out = ops.softmax_wkl_fwd(zd, yd, wd, EPS, red)
    upd = up.to(DEV).contiguous() if red == "none" else torch.ones(1, device=DEV)
    return out, ops.softmax_wkl_bwd(zd, yd, wd, upd, EPS, red)


def _dice_through_ops(z, y, kw, up):
    from cyhip import ops
    zd, yd = ops.to_nhwc(z.to(DEV)), y.to(DEV)
    red = kw.get("reduction", "mean")
    args = (kw.get("p", 2), kw.get("smooth", 1.0), kw.get("ignore_index"))
    out, table = ops.softmax_dice_fwd(zd, yd, *args, red)
    upd = up.to(DEV).contiguous() if red == "none" else torch.ones(1, device=DEV)
    return out, ops.softmax_dice_bwd(zd, yd, table, upd, args[0], args[2], red), table


def _through_module(crit, z, y, up):
    zl = gpu_leaf(z)
    out = crit.from_logits(zl, y.to(DEV))
    (out if out.dim() == 0 else (out * up.to(DEV)).sum()).backward()
    return out.detach(), zl.grad


@pytest.mark.parametrize("key,K,tag,red", kl_cases(), ids=[c[0] for c in kl_cases()])
def test_weighted_kl_against_the_reference(fx, key, K, tag, red):
    from contrastyou.losses.kl import KL_div
    z, y, upmap, _ = fx.inputs(K)
    crit = KL_div(reduction=red, weight=kl_weight(K, tag))
    assert torch.equal(crit._weight, normalised(kl_weight(K, tag)))
    e_ref = fx.e_ref("kl")
    for how, (out, grad) in (("ops", _kl_through_ops(z, y, crit._weight, red, upmap)),
                             ("KL_div.from_logits", _through_module(crit, z, y, upmap))):
        assert out.shape == (SHAPE if red == "none" else ())
        check(f"{key} {how}", figure(out, upmap), fx[f"{key}_loss64"], grad, fx.t(f"{key}_g64"), e_ref)
        if red == "none":
            check_output(f"{key} {how}", out, fx.t(f"{key}_out64"), e_ref[2])
    if tag == "zero":  # a class of weight 0: its pixels cost nothing and push nothing, exactly
        off = (y == K // 2)
        assert off.any() and (cpu64(grad).movedim(1, -1)[off] == 0).all()
        if red == "none":
            assert (cpu64(out)[off] == 0).all()


@pytest.mark.parametrize("key,K,kw", dice_cases(), ids=[c[0] for c in dice_cases()])
def test_dice_against_the_reference(fx, key, K, kw):
    from contrastyou.losses.dice_loss import DiceLoss
    z, y, _, upvec = fx.inputs(K)
    assert not (y[ABSENT_IMAGE] == ABSENT_CLASS).any() and (y[0] == ABSENT_CLASS).any()  # T = 0 in image 2 only
    red = kw.get("reduction", "mean")
    e_ref = fx.e_ref("dice")
    out, grad, table = _dice_through_ops(z, y, kw, upvec)
    results = (("ops", (out, grad)), ("DiceLoss.from_logits", _through_module(DiceLoss(**kw), z, y, upvec)))
    for how, (out, grad) in results:
        assert out.shape == ((SHAPE[0],) if red == "none" else ())
        check(f"{key} {how}", figure(out, upvec), fx[f"{key}_loss64"], grad, fx.t(f"{key}_g64"), e_ref)
        if red == "none":
            check_output(f"{key} {how}", out, fx.t(f"{key}_out64"), e_ref[2])
    # the table the backward reads: num = A + smooth, den = B + T + smooth, the ignored class included
    smooth, P = kw.get("smooth", 1.0), kw.get("p", 2)
    pr, onehot = z.double().softmax(1), F.one_hot(y, K).movedim(-1, 1).double()
    num = (pr * onehot).flatten(2).sum(2) + smooth
    den = (pr ** P).flatten(2).sum(2) + onehot.flatten(2).sum(2) + smooth
    want = torch.stack([num, den], -1)
    e = float(((table.cpu() - want).abs() / want).max())
    print(f"{key}: table e_max {e:.2e} (bound {bound(e_ref[2]):.2e})")
    assert table.dtype == torch.float64 and table.shape == (SHAPE[0], K, 2) and e <= bound(e_ref[2])
    assert float(table[ABSENT_IMAGE, ABSENT_CLASS, 0]) == smooth  # A = 0 exactly where the class is absent


# ------------------------------------------------------------------------------ 2. the unweighted mean keeps its path
def test_unweighted_mean_kl_div_is_still_softmax_kl(fx, monkeypatch):
    from contrastyou.losses.kl import KL_div
    from cyhip import _lib
    from cyhip.functions import SoftmaxKLFn
    z, y, _, _ = fx.inputs(4)
    za, zb = gpu_leaf(z), gpu_leaf(z)
    want = SoftmaxKLFn.apply(za, y.to(DEV), EPS)
    (3.0 * want).backward()
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    got = KL_div().from_logits(zb, y.to(DEV))
    (3.0 * got).backward()
    monkeypatch.undo()
    assert calls == ["cy_softmax_kl_fwd", "cy_softmax_kl_bwd"], calls
    assert torch.equal(got.detach(), want.detach()) and torch.equal(za.grad, zb.grad)


def test_every_other_configuration_runs_the_new_kernels(fx, monkeypatch):
    """one forward entry and one backward entry per call, nothing else of the library, and no host round trip"""
    from contrastyou.losses.dice_loss import DiceLoss
    from contrastyou.losses.kl import KL_div
    from cyhip import _lib
    z, y, upmap, upvec = fx.inputs(5)
    yd, upmap, upvec = y.to(DEV), upmap.to(DEV), upvec.to(DEV)
    crits = [(KL_div(weight=kl_weight(5, "ramp")), "wkl", "wkl"), (KL_div(reduction="sum"), "wkl", "wkl"),
             (KL_div(reduction="none"), "wkl_map", "wkl_map"), (DiceLoss(ignore_index=0), "dice", "dice"),
             (DiceLoss(reduction="none", p=1), "dice", "dice")]
    for crit, fwd, bwd in crits:
        crit.from_logits(gpu_leaf(z), yd)  # (the first call uploads the class weights)
        zl = gpu_leaf(z)
        torch.cuda.synchronize()
        calls, real = [], _lib.call
        monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = crit.from_logits(zl, yd)
            (out if out.dim() == 0 else (out * (upmap if out.dim() == 3 else upvec)).sum()).backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
            monkeypatch.undo()
        assert calls == [f"cy_softmax_{fwd}_fwd", f"cy_softmax_{bwd}_bwd"], (crit, calls)
        assert torch.isfinite(zl.grad).all().item()


# ---------------------------------------------------------------------------------- 3. tail and boundary shapes
def _labels(gen, n, K, H, W):
    """random labels; the last image of a batch never holds class K - 1 (images differ in what they hold)"""
    y = torch.randint(0, K, (n, H, W), generator=gen)
    if n > 1 and K > 1:
        y[-1] = torch.where(y[-1] == K - 1, torch.zeros_like(y[-1]), y[-1])
    return y


CONFIGS = [("kl", dict(reduction="mean", weight="ramp")), ("kl", dict(reduction="sum")),
           ("kl", dict(reduction="none", weight="zero")), ("dice", dict()), ("dice", dict(reduction="sum", smooth=1e-5)),
           ("dice", dict(reduction="none", p=1, ignore_index=0))]


def _against_f64(what, fx, z, y, gen):
    from contrastyou.losses.dice_loss import DiceLoss
    from contrastyou.losses.kl import KL_div
    n, K, H, W = z.shape
    upmap, upvec = torch.rand(n, H, W, generator=gen) + 0.5, torch.rand(n, generator=gen) + 0.5
    for family, kw in CONFIGS:
        if family == "kl":
            w = kl_weight(K, kw["weight"]) if "weight" in kw else None
            crit = KL_div(reduction=kw["reduction"], weight=w)
            fn, up = (lambda t: kl64(t, y, crit._weight, kw["reduction"])), upmap
        else:
            crit = DiceLoss(**kw)
            fn, up = (lambda t: dice64(t, y, **kw)), upvec
        out, grad = _through_module(crit, z, y, up)
        l64, g64, out64 = eval64(fn, z, up)
        check(f"{what} {family} {kw}", figure(out, up), l64, grad, g64, fx.e_ref(family))
        if out.dim():
            check_output(f"{what} {family} {kw}", out, out64, fx.e_ref(family)[2])


@pytest.mark.parametrize("n,K,H,W", [
    (1, 4, 11, 13),      # N = 1, HW = 143: less than one block; 16-byte rows
    (2, 5, 16, 16),      # HW = 256: exactly one block per image, two different images; the run-time-K kernels
    (2, 8, 1, 257),      # HW = 257: one block and one pixel; two 16-byte accesses per row
    (3, 2, 257, 1),      # ... 8-byte rows; an image that is not square
    (1, 16, 17, 19),     # the widest row
    (1, 3, 16, 16),      # N = 1 at exactly one block
])
def test_tail_and_boundary_shapes_against_f64_formulas(fx, n, K, H, W):
    gen = torch.Generator().manual_seed(100 * K + H)
    z = torch.randn(n, K, H, W, generator=gen) * (torch.rand(n, 1, H, W, generator=gen) * 3)
    _against_f64(f"{n}x{K}x{H}x{W}", fx, z, _labels(gen, n, K, H, W), gen)


def test_past_every_capped_grid(fx):
    """N = 2, 363 x 363, K = 4: 263 538 pixels > 1024 blocks x 256 (the grid-stride loops of the KL kernels go round
    again) and 131 769 pixels per image > 512 blocks x 256 (so do the Dice kernels' loops, within each image)"""
    gen = torch.Generator().manual_seed(363)
    z = torch.randn(2, 4, 363, 363, generator=gen) * (torch.rand(2, 1, 363, 363, generator=gen) * 3)
    _against_f64("2x4x363x363", fx, z, _labels(gen, 2, 4, 363, 363), gen)


def test_saturated_logits(fx):
    """logits of +-80: p_y = 0 exactly where the label's logit lost; log(0 + eps) is finite, nothing is NaN"""
    gen = torch.Generator().manual_seed(80)
    z = torch.where(torch.rand(2, 4, 19, 23, generator=gen) < 0.4, 80.0, -80.0)
    y = _labels(gen, 2, 4, 19, 23)
    assert (z.softmax(1).gather(1, y[:, None]) == 0).any()
    _against_f64("saturated", fx, z, y, gen)


# ---------------------------------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("n,K,H,W", [(2, 4, 363, 363), (3, 5, 19, 19)])
def test_two_runs_give_the_same_bits(n, K, H, W):
    gen = torch.Generator().manual_seed(7)
    z, y = torch.randn(n, K, H, W, generator=gen) * 2, _labels(gen, n, K, H, W)
    upmap, upvec = torch.rand(n, H, W, generator=gen), torch.rand(n, generator=gen)
    w = normalised(kl_weight(K, "ramp"))
    runs = []
    for _ in range(2):
        got = []
        for red in ("mean", "none"):
            got += [t.cpu() for t in _kl_through_ops(z, y, w, red, upmap)]
            got += [t.cpu() for t in _dice_through_ops(z, y, dict(reduction=red), upvec)]
        runs.append(got)
    assert len(runs[0]) == 10
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- 5. step level
def _criterion(name):
    from contrastyou.losses.dice_loss import DiceLoss
    from contrastyou.losses.kl import KL_div
    return DiceLoss(ignore_index=0) if name == "dice" else KL_div(weight=[1, 2, 2, 2])


def _trainer_run(name, tmp_path, *, graph, bf16, steps, K=4):
    """one epoch of `steps` steps of trainer_zoo["semi"] on the 128-channel toy under an entropy-minimisation hook, then
    one evaluation pass -> (training metrics, evaluation metrics, [(logits, labels, loss)] as the criterion saw them,
    the model, whether the passes were replayed from a graph)"""
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from cyhip import graphed
    from oracle import unet as ou
    from semi_seg.hooks import create_ent_min_hook
    from semi_seg.trainers import trainer_zoo
    tmp_path.mkdir(parents=True, exist_ok=True)
    default = graphed.GRAPH_STEP
    graphed.GRAPH_STEP = graph
    try:
        type(TrainerHook).names.clear()
        g = torch.Generator().manual_seed(21)
        lab, unl = [blob_batch(4, 32, K, g) for _ in range(steps)], [blob_batch(4, 32, K, g) for _ in range(steps)]
        val = [{k: v[0] for k, v in blob_batch(2, 32, K, g, views=1).items()}]
        cfg = {"Optim": {"name": "RAdam", "lr": 3e-3, "weight_decay": 1e-4}, "Trainer": {"name": "semi"}}
        model = UNet(input_dim=1, num_classes=K, max_channel=128, momentum=0.1)
        model.load_state_dict(ou.init_state_dict(1, K, 128, seed=14))
        crit, seen = _criterion(name), []
        inner = crit.from_logits

        def spy(logits, labels):
            loss = inner(logits, labels)
            seen.append((logits.detach().float().cpu(), labels.detach().cpu(), loss.detach().float().cpu()))
            return loss

        crit.from_logits = spy
        tr = trainer_zoo["semi"](model=model, labeled_loader=Loader(lab), unlabeled_loader=Loader(unl),
                                 val_loader=Loader(val), test_loader=Loader(val), criterion=crit,
                                 save_dir=str(tmp_path), max_epoch=1, num_batches=steps, device=DEV, disable_bn=False,
                                 two_stage=True, config=cfg, enable_scale=bf16)
        random.seed(9)
        with tr.register_hook(create_ent_min_hook(weight=0.5)):
            tr.init()
            tr.to(DEV)
            train = tr.tra_epoch()
            evaluation, _ = tr.eval_epoch(model=tr.inference_model, loader=tr._val_loader)
        torch.cuda.synchronize()
        replayed = any(isinstance(v, graphed.GraphedTwoPass) for v in model.__dict__.get("_cy_graphed", {}).values())
        return train, evaluation, seen, model, replayed
    finally:
        graphed.GRAPH_STEP = default
        type(TrainerHook).names.clear()


@pytest.mark.parametrize("name", ["dice", "kl"])
def test_a_trainer_step_under_the_criterion(fx, tmp_path, name):
    train, evaluation, seen, model, _ = _trainer_run(name, tmp_path, graph=False, bf16=False, steps=1)
    assert len(seen) == 2  # the training step and the evaluation batch, both through from_logits
    crit = _criterion(name)
    e_ref = fx.e_ref(name)[2]
    for what, (logits, labels, loss), reported in (("sup_loss", seen[0], train["semi"]["sup_loss"]),
                                                   ("eval loss", seen[1], evaluation["eval"]["loss"])):
        K = logits.shape[1]
        want = float(crit(logits.double().softmax(1), F.one_hot(labels, K).movedim(-1, 1).double()))
        e = abs(float(loss) - want) / abs(want)
        print(f"{name} {what}: fused {float(loss):.9g}, torch-ops forward in f64 {want:.9g}, e {e:.2e} "
              f"(bound {bound(e_ref):.2e}); reported {reported:.9g}")
        assert e <= bound(e_ref), (what, e)
        assert abs(reported - float(loss)) <= 1e-7 * abs(float(loss)), (what, reported, float(loss))
    grads = [p.grad for p in model.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
    assert np.isfinite(train["semi"]["reg_loss"]) and train["semi"]["reg_loss"] != 0


@pytest.mark.parametrize("name", ["dice", "kl"])
def test_graph_replayed_steps_report_what_eager_steps_report(tmp_path, name):
    """four steps either way: the criterion runs in the eager section after the replayed forward passes"""
    m_e, ev_e, _, _, rep_e = _trainer_run(name, tmp_path / "eager", graph=False, bf16=True, steps=4)
    m_g, ev_g, _, _, rep_g = _trainer_run(name, tmp_path / "graph", graph=True, bf16=True, steps=4)
    assert rep_g and not rep_e, "the second run must have captured and replayed the passes"
    print(name, "eager", m_e["semi"], "graph", m_g["semi"])
    assert np.isfinite(m_e["semi"]["sup_loss"]) and np.isfinite(m_e["semi"]["reg_loss"])
    assert m_e["semi"]["sup_loss"] == m_g["semi"]["sup_loss"]
    assert m_e["semi"]["reg_loss"] == m_g["semi"]["reg_loss"]
    assert ev_e["eval"]["loss"] == ev_g["eval"]["loss"]
