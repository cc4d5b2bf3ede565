"""Multi-prototype ("multicore") training on the GPU: the grouped softmax-KL and Dice kernels, the softmax-MSE at
16 < K <= 64 (csrc/cy_group_loss.hip), `MultiCoreKL`, the epochers and the trainer, against tests/golden/multicore.npz
(the reference's MultiCoreKL and consistency hook in f32 and f64, tests/golden/gen_goldens_multicore.py).

Tolerance rule (the one of tests/test_gpu_cc.py and tests/test_gpu_semi_baselines.py).  The yardstick is the reference's
own f32-to-f64 distance on the fixture's inputs:
    e(x) = |x - x64| relative: 2-norm for gradients, element-wise maximum over max|grad64|, |.| / |loss64| for the loss
    require e_hip <= max(4 * e_ref, 1e-6), e_ref = the largest value over the fixture's cases of the same kind
No pixel is left out of any comparison.  Every figure is printed before it is asserted.
"""
import math
import random

import numpy as np
import pytest
import torch

from multicore_fixture import (BIG, BIG_ROWS, CASES, CONS_KS, SHAPE, big_inputs, decode, groups_of, pixel_rows, tag)
from step_harness import OneBatchLoader
from test_gpu_hooks_dice import blob_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR, FACTOR = 1e-6, 4.0
EPS = 1e-16


@pytest.fixture(scope="module")
def fx(golden_dir):
    data = np.load(golden_dir / "multicore.npz")

    class Fx:
        def __getitem__(self, k):
            return data[k]

        def t(self, k):
            return torch.from_numpy(data[k])

        def dec(self, k):
            return decode(k, data[k])

        def e_ref(self, kind):
            """[2-norm, max, loss]: the largest over the fixture's cases of this kind"""
            rows = [data[k] for k in data.files if k.endswith("_e_ref") and k.startswith(kind)]
            assert rows, kind
            return np.max(np.stack(rows), axis=0)

        def kl_case(self, key):
            """(logits f32 [N,K,H,W], labels int64 [N,H,W]) of a multi-prototype case, on the CPU"""
            if key == "kl_big":
                z, t = big_inputs()
                return torch.from_numpy(z).float() / 8.0, torch.from_numpy(t).long()
            return self.dec(f"{key}_z_i8d8"), self.t(f"{key}_t").long()

    return Fx()


def bound(e_ref):
    return max(FACTOR * float(e_ref), FLOOR)


def cpu64(t):
    return t.detach().double().cpu()


def check(what, loss, loss64, grad, grad64, e_ref):
    loss, loss64 = float(loss.detach()), float(loss64)
    assert math.isfinite(loss), (what, loss)
    e_loss = abs(loss - loss64) / abs(loss64)
    got, g64 = cpu64(grad), cpu64(grad64)
    assert got.shape == g64.shape, (what, got.shape, g64.shape)
    assert torch.isfinite(got).all(), what
    d = got - g64
    e2, emax = float(d.norm() / g64.norm()), float(d.abs().max() / g64.abs().max())
    print(f"{what}: loss {loss:.9g} vs {loss64:.9g}  e_loss {e_loss:.2e} (bound {bound(e_ref[2]):.2e})  "
          f"grad e_2 {e2:.2e} (bound {bound(e_ref[0]):.2e})  e_max {emax:.2e} (bound {bound(e_ref[1]):.2e})")
    figures = (("loss", e_loss, e_ref[2]), ("e_2", e2, e_ref[0]), ("e_max", emax, e_ref[1]))
    fails = [f"{n} {e:.2e}" for n, e, b in figures if e > bound(b)]
    assert not fails, f"{what}: {fails}"


def gpu_leaf(t):
    return t.float().to(DEV).requires_grad_(True)


def group_kl(z, t, G, eps=EPS):
    """-> (loss, dloss/dz) of SoftmaxGroupKLFn on the device"""
    from cyhip.functions import SoftmaxGroupKLFn
    zz = gpu_leaf(z)
    loss = SoftmaxGroupKLFn.apply(zz, t.to(DEV), G, eps)
    loss.backward()
    return loss.detach(), zz.grad


def multicore64(z, t, C, m):
    """f64 CPU evaluation of the formula: -> (loss, dloss/dz, reduced arg-max)"""
    zz = z.double().requires_grad_(True)
    red = zz.softmax(1).unflatten(1, (C, m)).sum(2)
    onehot = torch.nn.functional.one_hot(t, C).movedim(-1, 1).double()
    loss = -(onehot * torch.log((red + EPS) / (onehot + EPS))).sum(1).mean()
    loss.backward()
    return loss.detach(), zz.grad, red.detach().argmax(1)


def counts_of(pred, target, C):
    """int64 [N, C, 2] (intersection, union) of class maps [N, H, W], as UniversalDice counts them"""
    po = torch.nn.functional.one_hot(pred.long(), C).movedim(-1, 1)
    to = torch.nn.functional.one_hot(target.long(), C).movedim(-1, 1)
    return torch.stack([(po * to).sum((2, 3)), (po + to).sum((2, 3))], dim=-1)


KEYS = [tag(C, m) for C, m in CASES] + ["kl_big"]
SHAPES = {**{tag(C, m): (C, m) for C, m in CASES}, "kl_big": BIG[:2]}


# ------------------------------------------------------------------------------------- 1. loss and gradient
@pytest.mark.parametrize("key", KEYS)
def test_group_kl_against_the_reference(fx, key):
    C, m = SHAPES[key]
    z, t = fx.kl_case(key)
    assert z.shape[1] == C * m
    loss, grad = group_kl(z, t, C)
    e_ref = fx.e_ref("kl_")
    if key == "kl_big":
        # every pixel against the f64 formula, the stored rows against the reference
        l64, g64, _ = multicore64(z, t, C, m)
        assert abs(float(l64) - float(fx[f"{key}_loss64"])) <= 1e-12 * abs(float(l64))
        check(f"{key} (formula, every pixel)", loss, l64, grad, g64, e_ref)
        check(f"{key} (reference, stored rows)", loss, fx[f"{key}_loss64"], pixel_rows(grad.cpu(), BIG_ROWS),
              fx.t(f"{key}_g64"), e_ref)
    else:
        check(key, loss, fx[f"{key}_loss64"], grad, fx.t(f"{key}_g64"), e_ref)
    loss2, grad2 = group_kl(z, t, C)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2), f"{key}: two runs differ"


def test_group_kl_scales_with_the_upstream_gradient(fx):
    from cyhip.functions import SoftmaxGroupKLFn
    z, t = fx.kl_case("kl_c3m7")
    _, g1 = group_kl(z, t, 3)
    zz = gpu_leaf(z)
    (SoftmaxGroupKLFn.apply(zz, t.to(DEV), 3, EPS) * 2.5).backward()
    assert torch.allclose(zz.grad, 2.5 * g1, rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------- 2. Dice
@pytest.mark.parametrize("key", KEYS)
def test_group_dice_counts_equal_the_references_arg_max(fx, key):
    from contrastyou.meters import UniversalDice
    C, m = SHAPES[key]
    z, t = fx.kl_case(key)
    meter = UniversalDice(C, report_axis=list(range(1, C)))
    meter.add_logits(z.to(DEV), t.unsqueeze(1).to(DEV), groups=C)
    (counts, names), = meter._pending
    want = counts_of(fx.t(f"{key}_argmax"), t, C)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (z.shape[0], C, 2)
    assert torch.equal(counts.cpu(), want), key
    # and through the meter: the Dice of the reference's `meters["dice"].add(reduced arg-max, target)`
    ref = UniversalDice(C, report_axis=list(range(1, C)))
    ref.add(fx.t(f"{key}_argmax").long(), t)
    assert meter.summary() == ref.summary()


def test_add_logits_without_groups_is_unchanged(fx):
    from contrastyou.meters import UniversalDice
    from cyhip import ops
    z, t = fx.kl_case("kl_c4m4")
    meter = UniversalDice(16)
    meter.add_logits(z.to(DEV), t.to(DEV))
    (counts, _), = meter._pending
    assert torch.equal(counts, ops.dice_counts(ops.to_nhwc(z.to(DEV)), t.to(DEV)))
    assert torch.equal(counts.cpu(), counts_of(z.argmax(1), t, 16))
    with pytest.raises(AssertionError):
        meter.add_logits(z.to(DEV), t.to(DEV), groups=4)  # the meter counts 16 classes


# ------------------------------------------------------------------------------------- 3. m = 1
@pytest.mark.parametrize("K", [4, 15, 16])
def test_one_prototype_per_class_equals_the_ungrouped_kernels(fx, K):
    from cyhip import ops
    from cyhip.functions import SoftmaxKLFn
    key = {4: "kl_c4m1", 15: "kl_c3m5", 16: "kl_c4m4"}[K]
    z, _ = fx.kl_case(key)
    z = z.clone()
    z[0, :, 0, :5] = 0.0     # exact ties over every class: the lowest index wins in both kernels
    z[1, 1:3, 2, 7] = 6.5    # a two-way tie at the top
    t = torch.randint(0, K, z.shape[:1] + z.shape[2:], generator=torch.Generator().manual_seed(K))
    zg, tg = ops.to_nhwc(z.to(DEV)), t.to(DEV)
    grouped, plain = ops.group_dice_counts(zg, tg, K), ops.dice_counts(zg, tg)
    assert torch.equal(grouped, plain)
    assert torch.equal(plain.cpu(), counts_of(z.argmax(1), t, K))
    loss, grad = group_kl(z, t, K)
    zz = gpu_leaf(z)
    ref = SoftmaxKLFn.apply(zz, tg, EPS)
    ref.backward()
    l64, g64, _ = multicore64(z, t, K, 1)
    e_ref = fx.e_ref("kl_")
    check(f"K={K} grouped vs f64", loss, l64, grad, g64, e_ref)
    check(f"K={K} SoftmaxKLFn vs f64", ref, l64, zz.grad, g64, e_ref)
    check(f"K={K} grouped vs SoftmaxKLFn", loss, ref.detach().double().cpu(), grad, zz.grad, e_ref)


# ------------------------------------------------------------------------------------- 4. any grouping
def test_any_grouping_composes_in_torch_and_matches_the_fused_path(fx):
    from contrastyou.losses.multicore_loss import MultiCoreKL
    from contrastyou.utils.general import class2one_hot
    z, t = fx.kl_case("kl_c4m4")
    fused_crit = MultiCoreKL(groups_of(4, 4))
    assert fused_crit.fusable(16)
    zf = gpu_leaf(z)
    fused = fused_crit.from_logits(zf, t.to(DEV))
    fused.backward()
    # the same partition written class by class in another order of members: not the contiguous pattern -> torch ops
    shuffled = [[3, 1, 0, 2], [5, 4, 7, 6], [8, 10, 9, 11], [15, 14, 13, 12]]
    crit = MultiCoreKL(shuffled)
    assert not crit.fusable(16)
    zc = gpu_leaf(z)
    composed = crit.from_logits(zc, t.to(DEV))
    composed.backward()
    zp = gpu_leaf(z)
    prob = fused_crit(zp.softmax(1), class2one_hot(t.to(DEV), 4))
    prob.backward()
    for what, loss, leaf in (("composed", composed, zc), ("probability space", prob, zp)):
        e_l = abs(float(loss) - float(fused)) / abs(float(fused))
        e_g = float((leaf.grad - zf.grad).abs().max() / zf.grad.abs().max())
        print(f"{what}: loss {float(loss):.9g} vs fused {float(fused):.9g}  e_loss {e_l:.2e}  e_grad {e_g:.2e}")
        assert e_l <= 1e-6 and e_g <= 1e-6, (what, e_l, e_g)
    # a grouping that is a different function: classes of interleaved channels
    inter = MultiCoreKL([[0, 4, 8, 12], [1, 5, 9, 13], [2, 6, 10, 14], [3, 7, 11, 15]])
    perm = [k for g in inter.groups for k in g]
    zi = gpu_leaf(z)
    li = inter.from_logits(zi, t.to(DEV))
    lf, _ = group_kl(z[:, perm], t, 4)
    assert abs(float(li) - float(lf)) <= 1e-6 * abs(float(lf))


# ------------------------------------------------------------------------------------- 5. wide consistency
@pytest.mark.parametrize("K", CONS_KS)
def test_wide_softmax_mse_against_the_references_consistency_hook(fx, K):
    from cyhip.functions import SoftmaxMSEFn
    key = f"cons_K{K}"
    a, b = fx.dec(f"{key}_a_i8d8"), fx.dec(f"{key}_b_i8d8")
    ag, bg = gpu_leaf(a), gpu_leaf(b)
    loss = SoftmaxMSEFn.apply(ag.detach(), bg)
    loss.backward()
    assert ag.grad is None
    check(key, loss, fx[f"{key}_loss64"], bg.grad, fx.t(f"{key}_g64"), fx.e_ref("cons_"))
    b2 = gpu_leaf(b)
    loss2 = SoftmaxMSEFn.apply(ag.detach(), b2)
    loss2.backward()
    assert torch.equal(loss, loss2) and torch.equal(bg.grad, b2.grad), "two runs differ"
    # gradients to both arguments: d/da of mse(a, b) is d/db of mse(b, a)
    a3, b3 = gpu_leaf(a), gpu_leaf(b)
    SoftmaxMSEFn.apply(a3, b3).backward()
    assert torch.equal(b3.grad, bg.grad)
    a4 = gpu_leaf(a)
    SoftmaxMSEFn.apply(bg.detach(), a4).backward()
    assert torch.allclose(a3.grad, a4.grad, rtol=0, atol=4e-7 * float(a4.grad.abs().max()))


def test_consistency_hook_at_k32(fx):
    """through the hook the recipes use (config/hooks/consistency.yaml)"""
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.meters import MeterInterface
    from semi_seg.hooks import create_consistency_hook
    type(TrainerHook).names.clear()
    hook = create_consistency_hook(weight=1.0)()

    class _Ep:
        meters, cur_epoch = MeterInterface(), 0

    ep = _Ep()
    hook.epocher = ep
    a, b = fx.dec("cons_K32_a_i8d8"), fx.dec("cons_K32_b_i8d8")
    bg = gpu_leaf(b)
    loss = hook(unlabeled_tf_logits=bg, unlabeled_logits_tf=a.to(DEV), seed=1, affine_transformer=lambda x, **k: x)
    loss.backward()
    check("hook K=32", loss, fx["cons_K32_loss64"], bg.grad, fx.t("cons_K32_g64"), fx.e_ref("cons_"))
    type(TrainerHook).names.clear()


# ------------------------------------------------------------------------------------- 6. a full step
class PlainMultiCore(torch.nn.Module):
    """the same formula in torch ops, without `from_logits`: the epochers' probability-space fallback"""

    def __init__(self, groups):
        super().__init__()
        self.groups = groups

    def reduced_simplex(self, p):
        return torch.cat([p[:, g].sum(1, keepdim=True) for g in self.groups], dim=1)

    def kl(self, red, onehot):
        return -(onehot * torch.log((red + EPS) / (onehot + EPS))).sum(1).mean()

    def forward(self, p, onehot):
        return self.kl(self.reduced_simplex(p), onehot)


C_STEP, M_STEP = 4, 8


def _step_batches():
    g = torch.Generator().manual_seed(31)
    return blob_batch(2, 32, C_STEP, g), blob_batch(3, 32, C_STEP, g), blob_batch(2, 32, C_STEP, g, views=1)


def _train_step(criterion, sd0, lab, unl):
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.optim import RAdam
    from semi_seg.epochers.features import MultiCoreTrainEpocher
    from semi_seg.hooks import create_consistency_hook
    type(TrainerHook).names.clear()
    model = UNet(input_dim=1, num_classes=C_STEP * M_STEP, max_channel=128)
    model.load_state_dict(sd0)
    model.to(DEV)
    hook = create_consistency_hook(0.1)
    opt = RAdam([{"params": list(model.parameters())}], lr=1e-3, weight_decay=1e-5)
    ep = MultiCoreTrainEpocher(model=model, optimizer=opt, labeled_loader=OneBatchLoader(lab),
                               unlabeled_loader=OneBatchLoader(unl), sup_criterion=criterion, num_batches=1,
                               cur_epoch=0, device=DEV, two_stage=True, disable_bn=False,
                               scaler=torch.amp.GradScaler("cuda", enabled=False), accumulate_iter=1)
    ep.init()
    assert ep.num_classes == C_STEP
    seen = {}

    from contrastyou.hooks.base import EpocherHook

    class Spy(EpocherHook):
        def _call_implementation(self, *, unlabeled_tf_logits, **kw):
            seen["channels"] = unlabeled_tf_logits.shape[1]
            seen["logits"] = unlabeled_tf_logits.detach().clone()
            return torch.zeros((), device=DEV)

    random.seed(5)
    with ep.register_hook(hook(), Spy(name="spy")):
        ep.run()
    torch.cuda.synchronize()
    type(TrainerHook).names.clear()
    params = {k: v.detach().float().cpu() for k, v in model.named_parameters()}
    return model, params, ep.get_metric(), seen


def test_a_full_multicore_step_fused_against_the_torch_composition():
    from contrastyou.arch import UNet
    from contrastyou.losses.multicore_loss import MultiCoreKL
    from semi_seg.epochers.features import MultiCoreEvalEpocher
    torch.manual_seed(11)
    sd0 = {k: v.clone() for k, v in UNet(input_dim=1, num_classes=C_STEP * M_STEP, max_channel=128).state_dict().items()}
    lab, unl, val = _step_batches()
    groups = groups_of(C_STEP, M_STEP)
    model, p_f, m_f, seen_f = _train_step(MultiCoreKL(groups), sd0, lab, unl)
    _, p_t, m_t, seen_t = _train_step(PlainMultiCore(groups), sd0, lab, unl)
    assert seen_f["channels"] == C_STEP * M_STEP, "hooks receive the K-channel logits"
    assert torch.equal(seen_f["logits"], seen_t["logits"]), "both forwards are bit-identical"
    semi_f, semi_t = m_f["semi"], m_t["semi"]
    print("fused", semi_f, "\ntorch", semi_t)
    for name in ("sup_loss", "reg_loss"):
        e = abs(semi_f[name] - semi_t[name]) / abs(semi_t[name])
        print(f"{name}: {semi_f[name]:.9g} vs {semi_t[name]:.9g}  e {e:.2e}")
        assert math.isfinite(semi_f[name]) and e <= 1e-6, (name, e)
    assert semi_f["reg_loss"] != 0
    worst = max(float((p_f[k] - p_t[k]).abs().max() / p_t[k].abs().max()) for k in p_t)
    moved = max(float((p_f[k] - sd0[k].float()).abs().max()) for k in p_f)
    print(f"parameters after the RAdam step: worst relative distance {worst:.2e}; largest move {moved:.2e}")
    assert moved > 0 and worst <= 1e-4
    assert semi_f["sup_dice"] == semi_t["sup_dice"], (semi_f["sup_dice"], semi_t["sup_dice"])
    assert len(semi_f["sup_dice"]) == C_STEP  # DSC1..DSC3 of the TRUE classes + DSC_mean

    ev = MultiCoreEvalEpocher(model=model, loader=OneBatchLoader({k: v[0] for k, v in val.items()}),
                              sup_criterion=MultiCoreKL(groups), cur_epoch=0, device=DEV,
                              scaler=torch.amp.GradScaler("cuda", enabled=False), accumulate_iter=1)
    ev.init()
    ev.run()
    stats = ev.get_metric()["eval"]
    print("eval", stats)
    assert math.isfinite(stats["loss"]) and stats["loss"] == stats["true_loss"]
    assert all(0.0 <= v <= 1.0 for v in stats["dice"].values())
    assert 0.0 <= ev.get_score() <= 1.0


# ------------------------------------------------------------------------------------- 7. the trainer
def test_multicore_trainer_runs_an_epoch(tmp_path):
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.losses.multicore_loss import MultiCoreKL
    from semi_seg.hooks import create_consistency_hook
    from semi_seg.trainers.features import MulticoreTrainer
    lab, unl, val = _step_batches()
    val = {k: v[0] for k, v in val.items()}
    cfg = {"Arch": {"true_num_classes": C_STEP, "max_channel": 128},
           "Optim": {"name": "RAdam", "lr": 1e-4, "weight_decay": 1e-5},
           "Scheduler": {"multiplier": 100, "warmup_max": 1}, "Trainer": {"name": "semi"}}
    type(TrainerHook).names.clear()
    torch.manual_seed(12)
    model = UNet(input_dim=1, num_classes=C_STEP * M_STEP, max_channel=128)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    tr = MulticoreTrainer(model=model, labeled_loader=OneBatchLoader(lab), unlabeled_loader=OneBatchLoader(unl),
                          val_loader=OneBatchLoader(val), test_loader=OneBatchLoader(val),
                          criterion=MultiCoreKL(groups_of(C_STEP, M_STEP)), save_dir=str(tmp_path), max_epoch=1,
                          num_batches=1, device=DEV, disable_bn=False, two_stage=True, config=cfg, enable_scale=False)
    with tr.register_hook(create_consistency_hook(0.1)):
        tr.init()
        groups = tr._optimizer.param_groups
        assert len(groups) == 2 and groups[1]["params"] == [] and groups[1]["lr"] == 1e-4
        tr.start_training()
    assert tr._cur_epoch == 1
    assert any(not torch.equal(v.detach().cpu(), before[k]) for k, v in model.named_parameters())
    assert all(torch.isfinite(v).all() for v in model.state_dict().values())
    header = (tmp_path / "storage.csv").read_text().strip().splitlines()[0]
    for col in ("tra/semi/sup_loss", "tra/semi/reg_loss", "val/eval/true_loss", "test/eval/true_loss"):
        assert col in header, (col, header)
    type(TrainerHook).names.clear()
