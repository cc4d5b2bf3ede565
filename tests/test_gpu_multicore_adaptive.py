"""The adaptive over-segmented criteria on the GPU: the class-mixing softmax-KL and Dice kernels (csrc/cy_mix_loss.hip),
`SoftmaxMixKLFn`, `UniversalDice.add_logits(mix=)`, the three criteria and the multi-prototype epochers under them,
against tests/golden/multicore_adaptive*.npz (the reference's criteria in f32 and f64,
tests/golden/gen_goldens_adaptive.py).

Tolerance rule (the one of tests/test_gpu_multicore.py, unchanged).  The yardstick is the reference's own f32-to-f64
distance on the fixture's inputs:
    e(x) = |x - x64| relative: 2-norm for gradients, element-wise maximum over max|grad64|, |.| / |loss64| for the loss
    require e_hip <= max(4 * e_ref, 1e-6), e_ref = the largest value over the fixture's cases of the same kind
with three kinds: logit gradients, parameter gradients, losses.  No pixel is left out of any comparison.  Every figure
is printed before it is asserted.
"""
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import adaptive_fixture as af
from adaptive_fixture import BIG, BIG_KEY, BIG_ROWS, CASES, E_GT, E_GZ, E_LOSS, MI_WEIGHT, decode, pixel_rows, tag

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR, FACTOR = 1e-6, 4.0
EPS = 1e-16
REPO = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def fx(golden_dir):
    data = af.load(golden_dir)

    class Fx:
        def __getitem__(self, k):
            return data[k]

        def __contains__(self, k):
            return k in data

        def t(self, k):
            return torch.from_numpy(data[k])

        def e_ref(self):
            """[gz 2-norm, gz max, gT 2-norm, gT max, loss]: the largest over the fixture's cases, kind by kind"""
            return np.nanmax(np.stack([v for k, v in data.items() if k.endswith("_e_ref")]), axis=0)

        def case(self, key):
            """(kind, K, C, logits f32 [N,K,H,W], labels int64 [N,H,W], parameter f32 or None), on the CPU"""
            if key == BIG_KEY:
                kind, K, C, _ = BIG
                z, t, T = af.big_inputs()
                return kind, K, C, torch.from_numpy(z).float() / 8, torch.from_numpy(t).long(), \
                    torch.from_numpy(T).float() / 8
            kind, K, C = SHAPES[key]
            T = decode(f"{key}_T_i8d8", data[f"{key}_T_i8d8"]) if f"{key}_T_i8d8" in data else None
            return kind, K, C, decode(f"{key}_z_i8d8", data[f"{key}_z_i8d8"]), self.t(f"{key}_t").long(), T

    return Fx()


SHAPES = {tag(*c): c for c in CASES}
KEYS = list(SHAPES) + [BIG_KEY]


def bound(e_ref):
    return max(FACTOR * float(e_ref), FLOOR)


def cpu64(t):
    return t.detach().double().cpu()


def check_loss(what, loss, loss64, e_ref):
    loss, loss64 = float(loss), float(loss64)
    e = abs(loss - loss64) / abs(loss64)
    print(f"{what}: loss {loss:.9g} vs {loss64:.9g}  e_loss {e:.2e} (bound {bound(e_ref[E_LOSS]):.2e})")
    assert math.isfinite(loss) and e <= bound(e_ref[E_LOSS]), (what, e)


def check_grad(what, grad, grad64, e_ref2):
    """e_ref2 = the (2-norm, max) pair of this gradient's kind"""
    got, g64 = cpu64(grad), cpu64(grad64)
    assert got.shape == g64.shape, (what, got.shape, g64.shape)
    assert torch.isfinite(got).all(), what
    d = got - g64
    e2, emax = float(d.norm() / g64.norm()), float(d.abs().max() / g64.abs().max())
    print(f"{what}: e_2 {e2:.2e} (bound {bound(e_ref2[0]):.2e})  e_max {emax:.2e} (bound {bound(e_ref2[1]):.2e})")
    fails = [f"{n} {e:.2e}" for n, e, b in (("e_2", e2, e_ref2[0]), ("e_max", emax, e_ref2[1])) if e > bound(b)]
    assert not fails, f"{what}: {fails}"


def make_criterion(kind, K, C, T):
    """this package's criterion of a case on the device, its parameter set to T"""
    from contrastyou.losses import multicore_loss as ml
    if kind == "adaptive":
        crit = ml.AdaptiveOverSegmentedLoss(K, C, DEV)
    elif kind == "stricter":
        crit = ml.StricterAdaptiveOverSegmentedLoss(K, C, DEV)
    else:
        crit = ml.StricterAdaptiveOverSegmentedLossWithMI(K, C, DEV, mi_weight=MI_WEIGHT)
    with torch.no_grad():
        crit._translate_matrix.copy_(T.to(DEV))
    return crit


def run_case(kind, K, C, z, t, T):
    """-> (loss, dloss/dz, dloss/dT or None) on the device: through the criterion's `from_logits`; the membership
    case through SoftmaxMixKLFn on the 0/1 matrix"""
    from cyhip.functions import SoftmaxMixKLFn
    zz = z.float().to(DEV).requires_grad_(True)
    if kind == "member":
        loss = SoftmaxMixKLFn.apply(zz, t.to(DEV), af.membership(K, C).to(DEV), EPS)
        loss.backward()
        return loss.detach(), zz.grad, None
    crit = make_criterion(kind, K, C, T)
    assert crit.fusable(K)
    loss = crit.from_logits(zz, t.to(DEV))
    loss.backward()
    gT = crit._translate_matrix.grad
    return loss.detach(), zz.grad, gT if crit._translate_matrix.numel() else None


def formulas64(z, t, M):
    """f64 CPU evaluation of the header's formulas for a [K, C] matrix M: -> (loss, dz, dM, reduced arg-max)"""
    z, M = z.double(), M.double()
    P = t.numel()
    p = z.softmax(1).movedim(1, -1).reshape(P, -1)         # [P, K]
    tt = t.reshape(P)
    R = p @ M                                              # [P, C]
    Rt = R.gather(1, tt[:, None])[:, 0]
    loss = -torch.log((Rt + EPS) / (1 + EPS)).mean()
    dz = -(p * (M[:, tt].t() - Rt[:, None]) / (Rt[:, None] + EPS)) / P
    dM = torch.zeros_like(M)
    dM.index_add_(1, tt, -(p / (Rt[:, None] + EPS)).t() / P)
    N, K, H, W = z.shape
    return loss, dz.reshape(N, H, W, K).movedim(-1, 1), dM, R.argmax(1).reshape(N, H, W)


def counts_of(pred, target, C):
    """int64 [N, C, 2] (intersection, union) of class maps [N, H, W], as UniversalDice counts them"""
    po = torch.nn.functional.one_hot(pred.long(), C).movedim(-1, 1)
    to = torch.nn.functional.one_hot(target.long(), C).movedim(-1, 1)
    return torch.stack([(po * to).sum((2, 3)), (po + to).sum((2, 3))], dim=-1)


# ------------------------------------------------------------------------------------- 1. loss, dz, dT
@pytest.mark.parametrize("key", KEYS)
def test_loss_and_gradients_against_the_reference(fx, key):
    kind, K, C, z, t, T = fx.case(key)
    assert z.shape[1] == K
    loss, gz, gT = run_case(kind, K, C, z, t, T)
    e_ref = fx.e_ref()
    print(f"e_ref (largest over the fixture): dz {e_ref[E_GZ]}  dT {e_ref[E_GT]}  loss {e_ref[E_LOSS]:.2e}")
    check_loss(key, loss, fx[f"{key}_loss64"], e_ref)
    if key == BIG_KEY:
        # every pixel against the f64 formulas, the stored rows against the reference
        M64 = af.mix_of(kind, K, C, T.double())
        l64, dz64, dM64, _ = formulas64(z, t, M64)
        Tleaf = T.double().requires_grad_(True)
        S = Tleaf.softmax(1)
        ent = -(S * (S + 1e-16).log()).sum(1).mean() * 1e-3  # the criterion's extra term (entropy_decay = 1e-3)
        (ent + (S * dM64).sum()).backward()                  # dM -> dT: the chain rule through the softmax
        assert abs(float(l64 + ent.detach()) - float(fx[f"{key}_loss64"])) <= 1e-12 * abs(float(l64))
        check_grad(f"{key} dz (formula, every pixel)", gz, dz64, e_ref[E_GZ])
        check_grad(f"{key} dT (formula)", gT, Tleaf.grad, e_ref[E_GT])
        check_grad(f"{key} dz (reference, stored rows)", pixel_rows(gz.cpu(), BIG_ROWS), fx.t(f"{key}_gz64"),
                   e_ref[E_GZ])
    else:
        check_grad(f"{key} dz", gz, fx.t(f"{key}_gz64"), e_ref[E_GZ])
    if f"{key}_gT64" in fx:
        check_grad(f"{key} dT", gT, fx.t(f"{key}_gT64"), e_ref[E_GT])
    else:
        assert gT is None, key


@pytest.mark.parametrize("key", ["adaptive_k16c4", "adaptive_k40c5"])
def test_kernel_gradient_with_respect_to_the_mix(fx, key):
    """dmix itself (before the softmax of T) against the f64 formula, for a matrix that is not row-stochastic"""
    from cyhip.functions import SoftmaxMixKLFn
    kind, K, C, z, t, T = fx.case(key)
    M = (T - T.min()) * 0.37                      # non-negative, rows do not sum to one, some zeros
    zz = z.to(DEV).requires_grad_(True)
    MM = M.to(DEV).requires_grad_(True)
    loss = SoftmaxMixKLFn.apply(zz, t.to(DEV), MM, EPS)
    (2.5 * loss).backward()
    l64, dz64, dM64, _ = formulas64(z, t, M)
    e_ref = fx.e_ref()
    check_loss(key, loss, l64, e_ref)
    check_grad(f"{key} dz", zz.grad, 2.5 * dz64, e_ref[E_GZ])
    check_grad(f"{key} dmix", MM.grad, 2.5 * dM64, e_ref[E_GT])


# every instantiation of the backward kernels that the fixture's shapes do not reach: the thread form's (K, C) register
# buckets {4, 8, 16} x {4, 8, 16}, the row form without 16-byte loads at C <= 8 and C <= 16, and K <= 16 with more than
# 128 accumulators, which takes the row form
BUCKET_SHAPES = [(4, 8), (4, 16), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (13, 16), (21, 7), (21, 12)]


@pytest.mark.parametrize("K,C", BUCKET_SHAPES)
def test_backward_register_buckets_against_the_f64_formulas(fx, K, C):
    """needs no fixture: seeded logits on the 1/8 grid and a non-negative matrix against the f64 formulas, under the
    fixture's bounds; and dlogits has the same bits with and without dmix"""
    from cyhip.functions import SoftmaxMixKLFn
    g = torch.Generator().manual_seed(100 * K + C)
    N, H, W = af.SHAPE
    z = torch.randint(-48, 49, (N, K, H, W), generator=g).float() / 8
    t = torch.randint(0, C, (N, H, W), generator=g)
    M = torch.randint(0, 17, (K, C), generator=g).float() / 8
    M[:, 0] += 0.125                              # no all-zero row of M: R_t > 0 at every pixel
    l64, dz64, dM64, _ = formulas64(z, t, M)
    e_ref = fx.e_ref()
    grads = []
    for need in (True, False):
        zz = z.to(DEV).requires_grad_(True)
        MM = M.to(DEV).requires_grad_(need)
        loss = SoftmaxMixKLFn.apply(zz, t.to(DEV), MM, EPS)
        loss.backward()
        grads.append(zz.grad)
        if need:
            check_loss(f"K={K} C={C}", loss, l64, e_ref)
            check_grad(f"K={K} C={C} dz", zz.grad, dz64, e_ref[E_GZ])
            check_grad(f"K={K} C={C} dmix", MM.grad, dM64, e_ref[E_GT])
    assert torch.equal(grads[0], grads[1]), f"K={K} C={C}: dz differs between dmix wanted and dmix NULL"


# ------------------------------------------------------------------------------------- 2. Dice
@pytest.mark.parametrize("key", KEYS)
def test_mix_dice_counts_equal_the_references_arg_max(fx, key):
    from contrastyou.meters import UniversalDice
    from cyhip import ops
    kind, K, C, z, t, T = fx.case(key)
    assert int((t[0] == C - 1).sum()) == 0 or C == 1, "class C - 1 is absent from image 0"
    M = af.mix_of(kind, K, C, T).to(DEV)
    want = counts_of(fx.t(f"{key}_argmax"), t, C)
    counts = ops.mix_dice_counts(ops.to_nhwc(z.to(DEV)), t.to(DEV), M)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (z.shape[0], C, 2)
    assert torch.equal(counts.cpu(), want), key
    # through the meter: the Dice of the reference's `meters["dice"].add(reduced arg-max, target)`
    meter = UniversalDice(C, report_axis=list(range(1, C)))
    meter.add_logits(z.to(DEV), t.unsqueeze(1).to(DEV), mix=M)
    (got, _), = meter._pending
    assert torch.equal(got, counts)
    ref = UniversalDice(C, report_axis=list(range(1, C)))
    ref.add(fx.t(f"{key}_argmax").long(), t)
    assert meter.summary() == ref.summary()
    if key == KEYS[0]:
        with pytest.raises(AssertionError):
            UniversalDice(C + 1).add_logits(z.to(DEV), t.to(DEV), mix=M)  # the meter counts C + 1 classes


# ------------------------------------------------------------------------------------- 3. logits vs probability space
@pytest.mark.parametrize("key", ["adaptive_k15c3", "adaptive_k32c4", "stricter_k4c4", "stricter_k40c5", "mi_k32c4"])
def test_from_logits_equals_the_probability_space_forward(fx, key):
    from contrastyou.utils.general import class2one_hot
    kind, K, C, z, t, T = fx.case(key)
    crit = make_criterion(kind, K, C, T)
    zg, tg = z.to(DEV), t.to(DEV)
    onehot = class2one_hot(tg, C)
    with torch.no_grad():
        fused, prob = crit.from_logits(zg, tg), crit(zg.softmax(1), onehot)
        kl_fused, kl_prob = crit.kl_from_logits(zg, tg), crit.kl(crit.reduced_simplex(zg.softmax(1)), onehot)
    for what, a, b in (("from_logits vs forward", fused, prob), ("kl_from_logits vs kl(reduced)", kl_fused, kl_prob)):
        e = abs(float(a) - float(b)) / abs(float(b))
        print(f"{key} {what}: {float(a):.9g} vs {float(b):.9g}  e {e:.2e}")
        assert e <= 1e-6, (key, what, e)
    if kind == "stricter":
        assert float(fused) == float(kl_fused)
    else:
        assert float(fused) != float(kl_fused)
    # the gradients of the two paths agree too: each is an f32 evaluation within the test-1 bound of the f64 value, so
    # they lie within twice that bound of each other
    e_ref = fx.e_ref()
    bz, bT = 2 * bound(e_ref[E_GZ][1]), 2 * bound(e_ref[E_GT][1])
    zf, zp = zg.clone().requires_grad_(True), zg.clone().requires_grad_(True)
    crit.from_logits(zf, tg).backward()
    gT_f = crit._translate_matrix.grad.clone() if crit._translate_matrix.numel() else None
    crit._translate_matrix.grad = None
    crit(zp.softmax(1), onehot).backward()
    e = float((zf.grad - zp.grad).abs().max() / zp.grad.abs().max())
    print(f"{key} dz: fused vs probability space e_max {e:.2e} (bound {bz:.2e})")
    assert e <= bz
    if gT_f is not None:
        gT_p = crit._translate_matrix.grad
        e = float((gT_f - gT_p).abs().max() / gT_p.abs().max())
        print(f"{key} dT: fused vs probability space e_max {e:.2e} (bound {bT:.2e})")
        assert e <= bT


def test_wider_shapes_compose_in_probability_space():
    from contrastyou.losses.multicore_loss import AdaptiveOverSegmentedLoss
    g = torch.Generator().manual_seed(4)
    crit = AdaptiveOverSegmentedLoss(80, 5, DEV)
    assert not crit.fusable(80)
    z = torch.randn(2, 80, 6, 5, generator=g).to(DEV).requires_grad_(True)
    t = torch.randint(0, 5, (2, 6, 5), generator=g).to(DEV)
    loss = crit.from_logits(z, t)
    loss.backward()
    M = crit.mix().detach().double().cpu()
    l64, dz64, _, _ = formulas64(z.detach().cpu(), t.cpu(), M)
    ent = float(crit.extra_terms())
    assert abs(float(loss) - (float(l64) + ent)) <= 1e-5 * abs(float(l64))
    assert float((z.grad.double().cpu() - dz64).abs().max() / dz64.abs().max()) <= 1e-5
    assert crit._translate_matrix.grad is not None


# ------------------------------------------------------------------------------------- 4. / 5. bits
@pytest.mark.parametrize("key", ["adaptive_k32c4", "adaptive_k16c4", BIG_KEY])
def test_two_runs_give_identical_bits_and_dz_does_not_depend_on_dmix(fx, key):
    from cyhip.functions import SoftmaxMixKLFn
    kind, K, C, z, t, T = fx.case(key)
    a, b = run_case(kind, K, C, z, t, T), run_case(kind, K, C, z, t, T)
    for name, x, y in zip(("loss", "dz", "dT"), a, b):
        assert torch.equal(x, y), f"{key}: two runs differ in {name}"
    # T without grad -> dmix is not computed (NULL): the same dz bits
    M = af.mix_of(kind, K, C, T).to(DEV)
    grads = []
    for need in (True, False):
        zz = z.to(DEV).requires_grad_(True)
        MM = M.clone().requires_grad_(need)
        SoftmaxMixKLFn.apply(zz, t.to(DEV), MM, EPS).backward()
        assert (MM.grad is not None) == need
        grads.append(zz.grad)
    assert torch.equal(grads[0], grads[1]), f"{key}: dz differs between dmix wanted and dmix NULL"


def test_stricter_at_k_equal_c_never_asks_for_dmix(fx, monkeypatch):
    from cyhip import ops
    kind, K, C, z, t, T = fx.case("stricter_k4c4")
    asked = []
    real = ops.softmax_mix_kl_bwd
    monkeypatch.setattr(ops, "softmax_mix_kl_bwd", lambda *a: (asked.append(a[-1]), real(*a))[1])
    run_case(kind, K, C, z, t, T)
    assert asked == [False]


# ------------------------------------------------------------------------------------- 6. epochers
@pytest.fixture(scope="module")
def stepped():
    import adaptive_step_case as sc
    return sc.run_steps(graph=True)


def test_the_translation_matrix_is_trained_by_the_step(fx, stepped):
    import adaptive_step_case as sc
    T = stepped["T"]
    assert len(T) == sc.STEPS + 1 and tuple(T[0].shape) == (sc.K_STEP - sc.C_STEP, sc.C_STEP)
    assert torch.equal(T[0], torch.zeros_like(T[0]))
    for a, b in zip(T, T[1:]):
        assert not torch.equal(a, b), "T did not move in a step"
    assert all(torch.isfinite(x).all() for x in T)
    # step 1: RAdam's first step is plain -lr * (g + wd * T) (rho_1 = 1 <= 5, bias-corrected first moment = g), T0 = 0,
    # g = the f64 dT of the logits the criterion saw
    z, t = stepped["logits"], stepped["labels"]
    assert z.shape[1] == sc.K_STEP
    Tleaf = T[0].double().requires_grad_(True)
    M = af.mix_of("stricter", sc.K_STEP, sc.C_STEP, Tleaf)
    red = torch.einsum("nkhw,kc->nchw", z.double().softmax(1), M)
    loss = -torch.log((red.gather(1, t[:, None]) + EPS) / (1 + EPS)).mean()
    loss.backward()
    e_ref = fx.e_ref()
    check_grad("T after the first step vs -lr * f64 dT", T[1], -sc.LR * Tleaf.grad, e_ref[E_GT])
    semi = stepped["metrics"]["semi"]
    print(semi)
    assert math.isfinite(semi["sup_loss"]) and len(semi["sup_dice"]) == sc.C_STEP


def test_graph_replay_and_eager_steps_train_the_same_matrix(stepped, tmp_path):
    """the replayed graphs cover the network passes; T's gradient arrives outside them.  The eager run is a fresh
    process under CY_GRAPH_STEP=0 (cyhip.graphed reads the switch at import)"""
    assert stepped["replayed"], "the run in this process must have captured and replayed the passes"
    out = tmp_path / "eager.pt"
    env = dict(os.environ, CY_GRAPH_STEP="0")
    r = subprocess.run([sys.executable, str(REPO / "tests" / "adaptive_step_case.py"), str(out)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    eager = torch.load(out, weights_only=True)
    assert not eager["replayed"]
    for i, (a, b) in enumerate(zip(stepped["T"], eager["T"])):
        d = float((a - b).abs().max())
        print(f"T after {i} steps: graph vs eager max |difference| {d:.3e}")
    for i, (a, b) in enumerate(zip(stepped["T"], eager["T"])):
        assert torch.equal(a, b), f"T after {i} steps differs between graph replay and eager steps"


def test_eval_epocher_true_loss(stepped):
    import adaptive_step_case as sc
    from contrastyou.losses.multicore_loss import AdaptiveOverSegmentedLoss
    from semi_seg.epochers.features import MultiCoreEvalEpocher
    from step_harness import OneBatchLoader
    _, _, val = sc.step_batches()
    val = {k: v[0] for k, v in val.items()}
    torch.manual_seed(2)
    for crit, same in ((stepped["criterion"], True), (AdaptiveOverSegmentedLoss(sc.K_STEP, sc.C_STEP, DEV), False)):
        ev = MultiCoreEvalEpocher(model=stepped["model"], loader=OneBatchLoader(val), sup_criterion=crit, cur_epoch=0,
                                  device=DEV, scaler=torch.amp.GradScaler("cuda", enabled=False), accumulate_iter=1)
        ev.init()
        ev.run()
        stats = ev.get_metric()["eval"]
        print(type(crit).__name__, stats)
        assert math.isfinite(stats["loss"]) and math.isfinite(stats["true_loss"])
        assert (stats["loss"] == stats["true_loss"]) == same
        if not same:
            with torch.no_grad():
                extra = float(crit.extra_terms())
            assert abs(stats["loss"] - stats["true_loss"] - extra) <= 1e-6 * abs(stats["loss"])
        assert all(0.0 <= v <= 1.0 for v in stats["dice"].values()) and len(stats["dice"]) == sc.C_STEP
        assert 0.0 <= ev.get_score() <= 1.0


def test_multicore_trainer_puts_the_matrix_into_the_second_param_group(tmp_path):
    import adaptive_step_case as sc
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.losses.multicore_loss import StricterAdaptiveOverSegmentedLoss
    from semi_seg.hooks import create_consistency_hook
    from semi_seg.trainers.features import MulticoreTrainer
    from step_harness import OneBatchLoader
    lab, unl, val = sc.step_batches()
    val = {k: v[0] for k, v in val.items()}
    cfg = {"Arch": {"true_num_classes": sc.C_STEP, "max_channel": 128},
           "Optim": {"name": "RAdam", "lr": 1e-4, "weight_decay": 1e-5},
           "Scheduler": {"multiplier": 100, "warmup_max": 1}, "Trainer": {"name": "semi"}}
    type(TrainerHook).names.clear()
    torch.manual_seed(12)
    model = UNet(input_dim=1, num_classes=sc.K_STEP, max_channel=128)
    crit = StricterAdaptiveOverSegmentedLoss(sc.K_STEP, sc.C_STEP, DEV)
    tr = MulticoreTrainer(model=model, labeled_loader=OneBatchLoader(lab), unlabeled_loader=OneBatchLoader(unl),
                          val_loader=OneBatchLoader(val), test_loader=OneBatchLoader(val), criterion=crit,
                          save_dir=str(tmp_path), max_epoch=1, num_batches=1, device=DEV, disable_bn=False,
                          two_stage=True, config=cfg, enable_scale=False)
    with tr.register_hook(create_consistency_hook(0.1)):
        tr.init()
        groups = tr._optimizer.param_groups
        assert len(groups) == 2 and len(groups[1]["params"]) == 1 and groups[1]["params"][0] is crit._translate_matrix
        tr.start_training()
    T = crit._translate_matrix.detach()
    assert torch.isfinite(T).all() and float(T.abs().max()) > 0, "the optimizer moved T"
    sd = tr.state_dict()  # the criterion is a non-trackable buffer: T is not part of the trainer's checkpoint
    assert "_criterion" not in sd["other_state"] and not any("_translate_matrix" in k for k in sd["module_state"])
    type(TrainerHook).names.clear()
