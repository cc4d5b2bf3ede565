"""SelfPacedSupConLoss on the fused kernels of csrc/cy_contrast.hip (supcon_sp_fwd_kernel, supcon_sp_finalize_kernel,
supcon_sp_bwd_kernel) against the float64 oracle, the reference's own record (tests/golden/selfpaced.npz) and the
composition the criterion keeps for the widths the kernels refuse.  Cases, tolerances and the rule every gamma comes
from: tests/selfpaced_cases.py; what those tables promise is asserted on the CPU in tests/test_selfpaced_host.py.
Bounds are max|got - ref| <= tol * max|ref| over the whole tensor, no element left out; the upstream gradient of every
backward is GSCALE."""
import functools
import random

import numpy as np
import pytest
import torch

from tests import selfpaced_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def check(got, ref, tol, what, floor=0.0):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} elements not finite"
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    print(f"{what}: err {err:.3e}, tol {tol:.1e} * {scale:.3e} + {floor:.1e}")
    assert err <= tol * scale + floor, f"{what}: max err {err:.3e} > {tol:.1e} * {scale:.3e} + {floor:.1e}"


def check_loss(got, ref, what, tol=sc.TOL_LOSS):
    got, ref = float(got), float(ref)
    print(f"{what}: {got!r} vs {ref!r}, rel {abs(got - ref) / abs(ref):.3e}")
    assert abs(got - ref) <= tol * abs(ref), f"{what}: {got!r} vs {ref!r}"


def criterion(mode, gamma, cg=False, defer=False):
    from contrastyou.losses import SelfPacedSupConLoss
    crit = SelfPacedSupConLoss(temperature=sc.T, weight_update=mode, correct_grad=cg)
    crit.set_gamma(gamma)
    crit.defer_checks = defer
    return crit


def run(crit, z1, z2, target, mask, composition=False):
    """forward and backward (upstream gradient GSCALE) -> loss, ratio, dz1, dz2"""
    a, b = z1.to(DEV).requires_grad_(True), z2.to(DEV).requires_grad_(True)
    m = None if mask is None else mask.to(DEV)
    loss = crit._composition(a, b, target, m) if composition else crit(a, b, target=target, mask=m)
    (loss * sc.GSCALE).backward()
    return loss.detach(), crit.downgrade_ratio, a.grad, b.grad


@functools.lru_cache(maxsize=None)
def oracle(p, mode, cg):
    """the oracle in float64 on the CPU, once per (problem, mode, correct_grad): gamma, loss, ratio, dz1, dz2"""
    from oracle import next_rows as onr
    z1, z2, target, mask = sc.tensors(p)
    gamma = sc.gamma_of(p, mode)
    a, b = z1.double().requires_grad_(True), z2.double().requires_grad_(True)
    loss, ratio = onr.self_paced_supcon(a, b, target, gamma=gamma, weight_update=mode, correct_grad=cg, t=sc.T, mask=mask)
    (loss * sc.GSCALE).backward()
    return gamma, loss.item(), ratio, a.grad, b.grad


def against_oracle(p, mode, cg, fused=True):
    gamma, want, wratio, da, db = oracle(p, mode, cg)
    z1, z2, target, mask = sc.tensors(p)
    crit = criterion(mode, gamma, cg)
    loss, ratio, g1, g2 = run(crit, z1, z2, target, mask)
    assert (crit._last is not None) == fused, f"{p.name}: which path ran"
    what = f"{p.name} {mode} c{int(cg)}"
    print(f"{what}: gamma {gamma:.6f}, ratio {ratio!r} vs {wratio!r}")
    assert isinstance(ratio, float), "defer_checks=False: downgrade_ratio is a Python float"
    check_loss(loss, want, what + " loss")
    assert abs(ratio - wratio) <= sc.RATIO_FLOOR, f"{what}: ratio {ratio!r} vs {wratio!r}"
    check(g1, da, sc.TOL_GRAD, what + " dz1")
    check(g2, db, sc.TOL_GRAD, what + " dz2")
    return crit


# ---------------------------------------------------------------- against the exact case, the oracle and the golden
@pytest.mark.parametrize("mode", sc.MODES)
def test_one_pair_is_exact(mode):
    """R = 2, both views the same +-1/4 row: l_ij = 0, w = 1, loss and gradient 0 within ONE_PAIR_ABS"""
    p = sc.ONE_PAIR
    z1, z2, target, mask = sc.tensors(p)
    for cg in (False, True):
        crit = criterion(mode, sc.gamma_of(p, mode), cg)
        loss, ratio, g1, g2 = run(crit, z1, z2, target, mask)
        assert crit._last is not None, "the fused path"
        print(f"one pair {mode} c{int(cg)}: loss {loss.item()!r}, ratio {ratio!r}, max|dz| {max(g1.abs().max().item(), g2.abs().max().item())!r}")
        assert abs(loss.item()) <= sc.ONE_PAIR_ABS and ratio == 1.0
        assert g1.abs().max().item() <= sc.ONE_PAIR_ABS and g2.abs().max().item() <= sc.ONE_PAIR_ABS


@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("p", sc.SIZE_PROBLEMS, ids=lambda p: p.name)
def test_sizes_against_the_oracle(p, mode):
    for cg in (False, True):
        against_oracle(p, mode, cg)


@pytest.mark.parametrize("p", sc.WIDTH_PROBLEMS, ids=lambda p: p.name)
def test_widths_against_the_oracle(p):
    crit = against_oracle(p, "soft", False)
    w = crit.sp_mask[crit.pos_mask.bool()]
    assert bool((w == 0).any()) and bool(((w > 0) & (w < 1)).any()), "both branches of the clamp"


@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("p", sc.FALLBACK_PROBLEMS, ids=lambda p: p.name)
def test_refused_widths_fall_back_to_the_composition(p, mode):
    against_oracle(p, mode, True, fused=False)


@pytest.mark.parametrize("mode", sc.MODES)
def test_general_mask(mode):
    """kind_d_mask(35, 61): asymmetric, values {0, 1, -1, 2} -- the MASK instantiations"""
    for cg in (False, True):
        against_oracle(sc.MASK_PROBLEM, mode, cg)


@pytest.mark.parametrize("cg", (False, True), ids=("c0", "c1"))
@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("p", sc.PATH_PROBLEMS, ids=lambda p: p.name)
def test_fused_against_the_composition(p, mode, cg):
    """both paths on the same tensors within TOL_PATHS, loss and gradients: the general mask (MASK instantiations) and
    labels over two and over fifteen column splits"""
    z1, z2, target, mask = sc.tensors(p)
    gamma = sc.gamma_of(p, mode)
    fc, cc_ = criterion(mode, gamma, cg), criterion(mode, gamma, cg)
    f = run(fc, z1, z2, target, mask)
    c = run(cc_, z1, z2, target, mask, composition=True)
    assert fc._last is not None and cc_._last is None, "which path ran"
    what = f"{p.name} {mode} c{int(cg)}: fused against composition"
    check_loss(f[0], c[0], what, sc.TOL_PATHS)
    assert abs(f[1] - c[1]) <= sc.RATIO_FLOOR, (what, f[1], c[1])
    check(f[2], c[2], sc.TOL_PATHS, what + " dz1")
    check(f[3], c[3], sc.TOL_PATHS, what + " dz2")


@pytest.mark.parametrize("tag", sc.GOLDEN_TAGS)
def test_golden(tag, golden_dir):
    """the reference's own float64 record: labels i % 3 and the asymmetric masks b, d; hard, soft; correct_grad"""
    g, src = np.load(golden_dir / sc.GOLDEN_FILE), np.load(golden_dir / sc.GOLDEN_INPUTS)
    positives, mode, cg = tag.split("_")
    target = [i % 3 for i in range(sc.GOLDEN_N)] if positives == "mod3" else None
    mask = None if positives == "mod3" else torch.from_numpy(src[f"{positives}_mask"])
    crit = criterion(mode, float(g[f"{tag}_gamma"]), cg == "c1")
    loss, ratio, g1, g2 = run(crit, torch.from_numpy(src["z1"]), torch.from_numpy(src["z2"]), target, mask)
    assert crit._last is not None, "the fused path"
    check_loss(loss, float(g[f"{tag}_loss"]), tag + " loss")
    print(f"{tag}: ratio {ratio!r} vs {float(g[tag + '_ratio'])!r}, tol {sc.ratio_tol(tag):.1e}")
    assert abs(ratio - float(g[f"{tag}_ratio"])) <= sc.ratio_tol(tag), tag
    check(g1, torch.from_numpy(g[f"{tag}_dz1"]), sc.TOL_GRAD, tag + " dz1")
    check(g2, torch.from_numpy(g[f"{tag}_dz2"]), sc.TOL_GRAD, tag + " dz2")


# ---------------------------------------------------------------- behaviour
@pytest.mark.parametrize("mode", sc.MODES)
def test_gamma_to_infinity_is_supcon(mode):
    from contrastyou.losses import SupConLoss1
    p = sc.WIDTH_PROBLEMS[1]
    z1, z2, target, mask = sc.tensors(p)
    crit = criterion(mode, sc.GAMMA_INF)
    loss, ratio, g1, g2 = run(crit, z1, z2, target, mask)
    a, b = z1.to(DEV).requires_grad_(True), z2.to(DEV).requires_grad_(True)
    plain = SupConLoss1(temperature=sc.T)
    want = plain(a, b, target=target)
    (want * sc.GSCALE).backward()
    assert crit._last is not None and plain._last is not None
    check_loss(loss, want.item(), f"gamma = 1e10 ({mode}) against SupConLoss1", sc.TOL_PATHS)
    check(g1, a.grad, sc.TOL_GRAD, f"gamma = 1e10 ({mode}) dz1")
    check(g2, b.grad, sc.TOL_GRAD, f"gamma = 1e10 ({mode}) dz2")
    if mode == "hard":
        assert ratio == 1.0, ratio
    else:
        assert abs(ratio - 1.0) <= sc.RATIO_FLOOR, ratio


@pytest.mark.parametrize("mode", sc.MODES)
def test_two_runs_give_the_same_bits(mode):
    p = sc.BIG
    z1, z2, target, mask = sc.tensors(p)
    gamma = sc.gamma_of(p, mode)
    runs = [run(criterion(mode, gamma, True), z1, z2, target, mask) for _ in range(2)]
    assert runs[0][0].item() == runs[1][0].item() and runs[0][1] == runs[1][1]
    assert torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][3], runs[1][3])


def test_no_similarity_matrix_is_allocated():
    """R = 4096, D = 256: one deferred forward and backward stays below one R x R float32 matrix (64 MiB) above its
    inputs -- the workspace is 4 splits x 4096 x 256 x 4 B = 16 MiB"""
    n, D = sc.NOMAT_N, sc.NOMAT_D
    g = torch.Generator().manual_seed(5)
    z = torch.nn.functional.normalize(torch.randn(2 * n, D, generator=g), dim=1).to(DEV).requires_grad_(True)
    z1, z2 = torch.chunk(z, 2)
    target = [i % 7 for i in range(n)]
    crit = criterion("soft", 8.0, defer=True)
    crit(z1.detach(), z2.detach(), target=target)   # (label upload, LDS limits, the allocator's first blocks)
    crit.validate()
    del crit
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    crit = criterion("soft", 8.0, defer=True)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = crit(z1, z2, target=target)
    (loss * sc.GSCALE).backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"peak above the inputs: {extra / 2 ** 20:.1f} MiB (one R x R matrix: {(2 * n) ** 2 * 4 / 2 ** 20:.0f} MiB)")
    assert extra < (2 * n) ** 2 * 4
    assert z.grad is not None and bool(torch.isfinite(z.grad).all()) and isinstance(crit.downgrade_ratio, torch.Tensor)
    crit.validate()


def test_deferred_step_does_not_wait_for_the_device():
    p = sc.SIZE_PROBLEMS[1]
    z1, z2, target, _ = sc.tensors(p)
    a, b = z1.to(DEV).requires_grad_(True), z2.to(DEV).requires_grad_(True)
    up = torch.full((), sc.GSCALE, device=DEV)
    crit = criterion("soft", sc.gamma_of(p, "soft"), cg=True, defer=True)
    crit(a, b, target=target).backward(up)   # the label cache is warm from here on
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            loss = crit(a, b, target=target)
            loss.backward(up)
        ratio = crit.downgrade_ratio
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert isinstance(ratio, torch.Tensor) and ratio.dim() == 0 and ratio.is_cuda and not ratio.requires_grad
    assert loss.dim() == 0 and loss.is_cuda
    _, want, wratio, _, _ = oracle(p, "soft", True)
    check_loss(loss.detach(), want, "deferred loss")
    assert abs(ratio.item() - wratio) <= sc.RATIO_FLOOR
    crit.validate()
    assert crit._pending == []


def test_deferred_step_with_a_device_mask_does_not_wait():
    """the mask's codes are formed on the device: a mask that is already there costs no host wait either"""
    p = sc.MASK_PROBLEM
    z1, z2, _, mask = sc.tensors(p)
    a, b, m = z1.to(DEV).requires_grad_(True), z2.to(DEV).requires_grad_(True), mask.to(DEV)
    up = torch.full((), sc.GSCALE, device=DEV)
    crit = criterion("hard", sc.gamma_of(p, "hard"), defer=True)
    crit(a, b, mask=m).backward(up)   # (first launches)
    a.grad = b.grad = None
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = crit(a, b, mask=m)
        loss.backward(up)
        ratio = crit.downgrade_ratio
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    _, want, wratio, da, db = oracle(p, "hard", False)
    check_loss(loss.detach(), want, "deferred loss, device mask")
    assert isinstance(ratio, torch.Tensor) and abs(ratio.item() - wratio) <= sc.RATIO_FLOOR
    check(a.grad, da, sc.TOL_GRAD, "deferred dz1, device mask")
    check(b.grad, db, sc.TOL_GRAD, "deferred dz2, device mask")
    crit.validate()


def test_validate_raises_like_the_reference():
    p = sc.SIZE_PROBLEMS[1]
    z1, z2, target, _ = sc.tensors(p)
    gamma = sc.gamma_of(p, "soft")
    # not unit norm: AssertionError, deferred until validate() -- and inside forward by default
    crit = criterion("soft", gamma, defer=True)
    crit((1.01 * z1).to(DEV), z2.to(DEV), target=target)
    with pytest.raises(AssertionError, match="normalized"):
        crit.validate()
    crit.validate()   # the evidence is consumed
    with pytest.raises(AssertionError, match="normalized"):
        criterion("soft", gamma)((1.01 * z1).to(DEV), z2.to(DEV), target=target)
    # a row without a positive: NaN loss, RuntimeError
    mask = torch.eye(p.n, dtype=torch.int8)
    mask[3, 3] = 0
    crit = criterion("hard", gamma, defer=True)
    loss = crit(z1.to(DEV), z2.to(DEV), mask=mask.to(DEV))
    with pytest.raises(RuntimeError):
        crit.validate()
    assert bool(torch.isnan(loss))
    with pytest.raises(RuntimeError):
        criterion("hard", gamma)(z1.to(DEV), z2.to(DEV), mask=mask.to(DEV))


def test_matrices_on_demand():
    """sim_exp, sim_logits, pos_mask, neg_mask, sp_mask of the fused path against the composition's"""
    p = sc.MASK_PROBLEM
    z1, z2, target, mask = sc.tensors(p)
    for mode in sc.MODES:
        gamma = sc.gamma_of(p, mode)
        f, c = criterion(mode, gamma), criterion(mode, gamma)
        run(f, z1, z2, target, mask)
        run(c, z1, z2, target, mask, composition=True)
        assert f._mats is None and c._mats is not None
        assert torch.equal(f.pos_mask, c.pos_mask) and torch.equal(f.neg_mask, c.neg_mask)
        check(f.sim_exp, c.sim_exp, 1e-5, f"{mode} sim_exp")
        check(f.sim_logits, c.sim_logits, 1e-5, f"{mode} sim_logits")
        if mode == "hard":
            assert torch.equal(f.sp_mask, c.sp_mask), "the margin keeps every weight on its side"
        else:
            check(f.sp_mask, c.sp_mask, 1e-5, "soft sp_mask")
        assert f._mats is not None


def test_hook_step_does_not_wait_for_the_device(monkeypatch):
    """_SPINFONCEEpochHook inside a SemiSupervisedEpocher step (the setup of
    test_self_paced_infonce_hook_gamma_schedule_and_loss): the hook call runs under sync-debug "error"; loss and
    sp_weight meters against the oracle"""
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import EpocherHook, TrainerHook
    from oracle import losses as ol
    from oracle import next_rows as onr
    from oracle import unet as ou
    from semi_seg.augment import AffineAugment
    from semi_seg.hooks import PScheduler, create_sp_infonce_hooks
    from semi_seg.hooks.infonce import _SPINFONCEEpochHook
    from contrastyou.losses.kl import KL_div
    from contrastyou.optim import RAdam
    from semi_seg.epochers import SemiSupervisedEpocher
    from tests.test_gpu_hooks_dice import Loader, blob_batch

    def _semi_epocher(model, hook_module, lab, unl, epoch):
        opt = RAdam([{"params": list(model.parameters())}, {"params": list(hook_module.parameters())}], lr=1e-3)
        ep = SemiSupervisedEpocher(model=model, optimizer=opt, labeled_loader=Loader([lab]), unlabeled_loader=Loader([unl]),
                                   sup_criterion=KL_div(), num_batches=1, cur_epoch=epoch, device=DEV, two_stage=True,
                                   disable_bn=False, scaler=torch.amp.GradScaler("cuda", enabled=False), accumulate_iter=1)
        ep.init()
        return ep

    calls = []
    inner = _SPINFONCEEpochHook._call_implementation

    def guarded(self, **kwargs):
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = inner(self, **kwargs)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        calls.append(self._criterion.downgrade_ratio)
        return out

    monkeypatch.setattr(_SPINFONCEEpochHook, "_call_implementation", guarded)
    g = torch.Generator().manual_seed(4)
    n, hw, K = sc.HOOK["n"], sc.HOOK["hw"], sc.HOOK["K"]
    sd0 = ou.init_state_dict(1, K, sc.HOOK["channels"], seed=5)
    lab, unl = blob_batch(n, hw, K, g), blob_batch(n, hw, K, g)
    unl["img"] = [unl["img"][0], torch.rand(n, 1, hw, hw, generator=g)]
    model = UNet(input_dim=1, num_classes=K, max_channel=sc.HOOK["channels"], momentum=0.01)
    model.load_state_dict(sd0)
    model.to(DEV)
    type(TrainerHook).names.clear()
    trainer_hook = create_sp_infonce_hooks(model=model, feature_names="Conv5", weights=0.7, contrast_ons="partition",
                                           data_name="acdc", begin_values=6.0, end_values=2.0, mode="soft", p=0.5,
                                           max_epoch=4, correct_grad=False).to(DEV)
    sp_hook = trainer_hook._hooks[0]
    ref_sched = PScheduler(max_epoch=4, begin_value=6.0, end_value=2.0, p=0.5)
    for epoch in range(2):
        psd = {k: v.detach().cpu().clone() for k, v in sp_hook._projector.state_dict().items()}
        ep = _semi_epocher(model, trainer_hook, lab, unl, epoch)
        tap = {}

        class Spy(EpocherHook):
            def _call_implementation(self, *, seed, partition_group, label_group, **kw):
                tap["seed"], tap["partition"], tap["group"] = seed, list(partition_group), list(label_group)
                tap["conv5"] = sp_hook._extractor.feature()[-2 * n:].detach().float().cpu()
                return torch.zeros((), device=DEV)

        random.seed(21 + epoch)
        with ep.register_hook(trainer_hook(), Spy(name=f"sp_spy{epoch}")):
            ep.run()
        torch.cuda.synchronize()
        assert len(calls) == epoch + 1 and isinstance(calls[-1], torch.Tensor) and calls[-1].is_cuda, "a device scalar"
        assert sp_hook._criterion.defer_checks is False and sp_hook._criterion._pending == [], "validated at close()"
        stats = ep.get_metric()
        gamma = float(ref_sched.value)
        ref_sched.step()
        key = "spinfoce/Conv5/partition"
        assert abs(stats[key]["age_param"] - gamma) < 1e-9, (epoch, stats[key], gamma)
        theta = torch.from_numpy(AffineAugment().sample(n, tap["seed"])[0])
        f_u, f_utf = torch.chunk(tap["conv5"], 2, 0)
        z = ol.projection_head(psd, torch.cat([ol.affine_nearest(f_u, theta), f_utf], 0))
        z1, z2 = torch.chunk(z, 2, 0)
        target = ol.get_label("partition", "acdc", tap["partition"], tap["group"])
        want, ratio = onr.self_paced_supcon(z1, z2, list(target), gamma=gamma, weight_update="soft")
        print(f"epoch {epoch}: loss {stats[key]['loss']!r} vs {want.item()!r}, sp_weight {stats[key]['sp_weight']!r} vs {ratio!r}")
        assert abs(stats[key]["loss"] - want.item()) < 3e-4 * abs(want.item()), (epoch, stats[key], want.item())
        assert abs(stats[key]["sp_weight"] - ratio) < 1e-4, (epoch, stats[key], ratio)
    type(TrainerHook).names.clear()
