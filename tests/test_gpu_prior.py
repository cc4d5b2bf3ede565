"""The DAE-prior and orthogonality kernels (csrc/cy_prior.hip), their autograd functions and hooks on the GPU, against
float64 torch on the CPU (tests/prior_cases.py) and, for the hooks, against the reference's own values
(tests/golden/prior.npz, written by tests/golden/gen_goldens_prior.py).

Bounds: prior_cases.bounds -- for each kind (loss; gradient in 2-norm and in max-norm, relative to the float64
gradient's own norm) four times the largest distance of the reference's f32 composition from float64 over the same
cases, a loss floored at 1.2e-6.  Against the reference's recorded f32 values the bound is one e_ref wider (both sides
are then away from float64).  Every figure is printed before it is asserted."""
import functools
import random

import numpy as np
import pytest
import torch

import prior_cases as pc
from step_harness import OneBatchLoader
from test_gpu_hooks_dice import Loader, blob_batch
from test_gpu_semi_baselines import _Epocher

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def npz(golden_dir):
    return pc.load(golden_dir)


@functools.lru_cache(maxsize=None)
def dae_ref(tag):
    return pc.dae_reference(pc.DAE_BY_TAG[tag])


@functools.lru_cache(maxsize=None)
def ortho_ref(tag):
    return pc.ortho_reference(pc.ORTHO_BY_TAG[tag])


@functools.lru_cache(maxsize=None)
def dae_bounds():
    b = pc.bounds([dae_ref(c.tag) for c in pc.DAE_CASES])
    print("DAE bounds (e_ref, bound):", {k: (f"{e:.3g}", f"{t:.3g}") for k, (e, t) in b.items()})
    return b


@functools.lru_cache(maxsize=None)
def ortho_bounds():
    b = pc.bounds([ortho_ref(c.tag) for c in pc.ORTHO_CASES])
    print("orthogonality bounds (e_ref, bound):", {k: (f"{e:.3g}", f"{t:.3g}") for k, (e, t) in b.items()})
    return b


def check(name, bounds, value, grads, value64, grads64, extra=0.0):
    """`extra`: how many e_ref the comparison's other side is itself away from float64 (the recorded f32 values: 1)"""
    value = value.detach() if torch.is_tensor(value) else value
    e = pc.errors(value, grads, value64, grads64) if grads64 is not None else [pc.rel_scalar(value, value64), 0.0, 0.0]
    lim = [bounds[k][1] + extra * bounds[k][0] for k in pc.KINDS]
    print(f"{name}: loss {e[0]:.3g} (<= {lim[0]:.3g})  grad2 {e[1]:.3g} (<= {lim[1]:.3g})  "
          f"gradmax {e[2]:.3g} (<= {lim[2]:.3g})")
    assert np.isfinite(float(value)) and all(bool(torch.isfinite(g).all()) for g in grads)
    assert e[0] <= lim[0] and e[1] <= lim[1] and e[2] <= lim[2], (name, e, lim)
    return e


def place(z, layout):
    """the logits [N,K,H,W] on the GPU as a leaf: "nchw" contiguous, "cl" channels-last, "slice" NHWC rows that start
    one float into a larger buffer (a base that is only 4-byte aligned)"""
    if layout == "nchw":
        t = z.to(DEV).contiguous()
    elif layout == "cl":
        t = z.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    else:
        N, K, H, W = z.shape
        buf = torch.full((z.numel() + 9,), 777.25, device=DEV)
        t = buf[1:1 + z.numel()].view(N, H, W, K).permute(0, 3, 1, 2)
        t.copy_(z)
        assert t.data_ptr() % 16 == 4
        t._guard = buf  # (checked by the caller: the kernels only read the logits)
    return t.requires_grad_(True)


@functools.lru_cache(maxsize=None)
def run_dae(tag):
    """two runs of DAELossFn forward + backward on the case -> [(loss, [dlogits, dw, db]) x 2], on the CPU"""
    from cyhip.functions import DAELossFn
    case = pc.DAE_BY_TAG[tag]
    z, w, b, img = pc.dae_inputs(case)
    runs = []
    for _ in range(2):
        zd = place(z, case.layout)
        wd = w.view(1, case.K, 1, 1).to(DEV).requires_grad_(True)
        bd = b.to(DEV).requires_grad_(True)
        loss = DAELossFn.apply(zd, wd, bd, img.to(DEV), case.act)
        loss.backward()
        torch.cuda.synchronize()
        if case.layout == "slice":
            assert float(zd._guard[0]) == 777.25 and bool((zd._guard[1 + z.numel():] == 777.25).all())
            assert torch.equal(zd.detach().cpu(), z)
        runs.append((loss.detach().cpu(), [zd.grad.cpu().contiguous(), wd.grad.cpu().view(-1), bd.grad.cpu()]))
    return runs


@functools.lru_cache(maxsize=None)
def run_ortho(tag):
    from cyhip import ops
    from cyhip.functions import OrthoLossFn
    case = pc.ORTHO_BY_TAG[tag]
    v = pc.ortho_inputs(case)
    runs = []
    for _ in range(2):
        if case.zero:  # forward only: the reference scales this row's gradient by 1e12
            loss, grads = ops.ortho_fwd(v.reshape(case.K, case.C).to(DEV).contiguous()), []
        else:
            vd = v.to(DEV).requires_grad_(True)
            loss = OrthoLossFn.apply(vd)
            loss.backward()
            assert vd.grad.shape == v.shape
            grads = [vd.grad.cpu()]
        torch.cuda.synchronize()
        runs.append((loss.detach().cpu(), grads))
    return runs


# ---------------------------------------------------------------------------------------------- 1. DAE kernels
@pytest.mark.parametrize("case", pc.DAE_CASES, ids=lambda c: c.tag)
def test_dae_loss_and_gradients_against_float64(case):
    from cyhip import ops
    plan = ops.prior_plan("dae", case.K, case.Cimg, case.N * case.H * case.W, align=4 if case.layout == "slice" else 16)
    print(case.tag, plan)
    v64, g64, e_ref = dae_ref(case.tag)
    loss, grads = run_dae(case.tag)[0]
    g64 = [g64[0], g64[1].reshape(-1), g64[2]]
    assert grads[0].shape == g64[0].shape
    check(case.tag, dae_bounds(), loss, grads, v64, g64)
    print(f"{case.tag}: the f32 composition's own errors {[f'{x:.3g}' for x in e_ref]}")
    if case.reach >= 30 and case.act == "sigmoid":
        # saturated pixels: r (1 - r) underflows cleanly to 0 -- some rows of dlogits are exactly 0, none is not finite
        rows = grads[0].movedim(1, -1).reshape(-1, case.K)
        assert int((rows == 0).all(1).sum()) > 0 and int((rows != 0).any(1).sum()) > 0


def test_dae_two_runs_give_the_same_bits():
    for case in pc.DAE_CASES:
        (l1, g1), (l2, g2) = run_dae(case.tag)
        assert torch.equal(l1, l2), case.tag
        assert all(torch.equal(a, b) for a, b in zip(g1, g2)), case.tag


def test_dae_upstream_gradient_and_the_image_carries_none():
    """the upstream gradient is a device scalar: weight * loss scales every gradient; the image gets no gradient"""
    from cyhip.functions import DAELossFn
    case = pc.DAE_BY_TAG["k5_70_c2"]
    z, w, b, img = pc.dae_inputs(case)
    zd, wd, bd = place(z, "cl"), w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    imd = img.to(DEV).requires_grad_(True)
    (DAELossFn.apply(zd, wd, bd, imd, case.act) * -2.5).backward()
    assert imd.grad is None
    v64, g64, _ = dae_ref(case.tag)
    check("upstream -2.5", dae_bounds(), 0.0, [zd.grad, wd.grad, bd.grad], 0.0, [-2.5 * g for g in g64])
    with pytest.raises(ValueError, match="activation"):
        DAELossFn.apply(zd, wd, bd, imd, "relu")
    with pytest.raises(ValueError, match="one channel"):
        DAELossFn.apply(zd, torch.zeros(2, case.K, 1, 1, device=DEV), bd, imd, "sigmoid")


# ---------------------------------------------------------------------------------------------- 2. orthogonality
@pytest.mark.parametrize("case", pc.ORTHO_CASES, ids=lambda c: c.tag)
def test_ortho_loss_and_gradient_against_float64(case):
    from cyhip import ops
    print(case.tag, ops.prior_plan("ortho", case.K, case.C))
    v64, g64, e_ref = ortho_ref(case.tag)
    loss, grads = run_ortho(case.tag)[0]
    check(case.tag, ortho_bounds(), loss, grads, v64, g64)
    print(f"{case.tag}: the f32 composition's own errors {[f'{x:.3g}' for x in e_ref]}")


def test_ortho_two_runs_give_the_same_bits_and_both_ranks_agree():
    from cyhip.functions import OrthoLossFn
    for case in pc.ORTHO_CASES:
        (l1, g1), (l2, g2) = run_ortho(case.tag)
        assert torch.equal(l1, l2), case.tag
        assert all(torch.equal(a, b) for a, b in zip(g1, g2)), case.tag
    case = pc.ORTHO_BY_TAG["k12_c16"]
    v4 = pc.ortho_inputs(case)
    v2 = v4.reshape(case.K, case.C).to(DEV).requires_grad_(True)
    OrthoLossFn.apply(v2).backward()
    loss, grads = run_ortho(case.tag)[0]
    assert torch.equal(v2.grad.cpu().view_as(grads[0]), grads[0])
    with pytest.raises(ValueError, match="prototypes"):
        OrthoLossFn.apply(torch.zeros(4, 8, 2, 2, device=DEV))


# ---------------------------------------------------------------------------------------------- 3. the hooks
@pytest.mark.parametrize("h", pc.HOOK_DAE, ids=lambda h: h["tag"])
def test_dae_epocher_hook_against_the_reference(npz, h):
    from semi_seg.hooks import AuxiliaryLayer
    from semi_seg.hooks.autoencoder import DenoisingAutoEncoderEpocherHook
    tag, K = h["tag"], h["K"]
    layer = AuxiliaryLayer(in_features=K)
    layer.load_state_dict({"fc.weight": torch.from_numpy(npz[f"aux_k{K}_weight"]),
                           "fc.bias": torch.from_numpy(npz[f"aux_k{K}_bias"])}, strict=True)
    layer.to(DEV)
    z = torch.from_numpy(npz[f"{tag}_z_i8d8"].astype(np.float32) / 8)
    img = torch.from_numpy(npz[f"{tag}_image"])
    zd = z.to(DEV).requires_grad_(True)
    ep = _Epocher()
    hook = ep.adopt(DenoisingAutoEncoderEpocherHook(extra_layer=layer, weight=h["weight"]))
    assert hook.name == "deAE"
    value = hook(unlabeled_image_tf=img.to(DEV), unlabeled_tf_logits=zd, seed=1)
    value.backward()
    grads = [zd.grad, layer.fc.weight.grad, layer.fc.bias.grad]
    v64, g64 = pc.grads_of(lambda a, c, d, e: h["weight"] * pc.dae64(a, c, d, e, "sigmoid"), z,
                           layer.fc.weight.detach().cpu(), layer.fc.bias.detach().cpu(), img, wrt=(0, 1, 2))
    check(f"{tag} vs f64", dae_bounds(), value, grads, v64, g64)
    recorded = [torch.from_numpy(npz[f"{tag}_g_{n}"]) for n in ("logits", "weight", "bias")]
    check(f"{tag} vs the reference", dae_bounds(), value, grads, npz[f"{tag}_value"], recorded, extra=1.0)
    meter = ep.summary(hook)["ls"]
    assert pc.rel_scalar(meter, npz[f"{tag}_meter"][0]) <= dae_bounds()["loss"][1] + dae_bounds()["loss"][0]


@pytest.mark.parametrize("h", pc.HOOK_ORTHO, ids=lambda h: h["tag"])
def test_orthogonal_epocher_hook_against_the_reference(npz, h):
    from semi_seg.hooks.orthogonal import _OrthogonalEpocherHook
    tag = h["tag"]
    v = torch.from_numpy(npz[f"{tag}_v"])
    p = torch.nn.Parameter(v.to(DEV))
    ep = _Epocher()
    hook = ep.adopt(_OrthogonalEpocherHook(name="orth", prototypes=p, weight=h["weight"]))
    value = hook(seed=1)
    value.backward()
    assert p.grad.shape == v.shape
    v64, g64 = pc.grads_of(lambda a: h["weight"] * pc.ortho64(a), v, wrt=(0,))
    check(f"{tag} vs f64", ortho_bounds(), value, [p.grad], v64, g64)
    check(f"{tag} vs the reference", ortho_bounds(), value, [p.grad], npz[f"{tag}_value"],
          [torch.from_numpy(npz[f"{tag}_g_v"])], extra=1.0)
    meter = ep.summary(hook)["loss"]
    assert pc.rel_scalar(meter, npz[f"{tag}_meter"][0]) <= ortho_bounds()["loss"][1] + ortho_bounds()["loss"][0]
    # a second backward adds into the live .grad buffer (the path a parameter of the flat optimizer takes)
    first = p.grad.clone()
    hook(seed=1).backward()
    assert torch.equal(p.grad, first + first)


def test_auxiliary_layer_forward_takes_the_head_kernels():
    from cyhip._lib import HipKernelError
    from semi_seg.hooks import AuxiliaryLayer
    torch.manual_seed(5)
    for act in ("sigmoid", "tanh"):
        layer = AuxiliaryLayer(in_features=8, activation=act)
        x = torch.randn(2, 8, 5, 7)
        want = getattr(torch, act)(torch.nn.functional.conv2d(x.double(), layer.fc.weight.double(), layer.fc.bias.double()))
        got = layer.to(DEV)(x.to(DEV))
        assert got.shape == (2, 1, 5, 7) and float((got.cpu().double() - want).abs().max()) <= 1e-6
    # the head kernels take channel counts that are multiples of 8; anything else is an error, never an eager fallback
    with pytest.raises(HipKernelError, match="CY_ERR_SHAPE"):
        AuxiliaryLayer(in_features=4).to(DEV)(torch.zeros(1, 4, 4, 4, device=DEV))


# ---------------------------------------------------------------------------------------------- 4. training steps
class _StepTrainer:
    def __init__(self, model, max_epoch):
        self._model, self._max_epoch = model, max_epoch


def test_a_semi_supervised_step_with_the_dae_hook():
    """one step with the default switches: the layer's weight moves, and the metered loss is the float64 value of the
    formula on the logits and the image the hook was handed"""
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import EpocherHook, TrainerHook
    from contrastyou.losses.kl import KL_div
    from contrastyou.optim import RAdam
    from oracle import unet as ou
    from semi_seg.epochers import SemiSupervisedEpocher
    from semi_seg.hooks import DenoisingAutoEncoderTrainerHook
    K = pc.STEP_DAE["K"]
    sd0 = ou.init_state_dict(1, K, 128, seed=14)
    g = torch.Generator().manual_seed(21)
    lab, unl = [blob_batch(4, 32, K, g)], [blob_batch(4, 32, K, g)]
    type(TrainerHook).names.clear()
    try:
        model = UNet(input_dim=1, num_classes=K, max_channel=128, momentum=0.1)
        model.load_state_dict(sd0)
        model.to(DEV)
        trainer = _StepTrainer(model, max_epoch=10)
        torch.manual_seed(3)
        hook = DenoisingAutoEncoderTrainerHook(hook_name="dae_step", num_classes=K, weight=pc.STEP_DAE["weight"]).to(DEV)
        hook.register_trainer(trainer)
        w0 = hook.aux_layer.fc.weight.detach().cpu().clone()
        b0 = hook.aux_layer.fc.bias.detach().cpu().clone()
        opt = RAdam([{"params": list(model.parameters())}, {"params": list(hook.parameters())}], lr=3e-3,
                    weight_decay=1e-4)
        ep = SemiSupervisedEpocher(model=model, optimizer=opt, labeled_loader=Loader(lab), unlabeled_loader=Loader(unl),
                                   sup_criterion=KL_div(), num_batches=1, cur_epoch=0, device=DEV, two_stage=True,
                                   disable_bn=False, scaler=torch.amp.GradScaler("cuda", enabled=False),
                                   accumulate_iter=1)
        ep.init(trainer)
        seen = {}

        class Spy(EpocherHook):
            def _call_implementation(self, *, unlabeled_tf_logits, unlabeled_image_tf, **kw):
                seen["z"], seen["img"] = unlabeled_tf_logits.detach().float().cpu(), unlabeled_image_tf.detach().cpu()
                return torch.zeros((), device=DEV)

        random.seed(9)
        with ep.register_hook(hook(), Spy(name="spy")):
            ep.run()
        torch.cuda.synchronize()
        metric = ep.get_metric()
        w1 = hook.aux_layer.fc.weight.detach().cpu()
        want = float(pc.dae64(seen["z"], w0, b0, seen["img"], "sigmoid"))
        got = metric["deAE"]["ls"]
        print("deAE ls", got, "f64", want, "reg_loss", metric["semi"]["reg_loss"])
        assert pc.rel_scalar(got, want) <= dae_bounds()["loss"][1]
        assert pc.rel_scalar(metric["semi"]["reg_loss"], pc.STEP_DAE["weight"] * want) <= 2 * dae_bounds()["loss"][1]
        assert not torch.equal(w1, w0) and bool(torch.isfinite(w1).all())
        assert not torch.equal(hook.aux_layer.fc.bias.detach().cpu(), b0)
        assert all(bool(torch.isfinite(v).all()) for v in model.state_dict().values())
    finally:
        type(TrainerHook).names.clear()


def _multicore_step(tmp_path, weight):
    """one MulticoreTrainer step (one epoch of one batch) -> (the head weight before the step, its gradient after)"""
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.losses.multicore_loss import MultiCoreKL
    from multicore_fixture import groups_of
    from semi_seg.hooks import OrthogonalTrainerHook, create_consistency_hook
    from semi_seg.trainers.features import MulticoreTrainer
    Ct, M = pc.STEP_ORTHO["true_classes"], pc.STEP_ORTHO["multiplier"]
    g = torch.Generator().manual_seed(31)
    lab, unl = blob_batch(2, 32, Ct, g), blob_batch(3, 32, Ct, g)
    val = {k: v[0] for k, v in blob_batch(2, 32, Ct, g, views=1).items()}
    cfg = {"Arch": {"true_num_classes": Ct, "max_channel": 128},
           "Optim": {"name": "RAdam", "lr": 1e-4, "weight_decay": 1e-5},
           "Scheduler": {"multiplier": 100, "warmup_max": 1}, "Trainer": {"name": "semi"}}
    type(TrainerHook).names.clear()
    tmp_path.mkdir(parents=True, exist_ok=True)
    try:
        torch.manual_seed(12)
        random.seed(4)
        model = UNet(input_dim=1, num_classes=Ct * M, max_channel=128)
        head = model._Deconv_1x1.weight
        before = head.detach().clone()
        tr = MulticoreTrainer(model=model, labeled_loader=OneBatchLoader(lab), unlabeled_loader=OneBatchLoader(unl),
                              val_loader=OneBatchLoader(val), test_loader=OneBatchLoader(val),
                              criterion=MultiCoreKL(groups_of(Ct, M)), save_dir=str(tmp_path), max_epoch=1,
                              num_batches=1, device=DEV, disable_bn=False, two_stage=True, config=cfg,
                              enable_scale=False)
        hooks = [create_consistency_hook(0.1)]
        if weight is not None:
            hooks.append(OrthogonalTrainerHook(hook_name="orth", prototypes=head, weight=weight))
        with tr.register_hook(*hooks):
            tr.init()
            tr.start_training()
        torch.cuda.synchronize()
        assert model._Deconv_1x1.weight is head and head.grad is not None
        assert not torch.equal(head.detach().cpu(), before)
        return before, head.grad.detach().cpu().clone()
    finally:
        type(TrainerHook).names.clear()


def test_a_multicore_step_adds_the_orthogonality_gradient_to_the_head(tmp_path):
    """with the step's default switches: the head weight's gradient with the hook is the one without it plus
    weight * the float64 orthogonality gradient of the weight the step started from.  The two steps differ in nothing
    else, and each element of the sum is rounded to f32 once more: 2^-23 of the largest gradient entry is allowed for."""
    weight = pc.STEP_ORTHO["weight"]
    before, with_hook = _multicore_step(tmp_path / "a", weight)
    before2, without = _multicore_step(tmp_path / "b", None)
    assert torch.equal(before, before2) and before.shape[0] == 4 and before.dim() == 4
    _, g64 = pc.grads_of(pc.ortho64, before, wrt=(0,))
    added = (with_hook.double() - without.double())
    want = weight * g64[0]
    err = float((added - want).abs().max())
    lim = ortho_bounds()["gradmax"][1] * float(want.abs().max()) + 2.0 ** -23 * float(without.abs().max())
    print(f"head gradient: |added - weight g64|_max {err:.3g} (<= {lim:.3g}); |weight g64|_max "
          f"{float(want.abs().max()):.3g}, |gradient without|_max {float(without.abs().max()):.3g}")
    assert float(want.abs().max()) > 0 and err <= lim
