"""The MixUp / ICT kernels (csrc/cy_mixup.hip), their autograd functions, hooks, epocher and trainer on the GPU, against
tests/golden/mixup.npz (the reference in f32 and f64, tests/golden/gen_goldens_mixup.py) and against the f64 restatement
of tests/mixup_fixture.py on the CPU, on the cases of tests/mixup_cases.py.

Tolerance: max(4 * the reference's own largest f32-to-f64 distance of that kind over the fixture, 1e-6), read from the
npz: 1.19e-6 for a loss, 1.0e-6 for a gradient's 2-norm, 2.91e-6 for its max-norm, all relative.  No element is left
out of any comparison, and every figure is printed before it is asserted.  The mixed images are held to the bits of
torch's CPU f32 evaluation.
"""
import random

import numpy as np
import pytest
import torch

import mixup_cases as mc
import mixup_fixture as fx
from test_gpu_hooks_dice import Loader, blob_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
UP = 0.7  # the upstream gradient of every backward here (not 1: the kernels read it)


@pytest.fixture(scope="module")
def npz(golden_dir):
    return fx.load(golden_dir)


@pytest.fixture(scope="module")
def tol(npz):
    t = fx.tolerances(npz)
    print("tolerances", t)
    return t


_REF64 = {}


def ref64(npz, case, which):
    """(loss, gradient) of the f64 restatement, computed once per case and left unchanged"""
    key = (case.tag, which)
    if key not in _REF64:
        s, t, y, index, (w_self, w_other) = fx.case_inputs(npz, case)
        if which == "kl":
            _REF64[key] = fx.grad_of(fx.mixkl64, s, y, index, w_self, w_other)
        else:
            _REF64[key] = fx.grad_of(fx.mixmse64, s, t, index, w_self, w_other)
    return _REF64[key]


def run_loss(npz, case, which, channels_last=True):
    """forward and backward of the autograd function on the GPU -> (loss, d(UP * loss)/dlogits) on the CPU"""
    from cyhip.functions import MixSoftmaxMSEFn, MixupKLFn
    s, t, y, index, (w_self, w_other) = fx.case_inputs(npz, case)
    z = s.to(DEV)
    if channels_last:
        z = z.contiguous(memory_format=torch.channels_last)
    z.requires_grad_(True)
    if which == "kl":
        loss = MixupKLFn.apply(z, y.to(DEV), index, w_self, w_other, fx.EPS)
    else:
        loss = MixSoftmaxMSEFn.apply(z, t.to(DEV), index, w_self, w_other)
    (UP * loss).backward()
    assert loss.shape == () and loss.is_cuda and z.grad.shape == z.shape
    return loss.detach().cpu(), z.grad.detach().cpu()


def check(name, v, g, v64, g64, tol, up=UP):
    d = fx.distances(v, g, v64, up * torch.as_tensor(g64, dtype=torch.float64))
    print(name, {k: f"{x:.3e}" for k, x in d.items()})
    assert torch.isfinite(torch.as_tensor(v)).all() and torch.isfinite(g).all()
    for kind in fx.KINDS:
        assert d[kind] <= tol[kind], (name, kind, d[kind], tol[kind])


# ---- images ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.IMAGE_CASES, ids=lambda c: c.tag)
def test_mixed_images_are_bit_equal_to_torch_cpu(npz, case):
    from cyhip import ops
    x = torch.from_numpy(mc.image_values(case))
    index = fx.index_of(npz, case.index, case.N)
    w_self, w_other = fx.weights_of(npz, case.weights)
    want = w_self * x + w_other * x[index, :]  # the reference's expression: Python f64 weights on an f32 tensor
    assert want.dtype == torch.float32
    if case.base == "slice":
        buf = torch.zeros(case.N * case.E + 1, device=DEV)
        xd = buf[1:].view(case.N, case.E)
        xd.copy_(x)
        assert xd.data_ptr() % 16 == 4
    else:
        xd = x.to(DEV)
    plan = ops.mix_plan("images", case.N, case.E, align=16 if xd.data_ptr() % 16 == 0 else 4)
    got = ops.mix_images(xd, index, w_self, w_other)
    print(case.tag, plan)
    assert got.shape == xd.shape and got.data_ptr() != xd.data_ptr()
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    assert torch.equal(xd.cpu(), x)  # the input is left alone
    again = ops.mix_images(xd, ops.mix_index(index, case.N, DEV), w_self, w_other)  # an uploaded index is taken as it is
    assert torch.equal(again, got)


def test_mixed_images_keep_the_memory_format(npz):
    from cyhip import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 3, 19, 19, generator=g)
    index, (w_self, w_other) = torch.tensor(mc.FIXED), fx.weights_of(npz, mc.DRAW_A1)
    want = w_self * x + w_other * x[index, :]
    for fmt in (torch.contiguous_format, torch.channels_last):
        got = ops.mix_images(x.to(DEV).contiguous(memory_format=fmt), index, w_self, w_other)
        assert got.is_contiguous(memory_format=fmt) and torch.equal(got.cpu(), want)
    strided = x.to(DEV)[:, :, ::2]  # neither format: mixed from a contiguous copy
    assert torch.equal(ops.mix_images(strided, index, w_self, w_other).cpu(), want[:, :, ::2])


def test_mixup_data_mixes_images_and_float_targets(npz):
    from contrastyou.utils.utils import fix_all_seed_within_context
    from semi_seg.hooks.utils import mixup_data
    g = torch.Generator().manual_seed(6)
    x, y = torch.randn(6, 1, 19, 19, generator=g), torch.rand(6, 4, 19, 19, generator=g)
    lam, index = fx.recorded_draw(npz, 3, 6, 0.2)
    with fix_all_seed_within_context(3):
        mx, my = mixup_data(x.to(DEV), y.to(DEV), alpha=0.2, device=DEV)
    index = torch.tensor(index)
    assert torch.equal(mx.cpu(), lam * x + (1 - lam) * x[index, :])
    assert torch.equal(my.cpu(), lam * y + (1 - lam) * y[index, :])


# ---- the two losses ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["kl", "mse"])
@pytest.mark.parametrize("case", mc.LOSS_CASES, ids=lambda c: c.tag)
def test_losses_against_f64_and_the_reference(npz, tol, case, which):
    from cyhip import ops
    print(case.tag, which, ops.mix_plan("mix" + which, case.N, case.H * case.W, case.K))
    v, g = run_loss(npz, case, which)
    v64, g64 = ref64(npz, case, which)
    check(f"{case.tag} {which} vs f64", v, g, v64, g64, tol)
    if case.golden:
        check(f"{case.tag} {which} vs reference", v, g, npz[f"{case.tag}_{which}64"], npz[f"{case.tag}_g{which}64"], tol)
    # two runs give the same bits, forward and backward
    v2, g2 = run_loss(npz, case, which)
    assert torch.equal(v, v2) and torch.equal(g, g2)


@pytest.mark.parametrize("which", ["kl", "mse"])
def test_nchw_logits_give_the_same_bits(npz, which):
    case = mc.LOSS_BY_TAG["k5_19_draw"]
    v, g = run_loss(npz, case, which)
    v2, g2 = run_loss(npz, case, which, channels_last=False)
    assert torch.equal(v, v2) and torch.equal(g, g2)


@pytest.mark.parametrize("K", [2, 8])
def test_compiled_class_counts_on_a_4_byte_aligned_base(npz, tol, K):
    """the rows of K = 2 / 8 are read 8 / 16 bytes at a time only where the base allows it; one float into a buffer
    the run-time kernel takes over (cy_mix_plan: kt = 0)"""
    from cyhip import ops
    case = mc.LOSS_BY_TAG["k2_19_fixed" if K == 2 else "k8_19_draw"]
    s, t, y, index, (w_self, w_other) = fx.case_inputs(npz, case)
    N, H, W = case.N, case.H, case.W

    def off_base(src):
        buf = torch.zeros(N * H * W * K + 1, device=DEV)
        view = buf[1:].view(N, H, W, K).permute(0, 3, 1, 2)
        view.copy_(src)
        assert view.data_ptr() % 8 == 4 and ops.is_nhwc(view)
        return view

    zs, zt, yd, up = off_base(s), off_base(t), y.to(DEV), torch.tensor([UP], device=DEV)
    v = ops.softmax_mixkl_fwd(zs, yd, index, w_self, w_other, fx.EPS)
    g = ops.softmax_mixkl_bwd(zs, yd, index, w_self, w_other, up, fx.EPS)
    check(f"K={K} off-base kl", v.cpu(), g.cpu(), *ref64(npz, case, "kl"), tol)
    v = ops.softmax_mixmse_fwd(zs, zt, index, w_self, w_other)
    g = ops.softmax_mixmse_bwd(zs, zt, index, w_self, w_other, up)
    check(f"K={K} off-base mse", v.cpu(), g.cpu(), *ref64(npz, case, "mse"), tol)


def test_unit_weights_reproduce_the_unmixed_kernels(npz, tol):
    """(1, 0) with any index: the plain softmax + KL against the own labels, and the softmax-pair MSE against the
    unmixed teacher"""
    from cyhip import ops
    case = mc.LOSS_BY_TAG["k5_19_draw"]
    s, t, y, _, _ = fx.case_inputs(npz, case)
    zs = s.to(DEV).contiguous(memory_format=torch.channels_last)
    zt = t.to(DEV).contiguous(memory_format=torch.channels_last)
    yd, up = y.to(DEV), torch.tensor([UP], device=DEV)
    for index in (torch.tensor([1, 1, 3, 0, 5, 5]), fx.index_of(npz, mc.DRAW6, 6)):
        v = ops.softmax_mixkl_fwd(zs, yd, index, 1.0, 0.0, fx.EPS)
        g = ops.softmax_mixkl_bwd(zs, yd, index, 1.0, 0.0, up, fx.EPS)
        v0, g0 = ops.softmax_kl_fwd(zs, yd, fx.EPS), ops.softmax_kl_bwd(zs, yd, up, fx.EPS)
        check("kl (1, 0) vs softmax_kl", v.cpu(), g.cpu(), v0.double().cpu(), g0.double().cpu() / UP, tol)
        check("kl (1, 0) vs f64", v.cpu(), g.cpu(), *fx.grad_of(fx.mixkl64, s, y, index, 1.0, 0.0), tol)
        v = ops.softmax_mixmse_fwd(zs, zt, index, 1.0, 0.0)
        g = ops.softmax_mixmse_bwd(zs, zt, index, 1.0, 0.0, up)
        v0 = ops.softmax_mse_fwd(zs, zt)
        g0, _ = ops.softmax_mse_bwd(zs, zt, up, True, False)
        check("mse (1, 0) vs softmax_mse", v.cpu(), g.cpu(), v0.double().cpu(), g0.double().cpu() / UP, tol)
    # (0, 1) is the partner's label alone
    index = torch.tensor([1, 1, 3, 0, 5, 5])
    v = ops.softmax_mixkl_fwd(zs, yd, index, 0.0, 1.0, fx.EPS)
    g = ops.softmax_mixkl_bwd(zs, yd, index, 0.0, 1.0, up, fx.EPS)
    yp = y[index].to(DEV).contiguous()
    check("kl (0, 1) vs softmax_kl on the partner's labels", v.cpu(), g.cpu(),
          ops.softmax_kl_fwd(zs, yp, fx.EPS).double().cpu(), ops.softmax_kl_bwd(zs, yp, up, fx.EPS).double().cpu() / UP,
          tol)


def test_an_index_out_of_range_raises_before_anything_runs(npz):
    from cyhip import ops
    from cyhip.functions import MixSoftmaxMSEFn, MixupKLFn
    z = torch.zeros(2, 3, 4, 4, device=DEV)
    y = torch.zeros(2, 4, 4, dtype=torch.int64, device=DEV)
    for bad in (torch.tensor([0, 2]), torch.tensor([-1, 0]), torch.tensor([2 ** 31, 0])):
        with pytest.raises(ValueError):
            ops.mix_images(z, bad, 0.5, 0.5)
        with pytest.raises(ValueError):
            MixupKLFn.apply(z, y, bad, 0.5, 0.5, fx.EPS)
        with pytest.raises(ValueError):
            MixSoftmaxMSEFn.apply(z, z, bad, 0.5, 0.5)
    torch.cuda.synchronize()


# ---- the hooks ---------------------------------------------------------------------------------------------------------
class _Ep:
    """what the two hooks see of their epocher"""

    def __init__(self, model):
        from contrastyou.meters import MeterInterface
        self.meters, self._model, self.device = MeterInterface(), model, DEV
        self.num_classes = model.num_classes

    def adopt(self, hook):
        hook.epocher = self
        hook._test_epocher = self  # the hook holds its epocher weakly
        return hook

    def reading(self, hook):
        return dict(self.meters.statistics())[hook.name]["loss"]


def _params_grad(model):
    return torch.cat([model.w.grad.flatten(), model.b.grad.flatten()]).cpu()


def test_mixup_hook_against_the_reference(npz, tol):
    from contrastyou.losses.kl import KL_div
    from semi_seg.hooks.mixup import _MixUpEpocherHook
    h = mc.HOOK_MIXUP
    model = fx.Conv1x1(npz["mixup_w"], npz["mixup_b"]).to(DEV)
    ep = _Ep(model)
    hook = ep.adopt(_MixUpEpocherHook(name="mix_reg", weight=h["weight"], criterion=KL_div(), enable_bn=True))
    value = hook(labeled_image=fx.decode(npz["mixup_image_i8d8"]).to(DEV),
                 labeled_image_tf=fx.decode(npz["mixup_image_tf_i8d8"]).to(DEV),
                 labeled_target=torch.from_numpy(npz["mixup_y"]).long().to(DEV),
                 labeled_target_tf=torch.from_numpy(npz["mixup_y_tf"]).float().to(DEV), seed=h["seed"])
    value.backward()
    check("mixup hook", value.detach().cpu(), _params_grad(model), npz["mixup_value64"], npz["mixup_g64"], tol, up=1.0)
    meter = ep.reading(hook)
    print("meter", meter, npz["mixup_meter64"])
    assert fx.rel_scalar(meter, npz["mixup_meter64"][0]) <= tol["scalar"]


def test_ict_hook_against_the_reference(npz, tol):
    from semi_seg.hooks.mt import EMAUpdater, _ICTMeanTeacherEpocherHook
    h = mc.HOOK_ICT
    model = fx.Conv1x1(npz["ict_w"], npz["ict_b"]).to(DEV)
    teacher = fx.Conv1x1(npz["ict_tw"], npz["ict_tb"]).to(DEV)
    ep = _Ep(model)
    hook = ep.adopt(_ICTMeanTeacherEpocherHook(name="ict", weight=h["weight"], model=model, teacher_model=teacher,
                                               updater=EMAUpdater()))
    value = hook(unlabeled_tf_logits=None, unlabeled_image=fx.decode(npz["ict_image_i8d8"]).to(DEV),
                 unlabeled_image_tf=fx.decode(npz["ict_image_tf_i8d8"]).to(DEV), seed=h["seed"])
    value.backward()
    check("ict hook", value.detach().cpu(), _params_grad(model), npz["ict_value64"], npz["ict_g64"], tol, up=1.0)
    assert teacher.w.grad is None and teacher.b.grad is None
    meter = ep.reading(hook)
    print("meter", meter, npz["ict_meter64"])
    assert fx.rel_scalar(meter, npz["ict_meter64"][0]) <= tol["scalar"]


# ---- steps on a small U-Net: the fused hook loss against the same step with the loss composed in torch -----------------
def _unfused_mixup_hook():
    from contrastyou.losses.kl import KL_div
    from contrastyou.utils.general import class2one_hot
    from contrastyou.utils.utils import fix_all_seed_within_context
    from semi_seg.hooks.mixup import MixUpTrainHook, _MixUpEpocherHook
    from semi_seg.hooks.utils import mixup_draw

    class Unfused(_MixUpEpocherHook):
        def _call_implementation(self, *, labeled_image, labeled_image_tf, labeled_target, labeled_target_tf, seed,
                                 **kwargs):
            K = self.num_classes
            oh = torch.cat([class2one_hot(labeled_target.long().squeeze(1), K),
                            class2one_hot(labeled_target_tf.long().squeeze(1), K)], dim=0).float()
            x = torch.cat([labeled_image, labeled_image_tf], dim=0)
            with fix_all_seed_within_context(seed):
                lam, index = mixup_draw(x.shape[0], alpha=1)
            index = index.to(x.device)
            mixed_image = lam * x + (1 - lam) * x[index, :]
            mixed_target = lam * oh + (1 - lam) * oh[index, :]
            with self.bn_context_manger(self._model):
                logits = self._model(mixed_image)
            loss = KL_div()(logits.float().softmax(1), mixed_target)
            self.meters["loss"].add(loss.detach())
            return loss * self._weight

    class UnfusedTrainHook(MixUpTrainHook):
        def __call__(self, **kwargs):
            return Unfused(name="mix_reg", weight=self._weight, criterion=KL_div(), enable_bn=self._enable_bn)

    return UnfusedTrainHook


def _unfused_ict_hook():
    from contrastyou.utils.utils import fix_all_seed_within_context
    from semi_seg.hooks.mt import ICTMeanTeacherTrainerHook, _ICTMeanTeacherEpocherHook
    from semi_seg.hooks.utils import mixup_draw

    class Unfused(_ICTMeanTeacherEpocherHook):
        def _call_implementation(self, *, unlabeled_tf_logits, unlabeled_image, unlabeled_image_tf, seed, **kwargs):
            with torch.no_grad():
                p = torch.cat([self._teacher_model(unlabeled_image).float().softmax(1),
                               self._teacher_model(unlabeled_image_tf).float().softmax(1)], dim=0)
                x = torch.cat([unlabeled_image, unlabeled_image_tf], dim=0)
                with fix_all_seed_within_context(seed):
                    lam, index = mixup_draw(x.shape[0], alpha=0.2)
                index = index.to(x.device)
                mixed_image = lam * x + (1 - lam) * x[index, :]
                mixed_target = lam * p + (1 - lam) * p[index, :]
            loss = torch.nn.MSELoss(reduction="none")(self._model(mixed_image).float().softmax(1), mixed_target).mean()
            self.meters["loss"].add(loss.detach())
            return self._weight * loss

    class UnfusedTrainHook(ICTMeanTeacherTrainerHook):
        def __call__(self):
            return Unfused(name=self._hook_name, weight=self._weight, model=self.trainer._model,
                           teacher_model=self._teacher_model, updater=self._updater)

    return UnfusedTrainHook


class _StepTrainer:
    def __init__(self, model, max_epoch):
        self._model, self._max_epoch = model, max_epoch


def _step(kind, fused, sd0, lab, unl, K=4):
    """one step (f32, eager) -> (metrics, {parameter: gradient}, BN buffers)"""
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.losses.kl import KL_div
    from contrastyou.optim import RAdam
    from cyhip import graphed
    from semi_seg.epochers import MixupEpocher, SemiSupervisedEpocher
    from semi_seg.hooks import ICTMeanTeacherTrainerHook, MixUpTrainHook
    default = graphed.GRAPH_STEP
    graphed.GRAPH_STEP = False
    try:
        type(TrainerHook).names.clear()
        model = UNet(input_dim=1, num_classes=K, max_channel=128, momentum=0.1)
        model.load_state_dict(sd0)
        model.to(DEV)
        if kind == "mixup":
            cls = MixUpTrainHook if fused else _unfused_mixup_hook()
            hook = cls(hook_name="mixup", weight=0.5, enable_bn=True)
            epocher = MixupEpocher
        else:
            cls = ICTMeanTeacherTrainerHook if fused else _unfused_ict_hook()
            hook = cls(name="ict", model=model, weight=5.0, alpha=0.99, weight_decay=1e-6)
            epocher = SemiSupervisedEpocher
        hook = hook.to(DEV)
        trainer = _StepTrainer(model, max_epoch=10)
        hook.register_trainer(trainer)
        opt = RAdam([{"params": list(model.parameters())}], lr=1e-3, weight_decay=1e-4)
        ep = epocher(model=model, optimizer=opt, labeled_loader=Loader(lab), unlabeled_loader=Loader(unl),
                     sup_criterion=KL_div(), num_batches=1, cur_epoch=0, device=DEV, two_stage=True, disable_bn=False,
                     scaler=torch.amp.GradScaler("cuda", enabled=False), accumulate_iter=1)
        ep.init(trainer)
        random.seed(9)
        with ep.register_hook(hook()):
            ep.run()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}
        return ep.get_metric(), grads
    finally:
        graphed.GRAPH_STEP = default
        type(TrainerHook).names.clear()


def _grad_distance(a, b):
    """the largest distance of a parameter's gradient from the other run's, relative to its own 2-norm"""
    assert a.keys() == b.keys() and len(a) > 10
    worst = max(((float((a[n] - b[n]).norm() / b[n].norm()), n) for n in a))
    return worst


@pytest.mark.parametrize("kind", ["mixup", "ict"])
def test_a_step_against_the_same_step_with_the_loss_composed_in_torch(npz, tol, kind):
    from oracle import unet as ou
    sd0 = ou.init_state_dict(1, 4, 128, seed=14)
    g = torch.Generator().manual_seed(21)
    lab, unl = [blob_batch(2, 32, 4, g)], [blob_batch(2, 32, 4, g)]
    m_f, g_f = _step(kind, True, sd0, lab, unl)
    m_u, g_u = _step(kind, False, sd0, lab, unl)
    m_u2, g_u2 = _step(kind, False, sd0, lab, unl)
    group = "mix_reg" if kind == "mixup" else "ict"
    noise = _grad_distance(g_u2, g_u)
    dist = _grad_distance(g_f, g_u)
    sup = fx.rel_scalar(m_f["semi"]["sup_loss"], m_u["semi"]["sup_loss"])
    reg = fx.rel_scalar(m_f["semi"]["reg_loss"], m_u["semi"]["reg_loss"])
    own = fx.rel_scalar(m_f[group]["loss"], m_u[group]["loss"])
    print(kind, "two unfused runs", noise, "fused vs unfused", dist, "sup", sup, "reg", reg, "hook meter", own,
          m_f["semi"], m_f[group])
    assert np.isfinite(m_f["semi"]["reg_loss"]) and m_f["semi"]["reg_loss"] > 0 and m_f[group]["loss"] > 0
    assert sup <= tol["scalar"] and reg <= tol["scalar"] and own <= tol["scalar"]
    assert dist[0] <= tol["grad2"], dist


def test_enable_bn_false_keeps_the_mixed_pass_out_of_the_running_statistics(npz):
    from contrastyou.arch import UNet
    from contrastyou.losses.kl import KL_div
    from semi_seg.hooks.mixup import _MixUpEpocherHook
    torch.manual_seed(4)
    model = UNet(input_dim=1, num_classes=4, max_channel=128, momentum=0.1).to(DEV).train()
    g = torch.Generator().manual_seed(2)
    b = blob_batch(2, 32, 4, g)
    image, target = b["img"][0].to(DEV), b["gt"][0].to(DEV)
    kwargs = dict(labeled_image=image, labeled_image_tf=image.flip(-1), labeled_target=target,
                  labeled_target_tf=target.flip(-1).float(), seed=11)

    def buffers():
        return {n: v.detach().clone() for n, v in model.named_buffers() if "running" in n or "num_batches" in n}

    before = buffers()
    assert len(before) > 10
    ep = _Ep(model)
    off = ep.adopt(_MixUpEpocherHook(name="mix_off", weight=1.0, criterion=KL_div(), enable_bn=False))
    v_off = off(**kwargs).detach()
    assert all(torch.equal(before[n], v) for n, v in buffers().items())
    on = ep.adopt(_MixUpEpocherHook(name="mix_on", weight=1.0, criterion=KL_div(), enable_bn=True))
    v_on = on(**kwargs).detach()
    assert any(not torch.equal(before[n], v) for n, v in buffers().items())
    # train mode either way: the same batch statistics (f32 rounding apart, should the two modes take other kernels)
    assert torch.isfinite(v_off) and abs(float(v_off) - float(v_on)) <= 1e-5 * abs(float(v_on))
    assert all(m.track_running_stats for m in model.modules() if hasattr(m, "track_running_stats"))


def test_mixup_trainer_trains_and_mt_trainer_runs_ict(tmp_path):
    """MixUpTrainer + MixUpTrainHook, and MTTrainer + ICTMeanTeacherTrainerHook (found by mt_in_hooks; evaluation on the
    teacher), each for two epochs of two steps"""
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.losses.kl import KL_div
    from semi_seg.hooks import ICTMeanTeacherTrainerHook, MixUpTrainHook, mt_in_hooks
    from semi_seg.trainers import MixUpTrainer, MTTrainer
    g = torch.Generator().manual_seed(8)
    lab, unl = [blob_batch(2, 32, 4, g) for _ in range(2)], [blob_batch(2, 32, 4, g) for _ in range(2)]
    val = [{k: v[0] for k, v in blob_batch(2, 32, 4, g, views=1).items()}]
    cfg = {"Optim": {"name": "RAdam", "lr": 1e-4, "weight_decay": 1e-5},
           "Scheduler": {"multiplier": 100, "warmup_max": 2}, "Trainer": {"name": "semi"}}
    for name in ("mixup", "ict"):
        type(TrainerHook).names.clear()
        torch.manual_seed(3)
        model = UNet(input_dim=1, num_classes=4, max_channel=128, momentum=0.1)
        cls = MixUpTrainer if name == "mixup" else MTTrainer
        save = tmp_path / name
        tr = cls(model=model, labeled_loader=Loader(lab), unlabeled_loader=Loader(unl), val_loader=Loader(val),
                 test_loader=Loader(val), criterion=KL_div(), save_dir=str(save), max_epoch=2, num_batches=2,
                 device=DEV, disable_bn=False, two_stage=True, config=cfg, enable_scale=True)
        if name == "mixup":
            hook = MixUpTrainHook(hook_name="mixup", weight=0.1, enable_bn=False)
            assert not mt_in_hooks(hook)
        else:
            hook = ICTMeanTeacherTrainerHook(name="ict", model=model, weight=1.0, alpha=0.99, weight_decay=1e-6)
            assert mt_in_hooks(hook)
        with tr.register_hook(hook):
            tr.init()
            if name == "ict":
                tr.set_model4inference(hook.teacher_model)
            tr.start_training()
        assert tr._cur_epoch == 2
        rows = (save / "storage.csv").read_text().strip().splitlines()
        group = "tra/mix_reg/loss" if name == "mixup" else "tra/ict/loss"
        assert group in rows[0], rows[0]
        col = rows[0].split(",").index(group)
        assert all(np.isfinite(float(r.split(",")[col])) and float(r.split(",")[col]) > 0 for r in rows[1:]), rows
        assert all(torch.isfinite(p).all() for p in model.parameters())
    type(TrainerHook).names.clear()
