"""Entropy minimisation, pseudo-label and UA-MT on the GPU (csrc/cy_pixel_reg.hip and the hooks on it) against
tests/golden/semi_baselines.npz (the reference's epocher hooks in f32 and f64, tests/golden/gen_goldens_semi.py) and
against f64 CPU evaluations written here from the formulas.

Tolerance rule (the one of tests/test_gpu_cc.py).  The yardstick is the reference's own f32-to-f64 distance on the
fixture's inputs:
    e(x) = |x - x64| relative: 2-norm for gradients, element-wise maximum over max|grad64|, |.| / |loss64| for the loss
    require e_hip <= max(4 * e_ref, 1e-6), e_ref = the largest value over the fixture's cases of the same kind
No pixel is left out of any comparison: the fixture's generator and `_inputs` below keep every teacher entropy 1e-4
away from the threshold (an f32 entropy is good to about 1e-6), so the f32 mask is the f64 mask.
Every figure is printed before it is asserted.
"""
import copy
import math
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from semi_fixture import KS, MAX_EPOCH, SHAPE, TEACHERS, ZERO_ROWS, StoredTeacher, decode, uamt_cases
from test_gpu_hooks_dice import Loader, blob_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR, FACTOR = 1e-6, 4.0
EPS = 1e-16
MARGIN = 1e-4


@pytest.fixture(scope="module")
def fx(golden_dir):
    data = np.load(golden_dir / "semi_baselines.npz")

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


# ---------------------------------------------------------------------------------------------- f64 formulas (CPU)
def entropy_of(p):
    return -(p * (p + EPS).log()).sum(1)


def ent64(z):
    return entropy_of(z.softmax(1)).mean()


def pl64(z):
    p = z.softmax(1)
    onehot = F.one_hot(z.detach().argmax(1), z.shape[1]).movedim(-1, 1).to(p.dtype)  # first maximal index
    return ((p - onehot) ** 2).mean()


def uamt64(zt, zs, thr, hard):
    """-> (loss, mask); thr is the f32 value the kernel is handed"""
    t = zt.softmax(1)
    mask = (entropy_of(t) < float(np.float32(thr))).to(zs.dtype)
    tau = F.one_hot(zt.argmax(1), zt.shape[1]).movedim(-1, 1).to(zs.dtype) if hard else t
    e = ((tau - zs.softmax(1)) ** 2).mean(1)
    return (e * mask).mean() / (float(np.float32(float(mask.mean()))) + 1e-2), mask


def eval64(fn, z):
    """-> (loss, dloss/dz) of an f64 formula"""
    z = z.double().requires_grad_(True)
    out = fn(z)
    loss = out[0] if isinstance(out, tuple) else out
    loss.backward()
    return loss.detach(), z.grad


# ------------------------------------------------------------------------------------- hooks without an epocher
class _Trainer:
    def __init__(self, max_epoch):
        self._max_epoch = max_epoch


class _Epocher:
    """what a hook sees of its epocher: meters, cur_epoch, trainer._max_epoch"""

    def __init__(self, cur_epoch=0, max_epoch=MAX_EPOCH):
        from contrastyou.meters import MeterInterface
        self.meters, self.cur_epoch, self.trainer = MeterInterface(), cur_epoch, _Trainer(max_epoch)

    def adopt(self, hook):
        hook.epocher = self  # (held weakly by the hook, like a real epocher: the hook keeps this one alive itself)
        hook._test_epocher = self
        return hook

    def summary(self, hook):
        return dict(self.meters.statistics())[hook.name]


def identity(t, mode=None):
    return t


def _call(hook, z, **kw):
    return hook(unlabeled_tf_logits=z, unlabeled_logits_tf=z, seed=1, affine_transformer=identity, **kw)


def _uamt_hook(teacher, hard, cur_epoch, max_epoch=MAX_EPOCH, student=None, cls=None):
    from semi_seg.hooks.mt import EMAUpdater, _UAMeanTeacherEpocherHook
    ep = _Epocher(cur_epoch, max_epoch)
    hook = (cls or _UAMeanTeacherEpocherHook)(name="mt", weight=1.0, model=student, teacher_model=teacher,
                                              updater=EMAUpdater(), hard_clip=hard)
    return ep.adopt(hook), ep


# ---------------------------------------------------------------------------------------------- 1. the fixture
@pytest.mark.parametrize("K", KS)
def test_entropy_min_hook_against_the_reference(fx, K):
    from contrastyou.losses.kl import Entropy
    from semi_seg.hooks.entmin import _EntropyEpocherHook
    ep = _Epocher()
    hook = ep.adopt(_EntropyEpocherHook(name="entropy", weight=1.0, criterion=Entropy()))
    z = gpu_leaf(fx.dec(f"K{K}_zs_i8d8"))
    loss = _call(hook, z)
    loss.backward()
    check(f"entmin K {K}", loss, fx[f"ent_K{K}_loss64"], z.grad, fx.t(f"ent_K{K}_g64"), fx.e_ref("ent"))
    assert abs(ep.summary(hook)["loss"] - float(loss)) <= 1e-7 * abs(float(loss))


@pytest.mark.parametrize("K", KS)
def test_pseudo_label_hook_against_the_reference(fx, K):
    from semi_seg.hooks.pseudolabel import _PLEpocherHook
    ep = _Epocher()
    hook = ep.adopt(_PLEpocherHook(name="plab", weight=1.0, criterion=torch.nn.MSELoss()))
    zs = fx.dec(f"K{K}_zs_i8d8")
    z = gpu_leaf(zs)
    loss = _call(hook, z)
    loss.backward()
    check(f"pseudo-label K {K}", loss, fx[f"pl_K{K}_loss64"], z.grad, fx.t(f"pl_K{K}_g64"), fx.e_ref("pl"))
    assert abs(ep.summary(hook)["loss"] - float(loss)) <= 1e-7 * abs(float(loss))
    # the tie rule: an all-zero row (what the warp pads with) takes class 0, the first maximal index
    rows = cpu64(z.grad)[:, :, :ZERO_ROWS]
    assert (zs[:, :, :ZERO_ROWS] == 0).all()
    P = zs.shape[0] * zs.shape[2] * zs.shape[3]
    p = torch.full((K,), 1.0 / K, dtype=torch.float64)
    d = p - F.one_hot(torch.tensor(0), K).double()
    want = 2.0 / (P * K) * p * (d - (d * p).sum())
    err = (rows - want.view(1, K, 1, 1)).abs().max().item()
    print(f"pseudo-label K {K}: zero rows, class-0 gradient max err {err:.2e}")
    assert err <= 8 * 2.0 ** -24 * want.abs().max().item()  # softmax, d, the dot and three products: < 8 f32 roundings
    assert rows[:, 0].max() < 0 and rows[:, 1:].min() > 0


@pytest.mark.parametrize("key,tag,K,cur_epoch,hard", uamt_cases(), ids=[c[0] for c in uamt_cases()])
def test_uamt_hook_against_the_reference(fx, key, tag, K, cur_epoch, hard):
    """the epocher hook on a teacher that returns the fixture's five logit tensors: mean, softmax, entropy, mask,
    [one-hot,] MSE and normalisation against the reference's, and the mask count exactly"""
    zt = fx.dec(f"{tag}_zt_i8d8").to(DEV)
    teacher = StoredTeacher(list(zt))
    hook, ep = _uamt_hook(teacher, hard, cur_epoch)
    z = gpu_leaf(fx.dec(f"{tag}_zs_i8d8"))
    image = torch.zeros(SHAPE[0], 1, *SHAPE[1:], device=DEV)
    loss = _call(hook, z, unlabeled_image=image, unlabeled_image_tf=image)
    loss.backward()
    assert teacher.calls == TEACHERS
    check(key, loss, fx[f"{key}_loss64"], z.grad, fx.t(f"{key}_g64"), fx.e_ref("uamt"))
    meters = ep.summary(hook)
    P, count = z.shape[0] * z.shape[2] * z.shape[3], int(fx[f"{key}_count"])
    print(f"{key}: mask_mean {meters['mask']!r}, fixture count {count} of {P}")
    assert meters["mask"] == float(np.float32(count / P)), (meters["mask"], count)
    assert round(meters["mask"] * P) == count
    assert abs(meters["loss"] - float(loss)) <= 1e-7 * abs(float(loss))
    from semi_seg.hooks.mt import uamt_threshold
    assert uamt_threshold(K, cur_epoch, MAX_EPOCH) == float(fx[f"{key}_thr"])


# ---------------------------------------------------------------------------------------------- 2. own f64 evaluation
def _inputs(gen, n, K, H, W, thr):
    """student and teacher logits with every teacher entropy at least MARGIN away from thr"""
    scale = torch.rand(n, 1, H, W, generator=gen) * 3
    zs = torch.randn(n, K, H, W, generator=gen) * scale.roll(1, 0)
    zt = torch.randn(n, K, H, W, generator=gen) * scale
    near = (entropy_of(zt.double().softmax(1)) - thr).abs() < MARGIN
    zt = torch.where(near[:, None], torch.zeros_like(zt), zt)  # a uniform row: entropy ln K > thr
    assert not ((entropy_of(zt.double().softmax(1)) - thr).abs() < MARGIN).any()
    return zs, zt


def _three_losses(what, fx, zs, zt, thr, hard):
    from cyhip.functions import SoftmaxEntropyFn, SoftmaxSelfMSEFn, UAMTLossFn
    assert not ((entropy_of(zt.double().softmax(1)) - thr).abs() < MARGIN).any(), "a teacher entropy on the threshold"
    ztd = zt.to(DEV)
    z = gpu_leaf(zs)
    loss = SoftmaxEntropyFn.apply(z, EPS)
    loss.backward()
    l64, g64 = eval64(ent64, zs)
    check(f"{what} entropy", loss, l64, z.grad, g64, fx.e_ref("ent"))
    z = gpu_leaf(zs)
    loss = SoftmaxSelfMSEFn.apply(z)
    loss.backward()
    l64, g64 = eval64(pl64, zs)
    check(f"{what} self-MSE", loss, l64, z.grad, g64, fx.e_ref("pl"))
    z = gpu_leaf(zs)
    loss, mask_mean = UAMTLossFn.apply(ztd, z, thr, hard)
    assert not mask_mean.requires_grad and mask_mean.shape == ()
    loss.backward()
    _, mask64 = uamt64(zt.double(), zs.double(), thr, hard)
    l64, g64 = eval64(lambda s: uamt64(zt.double(), s, thr, hard), zs)
    check(f"{what} UA-MT hard {hard}", loss, l64, z.grad, g64, fx.e_ref("uamt"))
    count = int(mask64.sum())
    print(f"{what} UA-MT: mask count {count} of {mask64.numel()}")
    assert 0 < count < mask64.numel()
    assert float(mask_mean) == float(np.float32(count / mask64.numel()))


@pytest.mark.parametrize("n,K,H,W", [
    (3, 2, 300, 300),    # 270 000 pixels > 1024 blocks x 256: the grid-stride loop goes round again; K = 2: 8-byte rows
    (3, 4, 300, 300),    # ... 16-byte rows
    (3, 5, 300, 300),    # ... the run-time-K kernels
    (3, 8, 300, 300),    # ... two 16-byte accesses per row
    (3, 16, 300, 300),   # ... the widest row
    (16, 4, 224, 224),   # the production size
    (2, 8, 17, 9),       # 306 pixels: one block and a tail
    (2, 3, 17, 9),
])
def test_sizes_the_fixture_does_not_hold_against_f64_formulas(fx, n, K, H, W):
    gen = torch.Generator().manual_seed(1000 * K + H)
    thr = 0.85 * math.log(K)
    zs, zt = _inputs(gen, n, K, H, W, thr)
    _three_losses(f"{n}x{K}x{H}x{W}", fx, zs, zt, thr, hard=(K % 3 == 2))


# ---------------------------------------------------------------------------------------------- 3. extremes
@pytest.mark.parametrize("K", [4, 5])
def test_saturated_logits(fx, K):
    """logits of +-80: exp(-160) underflows, p_k = 0 exactly; 0 * log(0 + eps) = 0 in both passes, nothing is NaN"""
    gen = torch.Generator().manual_seed(80 + K)
    thr = 0.85 * math.log(K)
    zs, zt = _inputs(gen, 2, K, 19, 23, thr)
    sat = torch.where(torch.rand(2, K, 19, 23, generator=gen) < 0.4, 80.0, -80.0)
    rows = torch.rand(2, 1, 19, 23, generator=gen) < 0.3
    zs = torch.where(rows, sat, zs)
    zt = torch.where(rows.roll(3, 2), sat.roll(1, 1), zt)
    assert (zs.softmax(1) == 0).any() and (zt.softmax(1) == 0).any()
    _three_losses(f"saturated K {K}", fx, zs, zt, thr, hard=False)
    _three_losses(f"saturated K {K}", fx, zs, zt, thr, hard=True)


@pytest.mark.parametrize("hard", [False, True])
def test_uamt_with_every_pixel_masked_out(hard):
    """thr = 0: no entropy lies below it; loss = 0 / (0 + 1e-2) = 0 exactly, the gradient is exactly 0"""
    from cyhip.functions import UAMTLossFn
    gen = torch.Generator().manual_seed(3)
    zs, zt = torch.randn(2, 4, 17, 9, generator=gen), torch.randn(2, 4, 17, 9, generator=gen) * 30
    z = gpu_leaf(zs)
    loss, mask_mean = UAMTLossFn.apply(zt.to(DEV), z, 0.0, hard)
    loss.backward()
    assert float(loss) == 0.0 and float(mask_mean) == 0.0
    assert torch.equal(z.grad, torch.zeros_like(z.grad))


# ---------------------------------------------------------------------------------------------- 4. determinism
def test_two_runs_give_the_same_bits():
    from cyhip.functions import SoftmaxEntropyFn, SoftmaxSelfMSEFn, UAMTLossFn
    gen = torch.Generator().manual_seed(5)
    for K in (4, 5):
        zs, zt = _inputs(gen, 3, K, 300, 300, 0.85 * math.log(K))
        ztd = zt.to(DEV)
        runs = []
        for _ in range(2):
            out = []
            for fn in (lambda z: SoftmaxEntropyFn.apply(z, EPS), SoftmaxSelfMSEFn.apply,
                       lambda z: UAMTLossFn.apply(ztd, z, 0.85 * math.log(K), False)[0]):
                z = gpu_leaf(zs)
                loss = fn(z)
                loss.backward()
                out += [loss.detach().cpu(), z.grad.cpu()]
            runs.append(out)
        for a, b in zip(*runs):
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- 5. launch counts
# kernel launches behind each entry point, as include/contrastyou_hip.h states them; what is observed here are the
# entry-point calls (the rule of tests/test_gpu_cc.py)
LAUNCHES = {"cy_softmax_entropy_fwd": 2, "cy_softmax_entropy_bwd": 1, "cy_softmax_selfmse_fwd": 2,
            "cy_softmax_selfmse_bwd": 1, "cy_uamt_mse_fwd": 2, "cy_uamt_mse_bwd": 1}


class _Count:
    def __init__(self, monkeypatch):
        from cyhip import _lib
        self.calls, real = [], _lib.call

        def counted(name, *args):
            self.calls.append(name)
            return real(name, *args)

        monkeypatch.setattr(_lib, "call", counted)

    def take(self):
        got, self.calls = self.calls, []
        return {n: got.count(n) for n in sorted(set(got))}


def _three_hooks(K, hard=False):
    from contrastyou.losses.kl import Entropy
    from semi_seg.hooks.entmin import _EntropyEpocherHook
    from semi_seg.hooks.pseudolabel import _PLEpocherHook
    gen = torch.Generator().manual_seed(6)
    zs, zt = _inputs(gen, 2, K, 40, 36, 0.75 * math.log(K))
    teacher = StoredTeacher([zt.to(DEV) + 0.01 * i for i in range(TEACHERS)])
    ent = _Epocher().adopt(_EntropyEpocherHook(name="entropy", weight=1.0, criterion=Entropy()))
    pl = _Epocher().adopt(_PLEpocherHook(name="plab", weight=0.1, criterion=torch.nn.MSELoss()))
    ua, _ = _uamt_hook(teacher, hard, cur_epoch=0)
    image = torch.zeros(2, 1, 40, 36, device=DEV)
    return zs, {"entropy": (ent, {}), "selfmse": (pl, {}),
                "uamt": (ua, dict(unlabeled_image=image, unlabeled_image_tf=image))}


@pytest.mark.parametrize("K", [4, 5])
def test_launch_counts_and_no_host_round_trip(monkeypatch, K):
    """each hook call: one forward entry (2 launches) and one backward entry (1 launch) and nothing else of the
    library; no device-to-host copy anywhere in the call or its backward"""
    zs, hooks = _three_hooks(K)
    for kind, (hook, kw) in hooks.items():
        z = gpu_leaf(zs)
        torch.cuda.synchronize()
        count = _Count(monkeypatch)
        torch.cuda.set_sync_debug_mode("error")
        try:
            loss = _call(hook, z, **kw)
            fwd = count.take()
            loss.backward()
            bwd = count.take()
        finally:
            torch.cuda.set_sync_debug_mode("default")
            monkeypatch.undo()
        name = "uamt_mse" if kind == "uamt" else f"softmax_{kind}"
        assert fwd == {f"cy_{name}_fwd": 1}, (kind, fwd)
        assert bwd == {f"cy_{name}_bwd": 1}, (kind, bwd)
        assert LAUNCHES[f"cy_{name}_fwd"] == 2 and LAUNCHES[f"cy_{name}_bwd"] == 1
        assert torch.isfinite(loss).item() and torch.isfinite(z.grad).all().item()


# ---------------------------------------------------------------------------------------------- 6. Entropy.from_logits
@pytest.mark.parametrize("K", KS)
def test_entropy_from_logits_equals_entropy_of_the_softmax(fx, K):
    from contrastyou.losses.kl import Entropy
    z = fx.dec(f"K{K}_zs_i8d8").to(DEV)
    got, want = Entropy().from_logits(z), Entropy()(z.softmax(1))
    e = abs(float(got) - float(want)) / abs(float(want))
    print(f"Entropy.from_logits K {K}: {float(got):.9g} vs {float(want):.9g}  e {e:.2e}")
    # both sides are f32 evaluations, each within the bound of the f64 value
    assert e <= 2 * bound(fx.e_ref("ent")[2])
    assert abs(float(got) - float(fx[f"ent_K{K}_loss64"])) <= bound(fx.e_ref("ent")[2]) * float(fx[f"ent_K{K}_loss64"])
    for red in ("sum", "none"):
        assert torch.equal(Entropy(reduction=red).from_logits(z), Entropy(reduction=red)(z.softmax(1)))


def test_entropy_from_logits_autograd(fx):
    from contrastyou.losses.kl import Entropy
    zs = torch.randn(2, 4, 5, 7, generator=torch.Generator().manual_seed(9)) * 2
    z = gpu_leaf(zs)
    loss = 3.0 * Entropy().from_logits(z)  # an upstream gradient other than 1
    loss.backward()
    l64, g64 = eval64(lambda t: 3.0 * ent64(t), zs)
    check("Entropy.from_logits autograd", loss, l64, z.grad, g64, fx.e_ref("ent"))


# ---------------------------------------------------------------------------------------------- 7. UA-MT on a U-Net
def test_uamt_hook_on_a_small_unet():
    """five teacher forwards, one of them tracked: num_batches_tracked + 1 and the running statistics of a single
    tracked forward; the loss is UAMTLossFn on the mean of the five logits; no gradient reaches the teacher"""
    from contrastyou.arch import UNet
    from cyhip.functions import UAMTLossFn
    from oracle import unet as ou
    from semi_seg.hooks.mt import _UAMeanTeacherEpocherHook, uamt_threshold
    K = 4
    student = UNet(input_dim=1, num_classes=K, max_channel=128, momentum=0.1)
    student.load_state_dict(ou.init_state_dict(1, K, 128, seed=11))
    student.to(DEV)
    teacher = copy.deepcopy(student)
    for p in teacher.parameters():
        p.detach_().requires_grad_(False)
    twin = copy.deepcopy(teacher).train()
    gen = torch.Generator().manual_seed(12)
    image = blob_batch(2, 32, K, gen)["img"][0].to(DEV)
    noise = [torch.randn(2, 1, 32, 32, generator=gen).to(DEV) for _ in range(4)]
    captured, asked = [], []

    class Hook(_UAMeanTeacherEpocherHook):
        def _noise(self, like, i):
            asked.append(i)
            return noise[i]

    hook, ep = _uamt_hook(teacher, False, cur_epoch=2, max_epoch=5, student=student, cls=Hook)
    handle = teacher.register_forward_hook(lambda m, a, out: captured.append(out.detach().clone()))
    before = {k: v.clone() for k, v in teacher.named_buffers()}
    z = gpu_leaf(torch.randn(2, K, 32, 32, generator=gen))
    for call in (1, 2):
        del captured[:], asked[:]
        z.grad = None
        loss = hook(unlabeled_tf_logits=z, unlabeled_image=image, unlabeled_image_tf=image, seed=7,
                    affine_transformer=identity)
        loss.backward()
        assert asked == [0, 1, 2, 3] and len(captured) == TEACHERS
        with torch.no_grad():
            twin(image)  # one tracked forward
        for k, v in teacher.named_buffers():
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(before[k]) + call, k
            assert torch.equal(v, dict(twin.named_buffers())[k]), k
        assert any(not torch.equal(v, before[k]) for k, v in teacher.named_buffers() if "running_mean" in k)
        assert all(m.track_running_stats for m in teacher.modules() if isinstance(m, torch.nn.BatchNorm2d))
        with torch.no_grad():
            for i in range(4):  # the noisy forwards saw image + 0.05 * noise under batch statistics
                assert torch.equal(captured[1 + i], twin_eval(twin, image + noise[i] * 0.05))
        thr = uamt_threshold(K, 2, 5)
        want, want_mask = UAMTLossFn.apply(torch.stack(captured, 0).mean(0), z.detach(), thr, False)
        assert torch.equal(loss.detach(), want), (loss, want)
        assert all(p.grad is None and not p.requires_grad for p in teacher.parameters())
        assert z.grad is not None and torch.isfinite(z.grad).all() and z.grad.abs().max() > 0
    handle.remove()
    meters = ep.summary(hook)
    assert math.isfinite(meters["loss"]) and meters["loss"] > 0
    assert 0 < meters["mask"] <= 1 and abs(meters["mask"] - float(want_mask)) < 1e-6


def twin_eval(twin, x):
    """the twin's logits under batch statistics without touching its running statistics"""
    with twin.switch_bn_track(enable=False):
        return twin(x)


# ------------------------------------------------------------------------------------- 8. semi-supervised steps
class _StepTrainer:
    def __init__(self, model, max_epoch):
        self._model, self._max_epoch = model, max_epoch


def _make_hook(kind, model):
    from semi_seg.hooks import create_ent_min_hook, create_pseudo_label_hook, create_uamt_hook
    if kind == "entmin":
        return create_ent_min_hook(weight=0.5)
    if kind == "pseudolabel":
        return create_pseudo_label_hook(weight=0.5)
    return create_uamt_hook(model=model, weight=10.0, alpha=0.99, weight_decay=1e-6, update_bn=False, num_teachers=1,
                            hard_clip=False)


def _semi_run(kind, lab, unl, sd0, *, graph, bf16=False, steps=1, K=4):
    """cur_epoch = max_epoch: the UA-MT threshold is ln K, so the mask of an untrained network is not empty"""
    from contrastyou.amp import BF16Scaler
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.losses.kl import KL_div
    from contrastyou.optim import RAdam
    from cyhip import graphed
    from semi_seg.epochers import SemiSupervisedEpocher
    default = graphed.GRAPH_STEP
    graphed.GRAPH_STEP = graph
    try:
        type(TrainerHook).names.clear()
        model = UNet(input_dim=1, num_classes=K, max_channel=128, momentum=0.1)
        model.load_state_dict(sd0)
        model.to(DEV)
        torch.manual_seed(3)
        hook = _make_hook(kind, model).to(DEV)
        trainer = _StepTrainer(model, max_epoch=10)
        hook.register_trainer(trainer)
        opt = RAdam([{"params": list(model.parameters())}], lr=3e-3, weight_decay=1e-4)
        scaler = BF16Scaler() if bf16 else torch.amp.GradScaler("cuda", enabled=False)
        ep = SemiSupervisedEpocher(model=model, optimizer=opt, labeled_loader=Loader(lab), unlabeled_loader=Loader(unl),
                                   sup_criterion=KL_div(), num_batches=steps, cur_epoch=10, device=DEV, two_stage=True,
                                   disable_bn=False, scaler=scaler, accumulate_iter=1)
        ep.init(trainer)
        random.seed(9)
        with ep.register_hook(hook()):
            ep.run()
        torch.cuda.synchronize()
        replayed = any(isinstance(v, graphed.GraphedTwoPass) for v in model.__dict__.get("_cy_graphed", {}).values())
        state = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
        if kind == "uamt":
            state.update({"teacher." + k: v.detach().float().cpu() for k, v in hook.teacher_model.state_dict().items()})
        return state, ep.get_metric(), replayed
    finally:
        graphed.GRAPH_STEP = default
        type(TrainerHook).names.clear()


def _batches(steps, n=4, hw=32, K=4, seed=21):
    g = torch.Generator().manual_seed(seed)
    return [blob_batch(n, hw, K, g) for _ in range(steps)], [blob_batch(n, hw, K, g) for _ in range(steps)]


GROUP = {"entmin": "entropy", "pseudolabel": "plab", "uamt": "mt"}


@pytest.mark.parametrize("kind", ["entmin", "pseudolabel", "uamt"])
def test_hooks_in_a_semi_supervised_step(kind):
    from oracle import unet as ou
    sd0 = ou.init_state_dict(1, 4, 128, seed=14)
    lab, unl = _batches(1)
    sd, m, _ = _semi_run(kind, lab, unl, sd0, graph=False)
    group = m[GROUP[kind]]
    print(kind, group, "reg_loss", m["semi"]["reg_loss"])
    assert np.isfinite(m["semi"]["reg_loss"]) and m["semi"]["reg_loss"] != 0
    assert np.isfinite(group["loss"]) and group["loss"] > 0
    if kind == "uamt":
        assert 0 < group["mask"] <= 1
        assert any(not torch.equal(sd["teacher." + k], sd0[k]) for k in sd0 if k.endswith(".weight"))  # the EMA ran
    assert all(torch.isfinite(v).all() for v in sd.values())


@pytest.mark.parametrize("kind", ["entmin", "pseudolabel", "uamt"])
def test_graph_replayed_steps_equal_eager_steps(kind):
    """the pattern of tests/test_gpu_cc.py: the hooks (and the UA-MT teacher's five forwards) run in the eager section
    between the two graph replays; four steps either way end in the same bits"""
    from oracle import unet as ou
    sd0 = ou.init_state_dict(1, 4, 128, seed=14)
    lab, unl = _batches(4)
    sd_e, m_e, rep_e = _semi_run(kind, lab, unl, sd0, graph=False, bf16=True, steps=4)
    sd_g, m_g, rep_g = _semi_run(kind, lab, unl, sd0, graph=True, bf16=True, steps=4)
    assert rep_g and not rep_e, "the second run must have captured and replayed the passes"
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k
    assert m_e["semi"]["reg_loss"] == m_g["semi"]["reg_loss"] and np.isfinite(m_e["semi"]["reg_loss"])
    assert m_e[GROUP[kind]] == m_g[GROUP[kind]]


def test_trainer_evaluates_the_uamt_teacher(tmp_path):
    """main_nd.py: `if mt_in_hooks(...): trainer.set_model4inference(hook.teacher_model)`"""
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.losses.kl import KL_div
    from semi_seg.hooks import create_uamt_hook, mt_in_hooks
    from semi_seg.trainers import trainer_zoo
    g = torch.Generator().manual_seed(8)
    lab, unl = [blob_batch(2, 32, 4, g)], [blob_batch(2, 32, 4, g)]
    val = [{k: v[0] for k, v in blob_batch(2, 32, 4, g, views=1).items()}]
    cfg = {"Optim": {"name": "RAdam", "lr": 1e-5, "weight_decay": 1e-5},
           "Scheduler": {"multiplier": 100, "warmup_max": 2}, "Trainer": {"name": "semi"}}
    type(TrainerHook).names.clear()
    model = UNet(input_dim=1, num_classes=4, max_channel=128, momentum=0.1)
    tr = trainer_zoo["semi"](model=model, labeled_loader=Loader(lab), unlabeled_loader=Loader(unl),
                             val_loader=Loader(val), test_loader=Loader(val), criterion=KL_div(),
                             save_dir=str(tmp_path), max_epoch=2, num_batches=1, device=DEV, disable_bn=False,
                             two_stage=True, config=cfg, enable_scale=True)
    hook = create_uamt_hook(model=model, weight=10.0, alpha=0.99, weight_decay=1e-6, update_bn=False, num_teachers=1,
                            hard_clip=False)
    assert mt_in_hooks(hook)
    with tr.register_hook(hook):
        tr.init()
        tr.set_model4inference(hook.teacher_model)
        assert tr.inference_model is hook.teacher_model
        tr.start_training()  # two epochs of one step: thr moves with cur_epoch / max_epoch, evaluation on the teacher
    assert tr._cur_epoch == 2
    rows = (tmp_path / "storage.csv").read_text().strip().splitlines()
    assert "tra/mt/mask" in rows[0] and "tra/mt/loss" in rows[0], rows[0]
    type(TrainerHook).names.clear()
