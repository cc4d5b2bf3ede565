"""The wide-K regularisers on the GPU (csrc/cy_wide_reg.hip: entropy, self-MSE, UA-MT and ICT's mix-MSE on
multi-prototype logits, 16 < K <= 64), their autograd functions, hooks and a multi-prototype step, against
tests/golden/semi_wide.npz (the reference's epocher hooks and ICT loss in f32 and f64,
tests/golden/gen_goldens_semi_wide.py) and against f64 CPU evaluations written here from the formulas.

Tolerance rule (the one of tests/test_gpu_semi_baselines.py).  The yardstick is the reference's own f32-to-f64 distance
on the fixture's inputs:
    e(x) = |x - x64| relative: 2-norm for gradients, element-wise maximum over max|grad64|, |.| / |loss64| for the loss
    require e_hip <= max(4 * e_ref, 1e-6), e_ref = the largest value over the new fixture's cases of the same kind
No pixel is left out of any comparison: the fixture's generator keeps every teacher entropy 1e-4 away from the
thresholds and asserts that the reference's f32 mask and arg-max are the f64 ones.  Every figure is printed before it is
asserted.
"""
import math
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import semi_wide_fixture as sw
from step_harness import OneBatchLoader
from test_gpu_hooks_dice import Loader, blob_batch
from test_gpu_semi_baselines import (DEV, EPS, MARGIN, _call, _Epocher, _StepTrainer, _uamt_hook, bound, check, cpu64,
                                     ent64, entropy_of, eval64, gpu_leaf, pl64, uamt64)

pytestmark = pytest.mark.gpu
GUARD = 777.25
P_FIX = sw.SHAPE[0] * sw.SHAPE[1] * sw.SHAPE[2]


@pytest.fixture(scope="module")
def fx(golden_dir):
    data = sw.load(golden_dir)

    class Fx:
        def __getitem__(self, k):
            return data[k]

        def t(self, k):
            return torch.from_numpy(data[k])

        def dec(self, k):
            return sw.decode(k, data[k])

        def e_ref(self, kind):
            """[2-norm, max, loss]: the largest over the fixture's cases of this kind"""
            rows = [data[k] for k in data.files if k.endswith("_e_ref") and k.startswith(kind)]
            assert rows, kind
            return np.max(np.stack(rows), axis=0)

    return Fx()


def ict64(zs, zt, index, w_self, w_other):
    """the weights are the f32 values the kernel is handed"""
    p = zt.softmax(1)
    mixed = float(np.float32(w_self)) * p + float(np.float32(w_other)) * p[index]
    return ((zs.softmax(1) - mixed) ** 2).mean()


def mt64(zt, zs, hard):
    t = zt.softmax(1)
    tau = F.one_hot(zt.argmax(1), zt.shape[1]).movedim(-1, 1).to(zs.dtype) if hard else t
    return ((tau - zs.softmax(1)) ** 2).mean()


def ict_args():
    from cyhip import ops
    return torch.tensor(sw.ICT_INDEX), ops.mix_weights(sw.ICT_LAM)


# ---------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("K", sw.KS)
def test_entropy_against_the_reference_and_f64(fx, K):
    from contrastyou.losses.kl import Entropy
    from cyhip.functions import SoftmaxEntropyFn
    from semi_seg.hooks.entmin import _EntropyEpocherHook
    zs = fx.dec(f"K{K}_zs_i8d8")
    ep = _Epocher()
    hook = ep.adopt(_EntropyEpocherHook(name="entropy", weight=1.0, criterion=Entropy()))
    z = gpu_leaf(zs)
    loss = _call(hook, z)
    loss.backward()
    check(f"entmin hook K {K}", loss, fx[f"ent_K{K}_loss64"], z.grad, fx.t(f"ent_K{K}_g64"), fx.e_ref("ent"))
    assert abs(ep.summary(hook)["loss"] - float(loss.detach())) <= 1e-7 * abs(float(loss.detach()))
    z2 = gpu_leaf(zs)
    loss2 = SoftmaxEntropyFn.apply(z2, EPS)
    loss2.backward()
    l64, g64 = eval64(ent64, zs)
    check(f"entropy K {K} vs f64", loss2, l64, z2.grad, g64, fx.e_ref("ent"))
    assert torch.equal(loss2.detach(), loss.detach()) and torch.equal(z2.grad, z.grad)


@pytest.mark.parametrize("K", sw.KS)
def test_self_mse_against_the_reference_and_f64(fx, K):
    from cyhip.functions import SoftmaxSelfMSEFn
    from semi_seg.hooks.pseudolabel import _PLEpocherHook
    zs = fx.dec(f"K{K}_zs_i8d8")
    ep = _Epocher()
    hook = ep.adopt(_PLEpocherHook(name="plab", weight=1.0, criterion=torch.nn.MSELoss()))
    z = gpu_leaf(zs)
    loss = _call(hook, z)
    loss.backward()
    check(f"pseudo-label hook K {K}", loss, fx[f"pl_K{K}_loss64"], z.grad, fx.t(f"pl_K{K}_g64"), fx.e_ref("pl"))
    assert abs(ep.summary(hook)["loss"] - float(loss.detach())) <= 1e-7 * abs(float(loss.detach()))
    z2 = gpu_leaf(zs)
    loss2 = SoftmaxSelfMSEFn.apply(z2)
    loss2.backward()
    l64, g64 = eval64(pl64, zs)
    check(f"self-MSE K {K} vs f64", loss2, l64, z2.grad, g64, fx.e_ref("pl"))


@pytest.mark.parametrize("key,K,cur_epoch,hard", sw.uamt_cases(), ids=[c[0] for c in sw.uamt_cases()])
def test_uamt_against_the_reference_and_f64(fx, key, K, cur_epoch, hard):
    from cyhip.functions import UAMTLossFn
    from semi_seg.hooks.mt import uamt_threshold
    zt = fx.dec(f"K{K}_zt_i8d8")
    teacher = sw.StoredTeacher(list(zt.to(DEV)))
    hook, ep = _uamt_hook(teacher, hard, cur_epoch, max_epoch=sw.MAX_EPOCH)
    zs = fx.dec(f"K{K}_zs_i8d8")
    z = gpu_leaf(zs)
    image = torch.zeros(sw.SHAPE[0], 1, *sw.SHAPE[1:], device=DEV)
    loss = _call(hook, z, unlabeled_image=image, unlabeled_image_tf=image)
    loss.backward()
    assert teacher.calls == sw.TEACHERS
    check(key, loss, fx[f"{key}_loss64"], z.grad, fx.t(f"{key}_g64"), fx.e_ref("uamt"))
    meters, count = ep.summary(hook), int(fx[f"{key}_count"])
    print(f"{key}: mask_mean {meters['mask']!r}, fixture count {count} of {P_FIX}")
    assert meters["mask"] == float(np.float32(count / P_FIX)), (meters["mask"], count)
    assert 0 < count < P_FIX
    thr = uamt_threshold(K, cur_epoch, sw.MAX_EPOCH)
    assert thr == float(fx[f"{key}_thr"])
    # the f64 formula on the mean of the five teachers
    zt64 = zt.double().mean(0)
    assert not ((entropy_of(zt64.softmax(1))[:, sw.ZERO_ROWS:] - thr).abs() < MARGIN).any()
    z2 = gpu_leaf(zs)
    loss2, mask_mean = UAMTLossFn.apply(zt.to(DEV).mean(0), z2, thr, hard)
    loss2.backward()
    l64, g64 = eval64(lambda s: uamt64(zt64, s, thr, hard), zs)
    check(f"{key} vs f64", loss2, l64, z2.grad, g64, fx.e_ref("uamt"))
    assert float(mask_mean) == float(np.float32(count / P_FIX))


@pytest.mark.parametrize("K", sw.KS)
def test_mix_mse_against_the_reference_and_f64(fx, K):
    from cyhip.functions import MixSoftmaxMSEFn
    zs, zt = fx.dec(f"K{K}_zs_i8d8"), fx.dec(f"K{K}_zt_i8d8")[0]
    index, (w_self, w_other) = ict_args()
    z, t = gpu_leaf(zs), gpu_leaf(zt)
    loss = MixSoftmaxMSEFn.apply(z, t, index, w_self, w_other)
    loss.backward()
    assert t.grad is None  # the teacher carries no gradient
    check(f"ict K {K}", loss, fx[f"ict_K{K}_loss64"], z.grad, fx.t(f"ict_K{K}_g64"), fx.e_ref("ict"))
    l64, g64 = eval64(lambda s: ict64(s, zt.double(), index, w_self, w_other), zs)
    check(f"ict K {K} vs f64", loss, l64, z.grad, g64, fx.e_ref("ict"))


# ---------------------------------------------------------------------------------------------- 2. ties and zero rows
def _row_grad(K, P, p, first):
    """f64 gradient of mean((p - onehot(first))^2) over P pixels of K classes with respect to the row's logits"""
    d = p - F.one_hot(torch.tensor(first), K).double()
    return 2.0 / (P * K) * p * (d - (d * p).sum())


@pytest.mark.parametrize("K", sw.KS)
def test_a_maximum_tied_across_lanes_takes_the_first_index(fx, K):
    from cyhip.functions import SoftmaxSelfMSEFn, UAMTLossFn
    zs, zt = fx.dec(f"K{K}_zs_i8d8"), fx.dec(f"K{K}_zt_i8d8").to(DEV).mean(0)
    n, h, w = sw.TIE_PIXEL
    a, b = sw.tie_channels(K)
    assert a // 4 != b // 4 and zs[n, a, h, w] == zs[n, b, h, w] == zs[n, :, h, w].max()
    assert zt[n, a, h, w] == zt[n, b, h, w] == zt[n, :, h, w].max()
    assert int(zs[n, :, h, w].argmax()) == a and (zs[:, :, :sw.ZERO_ROWS] == 0).all()
    e_max = bound(fx.e_ref("pl")[1])

    z = gpu_leaf(zs)
    SoftmaxSelfMSEFn.apply(z).backward()
    g = cpu64(z.grad)
    scale = g.abs().max().item()
    p = zs[n, :, h, w].double().softmax(0)
    want = _row_grad(K, P_FIX, p, a)
    err = (g[n, :, h, w] - want).abs().max().item()
    print(f"self-MSE K {K}: tied row, first-index gradient max err {err:.2e} of {scale:.2e} (bound {e_max:.2e})")
    assert err <= e_max * scale
    assert g[n, a, h, w] < 0 < g[n, b, h, w], "the one-hot sits on the first of the two tied channels"
    uniform = torch.full((K,), 1.0 / K, dtype=torch.float64)
    want0 = _row_grad(K, P_FIX, uniform, 0)
    err0 = (g[:, :, :sw.ZERO_ROWS] - want0.view(1, K, 1, 1)).abs().max().item()
    print(f"self-MSE K {K}: zero rows, class-0 gradient max err {err0:.2e}")
    assert err0 <= 8 * 2.0 ** -24 * want0.abs().max().item()  # softmax, d, the dot and three products: < 8 f32 roundings
    assert g[:, 0, :sw.ZERO_ROWS].max() < 0 and g[:, 1:, :sw.ZERO_ROWS].min() > 0

    # hard UA-MT with every pixel inside the mask (thr above ln K): the teacher's one-hot, student gradient
    z = gpu_leaf(zs)
    loss, mask_mean = UAMTLossFn.apply(zt, z, 10.0, True)
    loss.backward()
    assert float(mask_mean) == 1.0
    g = cpu64(z.grad)
    scale = g.abs().max().item()
    s = zs[n, :, h, w].double().softmax(0)
    want = _row_grad(K, P_FIX, s, a) / (1.0 + 1e-2)
    err = (g[n, :, h, w] - want).abs().max().item()
    print(f"hard UA-MT K {K}: tied teacher row, first-index gradient max err {err:.2e} of {scale:.2e}")
    assert err <= bound(fx.e_ref("uamt")[1]) * scale
    other = _row_grad(K, P_FIX, s, b) / (1.0 + 1e-2)
    assert (g[n, :, h, w] - other).abs().max().item() > 100 * err, "the other tied channel gives another gradient"
    want0 = _row_grad(K, P_FIX, uniform, 0) / (1.0 + 1e-2)
    err0 = (g[:, :, :sw.ZERO_ROWS] - want0.view(1, K, 1, 1)).abs().max().item()
    print(f"hard UA-MT K {K}: zero rows, class-0 gradient max err {err0:.2e}")
    assert err0 <= 16 * 2.0 ** -24 * want0.abs().max().item()
    assert g[:, 0, :sw.ZERO_ROWS].max() < 0 and g[:, 1:, :sw.ZERO_ROWS].min() > 0


# ---------------------------------------------------------------------------------------------- 3. extremes
@pytest.mark.parametrize("K", [17, 20])
def test_entropy_with_eps_zero_is_finite(fx, K):
    """absent channels are masked by index: 0 * log(0 + 0) never enters the sum"""
    from cyhip.functions import SoftmaxEntropyFn
    gen = torch.Generator().manual_seed(40 + K)
    zs = torch.rand(2, K, 13, 11, generator=gen) * 4 - 2
    z = gpu_leaf(zs)
    loss = SoftmaxEntropyFn.apply(z, 0.0)
    loss.backward()
    assert math.isfinite(float(loss.detach())) and torch.isfinite(z.grad).all()
    l64, g64 = eval64(lambda t: -(t.softmax(1) * t.softmax(1).log()).sum(1).mean(), zs)
    check(f"entropy eps 0 K {K}", loss, l64, z.grad, g64, fx.e_ref("ent"))


@pytest.mark.parametrize("K,hard", [(17, False), (20, True)])
def test_uamt_with_every_pixel_masked_out(K, hard):
    """thr = 0: no entropy lies below it; loss = 0 / (0 + 1e-2) = 0 exactly, the gradient is exactly 0"""
    from cyhip.functions import UAMTLossFn
    gen = torch.Generator().manual_seed(3)
    zs, zt = torch.randn(2, K, 17, 9, generator=gen), torch.randn(2, K, 17, 9, generator=gen) * 30
    z = gpu_leaf(zs)
    loss, mask_mean = UAMTLossFn.apply(zt.to(DEV), z, 0.0, hard)
    loss.backward()
    assert float(loss) == 0.0 and float(mask_mean) == 0.0
    assert torch.equal(z.grad, torch.zeros_like(z.grad))


# ---------------------------------------------------------------------------------------------- 4. the second trip
def _smooth_inputs(gen, n, K, H, W, thr):
    """student and teacher logits with every teacher entropy at least MARGIN away from thr"""
    scale = torch.rand(n, 1, H, W, generator=gen) * 3
    zs = torch.randn(n, K, H, W, generator=gen) * scale.flip(2)
    zt = torch.randn(n, K, H, W, generator=gen) * scale
    near = (entropy_of(zt.double().softmax(1)) - thr).abs() < MARGIN
    zt = torch.where(near[:, None], torch.zeros_like(zt), zt)  # a uniform row: entropy ln K > thr
    assert not ((entropy_of(zt.double().softmax(1)) - thr).abs() < MARGIN).any()
    return zs, zt


@pytest.fixture(scope="module")
def second_trip():
    """K = 20 inputs one pixel past what the capped grid covers in one trip, and their f64 results (computed once)"""
    from cyhip import ops
    K = 20
    plan = ops.wide_reg_plan("entropy", P_FIX, K)
    cap = ops.wide_reg_plan("entropy", 1 << 30, K)["fwd_grid"]
    npix = plan["rows_per_block"] * cap + 1
    for fam in ("entropy", "selfmse", "uamt", "mixmse"):
        p = ops.wide_reg_plan(fam, npix, K)
        assert p["fwd_trips"] == 2 and p["bwd_trips"] == 2 and p["vec"] == 4, (fam, p)
        assert ops.wide_reg_plan(fam, npix - 1, K)["fwd_trips"] == 1
    thr = 0.85 * math.log(K)
    zs, zt = _smooth_inputs(torch.Generator().manual_seed(65537), 1, K, npix, 1, thr)
    return K, npix, thr, zs, zt


@pytest.mark.parametrize("family", ["entropy", "selfmse", "uamt_soft", "uamt_hard", "mixmse"])
def test_one_pixel_past_the_first_trip(fx, second_trip, family):
    from cyhip.functions import MixSoftmaxMSEFn, SoftmaxEntropyFn, SoftmaxSelfMSEFn, UAMTLossFn
    K, npix, thr, zs, zt = second_trip
    z, ztd = gpu_leaf(zs), zt.to(DEV)
    what = f"{family} K {K}, {npix} pixels"
    if family == "entropy":
        loss, ref, kind = SoftmaxEntropyFn.apply(z, EPS), ent64, "ent"
    elif family == "selfmse":
        loss, ref, kind = SoftmaxSelfMSEFn.apply(z), pl64, "pl"
    elif family == "mixmse":
        index, (w_self, w_other) = torch.tensor([0]), (0.25, 0.75)  # one image: its partner is itself
        loss = MixSoftmaxMSEFn.apply(z, ztd, index, w_self, w_other)
        ref, kind = (lambda s: ict64(s, zt.double(), index, w_self, w_other)), "ict"
    else:
        hard = family == "uamt_hard"
        loss, mask_mean = UAMTLossFn.apply(ztd, z, thr, hard)
        ref, kind = (lambda s: uamt64(zt.double(), s, thr, hard)), "uamt"
        _, mask64 = uamt64(zt.double(), zs.double(), thr, hard)
        count = int(mask64.sum())
        print(f"{what}: mask count {count} of {npix}, the last pixel {'in' if mask64.flatten()[-1] else 'out'}")
        assert 0 < count < npix and float(mask_mean) == float(np.float32(count / npix))
    loss.backward()
    l64, g64 = eval64(ref, zs)
    check(what, loss, l64, z.grad, g64, fx.e_ref(kind))
    last = cpu64(z.grad)[0, :, -1, 0]
    assert torch.equal(last != 0, g64[0, :, -1, 0] != 0), "the pixel of the second trip has its gradient"


# ---------------------------------------------------------------------------------------------- 5. guarded slices
def place(t, sliced, fill=None):
    """(flat view on the GPU holding t [or `fill`], its buffer, the guard floats in front): 4 in front -- 5 for a base
    that is only 4-byte aligned -- and 4 behind"""
    lead = 5 if sliced else 4
    n = t if isinstance(t, int) else t.numel()
    buf = torch.full((n + lead + 4,), GUARD, device=DEV)
    view = buf[lead:lead + n]
    if isinstance(t, int):
        view.fill_(fill)
    else:
        view.copy_(t.reshape(-1))
    assert view.data_ptr() % 16 == (4 if sliced else 0)
    return view, buf, lead


def intact(placed):
    view, buf, lead = placed
    return bool((buf[:lead] == GUARD).all()) and bool((buf[lead + view.numel():] == GUARD).all())


def _raw_run(family, zs, zt, sliced, K, thr=1.5):
    """the entries themselves on [npix][K] rows placed by `place` -> (result floats, gradient), both on the CPU"""
    from cyhip import _lib, ops
    lib = _lib.load()
    npix = zs.shape[0]
    s, t = place(zs, sliced), place(zt, sliced)
    out, grad = place(2, sliced, fill=-5.0), place(npix * K, sliced, fill=-5.0)
    gscale, stream = torch.ones(1, device=DEV), ops._stream()
    index = torch.zeros(1, dtype=torch.int32, device=DEV)
    S, T, O, G = (x[0].data_ptr() for x in (s, t, out, grad))
    assert ops.wide_reg_plan("entropy", npix, K, align=4 if sliced else 16)["vec"] == (1 if sliced else 4)
    if family == "entropy":
        nb = lib.cy_softmax_entropy_row_ws_bytes(npix)
        ws = place(nb // 4, False, fill=0.0)
        _lib.call("cy_softmax_entropy_row_fwd", S, O, npix, K, EPS, ws[0].data_ptr(), nb, stream)
        _lib.call("cy_softmax_entropy_row_bwd", S, gscale.data_ptr(), G, npix, K, EPS, stream)
    elif family == "selfmse":
        nb = lib.cy_softmax_selfmse_row_ws_bytes(npix)
        ws = place(nb // 4, False, fill=0.0)
        _lib.call("cy_softmax_selfmse_row_fwd", S, O, npix, K, ws[0].data_ptr(), nb, stream)
        _lib.call("cy_softmax_selfmse_row_bwd", S, gscale.data_ptr(), G, npix, K, stream)
    elif family == "uamt":
        nb = lib.cy_uamt_mse_row_ws_bytes(npix)
        ws = place(nb // 4, False, fill=0.0)
        _lib.call("cy_uamt_mse_row_fwd", T, S, O, npix, K, thr, 1, ws[0].data_ptr(), nb, stream)
        _lib.call("cy_uamt_mse_row_bwd", T, S, O, gscale.data_ptr(), G, npix, K, thr, 1, stream)
    else:
        nb = lib.cy_softmax_mixmse_row_ws_bytes(1, npix)
        ws = place(nb // 4, False, fill=0.0)
        _lib.call("cy_softmax_mixmse_row_fwd", S, T, index.data_ptr(), 0.25, 0.75, O, 1, npix, K, ws[0].data_ptr(), nb,
                  stream)
        _lib.call("cy_softmax_mixmse_row_bwd", S, T, index.data_ptr(), 0.25, 0.75, gscale.data_ptr(), G, 1, npix, K,
                  stream)
    torch.cuda.synchronize()
    for name, pl in (("student", s), ("teacher", t), ("result", out), ("gradient", grad), ("workspace", ws)):
        assert intact(pl), f"{family}: the guards of the {name} were written"
    assert torch.equal(s[0].cpu(), zs.reshape(-1)) and torch.equal(t[0].cpu(), zt.reshape(-1))  # inputs are read only
    res = out[0].cpu()
    if family != "uamt":
        assert float(res[1]) == -5.0, "one float of result"
    g = grad[0].cpu()
    assert bool((g != -5.0).all()), "every gradient element was written"
    return res, g


@pytest.mark.parametrize("npix", [286, 1])
@pytest.mark.parametrize("family", ["entropy", "selfmse", "uamt", "mixmse"])
def test_slices_one_float_into_a_guarded_buffer(fx, family, npix):
    K = 20
    gen = torch.Generator().manual_seed(9 + npix)
    zs = torch.randn(npix, K, generator=gen) * 2
    zt = torch.randn(npix, K, generator=gen) * 3
    zt[:, 3] += 12  # peaked rows: every teacher entropy lies far below thr = 1.5
    kind = {"entropy": "ent", "selfmse": "pl", "uamt": "uamt", "mixmse": "ict"}[family]
    res_a, g_a = _raw_run(family, zs, zt, False, K)
    res_s, g_s = _raw_run(family, zs, zt, True, K)
    assert torch.equal(res_a, res_s), (family, res_a, res_s)  # the forward: the same bits in both forms
    if family == "uamt":
        assert float(res_a[1]) > 0, "a mask that is not empty"
    e = float((g_s.double() - g_a.double()).abs().max() / g_a.double().abs().max())
    print(f"{family} npix {npix}: scalar form against vector form, gradient e_max {e:.2e} "
          f"(bound {bound(fx.e_ref(kind)[1]):.2e}); result {res_a.tolist()}")
    assert e <= bound(fx.e_ref(kind)[1])


# ---------------------------------------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize("K", [20, 63])
def test_two_runs_give_the_same_bits(K):
    from cyhip.functions import MixSoftmaxMSEFn, SoftmaxEntropyFn, SoftmaxSelfMSEFn, UAMTLossFn
    thr = 0.85 * math.log(K)
    zs, zt = _smooth_inputs(torch.Generator().manual_seed(5), 3, K, 150, 150, thr)  # 67 500 pixels: two trips
    ztd, index = zt.to(DEV), torch.tensor([2, 0, 0])
    runs = []
    for _ in range(2):
        out = []
        for fn in (lambda z: SoftmaxEntropyFn.apply(z, EPS), SoftmaxSelfMSEFn.apply,
                   lambda z: UAMTLossFn.apply(ztd, z, thr, False)[0], lambda z: UAMTLossFn.apply(ztd, z, thr, True)[0],
                   lambda z: MixSoftmaxMSEFn.apply(z, ztd, index, 0.3, 0.7)):
            z = gpu_leaf(zs)
            loss = fn(z)
            loss.backward()
            out += [loss.detach().cpu(), z.grad.cpu()]
        runs.append(out)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- 7. hooks at K = 20
def _trainer_hook(hook, model=None, cur_epoch=0):
    """a trainer hook's epocher hook, adopted by a stand-in epocher"""
    from contrastyou.hooks.base import TrainerHook
    hook.register_trainer(_StepTrainer(model, sw.MAX_EPOCH))
    ep = _Epocher(cur_epoch, sw.MAX_EPOCH)
    out = ep.adopt(hook())
    type(TrainerHook).names.clear()
    return out, ep


def test_trainer_hooks_at_k20(fx):
    from contrastyou.hooks.base import TrainerHook
    from semi_seg.hooks import (EntropyMinTrainerHook, MeanTeacherTrainerHook, PseudoLabelTrainerHook,
                                UAMeanTeacherTrainerHook)
    type(TrainerHook).names.clear()
    K = 20
    zs, zt = fx.dec(f"K{K}_zs_i8d8"), fx.dec(f"K{K}_zt_i8d8")
    image = torch.zeros(sw.SHAPE[0], 1, *sw.SHAPE[1:], device=DEV)
    kw = dict(unlabeled_image=image, unlabeled_image_tf=image)

    hook, _ = _trainer_hook(EntropyMinTrainerHook(name="entropy", weight=0.5))
    z = gpu_leaf(zs)
    loss = _call(hook, z)
    loss.backward()
    check("EntropyMinTrainerHook", 2 * loss, fx[f"ent_K{K}_loss64"], 2 * z.grad, fx.t(f"ent_K{K}_g64"),
          fx.e_ref("ent"))

    hook, _ = _trainer_hook(PseudoLabelTrainerHook(name="plab", weight=0.5))
    z = gpu_leaf(zs)
    loss = _call(hook, z)
    loss.backward()
    check("PseudoLabelTrainerHook", 2 * loss, fx[f"pl_K{K}_loss64"], 2 * z.grad, fx.t(f"pl_K{K}_g64"), fx.e_ref("pl"))

    for hard in (False, True):
        key = f"uamt_K{K}_e4_h{int(hard)}"
        stored = sw.StoredTeacher(list(zt.to(DEV)))
        hook, ep = _trainer_hook(UAMeanTeacherTrainerHook(name="mt", model=stored, weight=0.5, hard_clip=hard),
                                 model=stored, cur_epoch=4)
        z = gpu_leaf(zs)
        loss = _call(hook, z, **kw)
        loss.backward()
        check(f"UAMeanTeacherTrainerHook hard {hard}", 2 * loss, fx[f"{key}_loss64"], 2 * z.grad, fx.t(f"{key}_g64"),
              fx.e_ref("uamt"))
        assert ep.summary(hook)["mask"] == float(np.float32(int(fx[f"{key}_count"]) / P_FIX))

    # coverage only (SoftmaxMSEFn's row form, there before the wide regularisers): the plain mean teacher
    for hard in (False, True):
        stored = sw.StoredTeacher([zt[0].to(DEV)])
        hook, _ = _trainer_hook(MeanTeacherTrainerHook(name="mt", model=stored, weight=0.5, hard_clip=hard),
                                model=stored)
        z = gpu_leaf(zs)
        loss = _call(hook, z, **kw)
        loss.backward()
        l64, g64 = eval64(lambda s: mt64(zt[0].double(), s, hard), zs)
        check(f"MeanTeacherTrainerHook hard {hard}", 2 * loss, l64, 2 * z.grad, g64, fx.e_ref("uamt"))
    type(TrainerHook).names.clear()


def test_ict_epocher_hook_at_k20(fx):
    from contrastyou.utils.utils import fix_all_seed_within_context
    from cyhip import ops
    from mixup_fixture import Conv1x1
    from semi_seg.hooks.mt import EMAUpdater, _ICTMeanTeacherEpocherHook
    from semi_seg.hooks.utils import mixup_draw
    K, B, H, W, seed = 20, 3, 13, 11, 77
    gen = torch.Generator().manual_seed(20)
    w, b, tw, tb = (torch.randn(K, generator=gen) * s for s in (2, 1, 2, 1))
    image, image_tf = torch.rand(B, 1, H, W, generator=gen), torch.rand(B, 1, H, W, generator=gen)
    model, teacher = Conv1x1(w, b).to(DEV), Conv1x1(tw, tb).to(DEV)
    ep = _Epocher()
    hook = ep.adopt(_ICTMeanTeacherEpocherHook(name="ict", weight=1.0, model=model, teacher_model=teacher,
                                               updater=EMAUpdater()))
    value = hook(unlabeled_tf_logits=None, unlabeled_image=image.to(DEV), unlabeled_image_tf=image_tf.to(DEV),
                 seed=seed)
    value.backward()
    assert teacher.w.grad is None and teacher.b.grad is None
    # f64: the same draw, the f32 mixed image the student saw, the f32 weights cast up
    with fix_all_seed_within_context(seed):
        lam, index = mixup_draw(2 * B, alpha=_ICTMeanTeacherEpocherHook.MIX_ALPHA)
    w_self, w_other = (float(np.float32(v)) for v in ops.mix_weights(lam))
    x = torch.cat([image, image_tf], 0)
    mixed = (w_self * x + w_other * x[index]).double()  # (f32, as ops.mix_images forms it)
    m64, t64 = Conv1x1(w, b, torch.float64), Conv1x1(tw, tb, torch.float64)
    l64 = ict64(m64(mixed), t64(x.double()).detach(), index, w_self, w_other)
    l64.backward()
    got = torch.cat([model.w.grad.flatten(), model.b.grad.flatten()])
    want = torch.cat([m64.w.grad.flatten(), m64.b.grad.flatten()])
    check("ICT hook K 20", value, l64.detach(), got, want, fx.e_ref("ict"))


# ---------------------------------------------------------------------------------------------- 8. end to end
C_TRUE, MULT = 5, 4  # the 5-class datasets at multiplier 4: 20 outputs


def _groups():
    return [list(range(c * MULT, (c + 1) * MULT)) for c in range(C_TRUE)]


def _batches(steps=1):
    """(labeled batches, unlabeled batches, one validation batch)"""
    g = torch.Generator().manual_seed(31)
    return ([blob_batch(2, 32, C_TRUE, g) for _ in range(steps)], [blob_batch(3, 32, C_TRUE, g) for _ in range(steps)],
            blob_batch(2, 32, C_TRUE, g, views=1))


def _unfused_entropy_hook():
    from semi_seg.hooks.entmin import EntropyMinTrainerHook, _EntropyEpocherHook

    class Unfused(_EntropyEpocherHook):
        def _call_implementation(self, *, unlabeled_logits_tf, **kwargs):
            loss = self._criterion(unlabeled_logits_tf.float().softmax(1))
            self.meters["loss"].add(loss.detach())
            return self._weight * loss

    class UnfusedTrainHook(EntropyMinTrainerHook):
        def __call__(self):
            return Unfused(name=self._hook_name, weight=self._weight, criterion=self._criterion)

    return UnfusedTrainHook


def _unfused_uamt_hook():
    from semi_seg.hooks.mt import UAMeanTeacherTrainerHook, _UAMeanTeacherEpocherHook, uamt_threshold

    class Unfused(_UAMeanTeacherEpocherHook):
        def _call_implementation(self, *, unlabeled_tf_logits, unlabeled_image, seed, affine_transformer, **kwargs):
            zt = self._aggregate_predictions(unlabeled_image=unlabeled_image, N=4,
                                             affine_transformer=affine_transformer, seed=seed)
            thr = uamt_threshold(unlabeled_tf_logits.shape[1], self.cur_epoch, self.max_epoch)
            t = zt.float().softmax(1)
            mask = (entropy_of(t) < thr).float()
            if self._hard_clip:
                t = F.one_hot(t.argmax(1), t.shape[1]).movedim(-1, 1).float()
            e = torch.nn.MSELoss(reduction="none")(t, unlabeled_tf_logits.float().softmax(1)).mean(1)
            loss = (e * mask).mean() / (mask.mean() + 1e-2)
            self.meters["loss"].add(loss.detach())
            self.meters["mask"].add(mask.mean())
            return self._weight * loss

    class UnfusedTrainHook(UAMeanTeacherTrainerHook):
        def __call__(self):
            return Unfused(name=self._hook_name, weight=self._weight, model=self.trainer._model,
                           teacher_model=self._teacher_model, updater=self._updater, hard_clip=self._hard_clip)

    return UnfusedTrainHook


def _recipe(kind, model, fused):
    """the hooks of the reference's multicore sweep (entropy-min + mean teacher, hard_clip + IIC), or UA-MT"""
    from semi_seg.hooks import (EntropyMinTrainerHook, UAMeanTeacherTrainerHook, create_iid_seg_hook, create_mt_hook)
    if kind == "sweep":
        ent = (EntropyMinTrainerHook if fused else _unfused_entropy_hook())(name="entropy", weight=0.1)
        return [ent, create_mt_hook(model=model, weight=5.0, alpha=0.99, weight_decay=1e-6, hard_clip=True),
                create_iid_seg_hook(weight=0.1)]
    cls = UAMeanTeacherTrainerHook if fused else _unfused_uamt_hook()
    return [cls(name="mt", model=model, weight=10.0, alpha=0.99, weight_decay=1e-6, hard_clip=False)]


def _mc_step(kind, sd0, lab, unl, *, fused=True, graph=False, bf16=False):
    """MultiCoreTrainEpocher steps, one per batch, at cur_epoch = max_epoch (the UA-MT threshold is ln K: an untrained
    network's mask is not empty) -> (parameters, metrics, replayed)"""
    from contrastyou.amp import BF16Scaler
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.losses.multicore_loss import MultiCoreKL
    from contrastyou.optim import RAdam
    from cyhip import graphed
    from semi_seg.epochers.features import MultiCoreTrainEpocher
    default = graphed.GRAPH_STEP
    graphed.GRAPH_STEP = graph
    try:
        type(TrainerHook).names.clear()
        model = UNet(input_dim=1, num_classes=C_TRUE * MULT, max_channel=128)
        model.load_state_dict(sd0)
        model.to(DEV)
        torch.manual_seed(3)
        hooks = [h.to(DEV) for h in _recipe(kind, model, fused)]
        trainer = _StepTrainer(model, max_epoch=10)
        for h in hooks:
            h.register_trainer(trainer)
        opt = RAdam([{"params": list(model.parameters())}], lr=1e-3, weight_decay=1e-5)
        scaler = BF16Scaler() if bf16 else torch.amp.GradScaler("cuda", enabled=False)
        ep = MultiCoreTrainEpocher(model=model, optimizer=opt, labeled_loader=Loader(lab), unlabeled_loader=Loader(unl),
                                   sup_criterion=MultiCoreKL(_groups()), num_batches=len(lab), cur_epoch=10,
                                   device=DEV, two_stage=True, disable_bn=False, scaler=scaler, accumulate_iter=1)
        ep.init(trainer)
        assert ep.num_classes == C_TRUE
        random.seed(5)
        with ep.register_hook(*[h() for h in hooks]):
            ep.run()
        torch.cuda.synchronize()
        replayed = any(isinstance(v, graphed.GraphedTwoPass) for v in model.__dict__.get("_cy_graphed", {}).values())
        params = {k: v.detach().float().cpu() for k, v in model.named_parameters()}
        return params, ep.get_metric(), replayed
    finally:
        graphed.GRAPH_STEP = default
        type(TrainerHook).names.clear()


@pytest.fixture(scope="module")
def sd0():
    from contrastyou.arch import UNet
    torch.manual_seed(11)
    return {k: v.clone() for k, v in UNet(input_dim=1, num_classes=C_TRUE * MULT, max_channel=128).state_dict().items()}


@pytest.mark.parametrize("kind", ["sweep", "uamt"])
def test_a_multicore_step_fused_against_the_torch_composition(sd0, kind):
    lab, unl, _ = _batches()
    p_f, m_f, rep_f = _mc_step(kind, sd0, lab, unl, fused=True)
    p_t, m_t, _ = _mc_step(kind, sd0, lab, unl, fused=False)
    assert not rep_f
    print("fused", m_f, "\ntorch", m_t)
    groups = (("entropy", "loss"), ("mt", "loss"), ("iid", "mi")) if kind == "sweep" else (("mt", "loss"),)
    for name, a, b in [("reg_loss", m_f["semi"]["reg_loss"], m_t["semi"]["reg_loss"])] + [
            (g, m_f[g][key], m_t[g][key]) for g, key in groups]:
        e = abs(a - b) / abs(b)
        print(f"{kind} {name}: {a:.9g} vs {b:.9g}  e {e:.2e}")
        assert math.isfinite(a) and a != 0 and e <= 1e-6, (name, e)
    if kind == "uamt":
        assert 0 < m_f["mt"]["mask"] <= 1 and m_f["mt"]["mask"] == m_t["mt"]["mask"]
    worst = max(float((p_f[k] - p_t[k]).abs().max() / p_t[k].abs().max()) for k in p_t)
    moved = max(float((p_f[k] - sd0[k].float()).abs().max()) for k in p_f)
    print(f"{kind}: parameters after the RAdam step: worst relative distance {worst:.2e}; largest move {moved:.2e}")
    assert moved > 0 and worst <= 1e-4


@pytest.mark.parametrize("kind", ["sweep", "uamt"])
def test_graph_replayed_multicore_steps_equal_eager_steps(sd0, kind):
    """the pattern of tests/test_gpu_semi_baselines.py: the hooks (and the teachers' forwards) run in the eager section
    between the two graph replays; three steps either way end in the same bits"""
    lab, unl, _ = _batches(3)
    p_e, m_e, rep_e = _mc_step(kind, sd0, lab, unl, graph=False, bf16=True)
    p_g, m_g, rep_g = _mc_step(kind, sd0, lab, unl, graph=True, bf16=True)
    assert rep_g and not rep_e, "the second run must have captured and replayed the passes"
    for k in p_e:
        assert torch.equal(p_e[k], p_g[k]), k
    assert m_e["semi"]["reg_loss"] == m_g["semi"]["reg_loss"] and np.isfinite(m_e["semi"]["reg_loss"])
    assert m_e["mt"] == m_g["mt"]


@pytest.mark.parametrize("kind", ["sweep", "uamt"])
def test_multicore_trainer_runs_an_epoch_with_the_wide_regularisers(tmp_path, kind):
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.losses.multicore_loss import MultiCoreKL
    from semi_seg.trainers.features import MulticoreTrainer
    (lab,), (unl,), val = _batches()
    val = {k: v[0] for k, v in val.items()}
    cfg = {"Arch": {"true_num_classes": C_TRUE, "max_channel": 128},
           "Optim": {"name": "RAdam", "lr": 1e-4, "weight_decay": 1e-5},
           "Scheduler": {"multiplier": 100, "warmup_max": 1}, "Trainer": {"name": "semi"}}
    type(TrainerHook).names.clear()
    torch.manual_seed(12)
    model = UNet(input_dim=1, num_classes=C_TRUE * MULT, max_channel=128)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    tr = MulticoreTrainer(model=model, labeled_loader=OneBatchLoader(lab), unlabeled_loader=OneBatchLoader(unl),
                          val_loader=OneBatchLoader(val), test_loader=OneBatchLoader(val),
                          criterion=MultiCoreKL(_groups()), save_dir=str(tmp_path), max_epoch=1, num_batches=1,
                          device=DEV, disable_bn=False, two_stage=True, config=cfg, enable_scale=False)
    with tr.register_hook(*_recipe(kind, model, True)):
        tr.init()
        tr.start_training()
    assert tr._cur_epoch == 1
    assert any(not torch.equal(v.detach().cpu(), before[k]) for k, v in model.named_parameters())
    assert all(torch.isfinite(v).all() for v in model.state_dict().values())
    lines = (tmp_path / "storage.csv").read_text().strip().splitlines()
    row = dict(zip(lines[0].split(","), lines[1].split(",")))
    cols = ["tra/semi/sup_loss", "tra/semi/reg_loss", "tra/mt/loss"] + (
        ["tra/entropy/loss", "tra/iid/mi"] if kind == "sweep" else ["tra/mt/mask"])
    for col in cols:
        assert col in row, (col, lines[0])
        print(col, row[col])
        assert math.isfinite(float(row[col])), (col, row[col])
    type(TrainerHook).names.clear()
