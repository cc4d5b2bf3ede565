"""The adversarial baseline on the GPU: the kernels of csrc/cy_disc.hip, `Discriminator`, `AdversarialEpocher`.

Against tests/golden/adversarial.npz (the reference's `Discriminator` under `nn.BCELoss` on the CPU in f32 and f64,
tests/golden/gen_goldens_adv.py; layout: tests/adversarial_fixture.py) and against f64 CPU formulas written here.

Tolerance rule (the one of tests/test_gpu_semi_baselines.py).  The yardstick is the reference's own f32-to-f64 distance:
    e(x) = |x - x64| relative: 2-norm, and element-wise maximum over max|x64|; |.| / |loss64| for a loss
    require e_hip <= max(4 * e_ref, 1e-6), e_ref = the largest value over the fixture's cases of the same kind
Kinds of the fixture: "out" (discriminator outputs), "gen" (generator_err, its gradient on the logits), "dis"
(disc_loss, parameter gradients), "buf" (BatchNorm running statistics).  A kernel no fixture kind speaks for (softmax +
concat, BatchNorm + LeakyReLU, LeakyReLU) is measured against torch's own f32 CPU evaluation of the same formula on the
same inputs: e_ref = that evaluation's distance to f64.  The sigmoid + BCE kernel is the "gen" kind (generator_err is
this loss).  No element is left out of any comparison; every figure is printed before it is asserted.

The f64 gradient on the unlabeled logits is recomputed on the CPU (adversarial_fixture.generator_gradient64) and pinned
to the reference's by the fixture's norm / maximum / projections before anything is compared with it.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import disc_flat_cases as dc
from adversarial_fixture import (ARMS, BN_ROWS, BUFFERS, CASES, HIDDEN, K, PARAMS, SCORE_SHAPE, StoredLogits, arm_tag,
                                 decode, generator_gradient64, pin, replica, state_dict_of)
from test_gpu_hooks_dice import Loader, blob_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR, FACTOR = 1e-6, 4.0
SLOPE, EPS, MOMENTUM = 0.2, 1e-5, 0.1


@pytest.fixture(scope="module")
def fx(golden_dir):
    data = np.load(golden_dir / "adversarial.npz")

    class Fx:
        files = data.files
        raw = data

        def __getitem__(self, k):
            return data[k]

        def t(self, k):
            return torch.from_numpy(np.asarray(data[k]))

        def inputs(self, case):
            return tuple(decode(k, data[f"{case}_{k}"]) for k in ("image_i8d32", "lab_i8d8", "unl_i8d8"))

        def e_ref(self, kind):
            """[2-norm, max, loss]: the largest over the fixture's cases of this kind"""
            rows = [data[k] for k in data.files if k.endswith(f"_{kind}_e_ref")]
            assert len(rows) == len(CASES) * len(ARMS), kind
            return np.max(np.stack(rows), axis=0)

        def sd(self, arm):
            return state_dict_of(data, arm)

    return Fx()


@pytest.fixture(scope="module")
def gen64(fx):
    """{(case, arm): (generator_err, its gradient on the unlabeled logits)}, f64, recomputed once and pinned"""
    out = {}
    for case in CASES:
        image, _, unl = fx.inputs(case)
        for arm in ARMS:
            key = f"{case}_{arm_tag(arm)}"
            loss, g = generator_gradient64(fx.sd(arm), arm, image, unl)
            norm, gmax, proj = pin(g)
            assert abs(float(loss) - float(fx[f"{key}_gen_loss64"])) <= 1e-9 * float(loss), key
            assert abs(norm - float(fx[f"{key}_gen_g64_norm"])) <= 1e-9 * norm, key
            assert abs(gmax - float(fx[f"{key}_gen_g64_max"])) <= 1e-9 * gmax, key
            assert np.abs(proj - fx[f"{key}_gen_g64_proj"]).max() <= 1e-9 * norm, key
            out[(case, arm)] = (loss, g)
    return out


def bound(e_ref):
    return max(FACTOR * float(e_ref), FLOOR)


def cpu64(t):
    return t.detach().double().cpu()


def dist(got, want):
    """(2-norm, max) relative distance of `got` to the f64 tensor `want`; every element takes part"""
    got, want = cpu64(got), cpu64(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all()
    d = got - want
    n, m = float(want.norm()), float(want.abs().max())
    if n == 0.0:
        return float(d.norm()), float(d.abs().max())
    return float(d.norm() / n), float(d.abs().max() / m)


def check_tensor(what, got, want, e_ref):
    e2, emax = dist(got, want)
    print(f"{what}: e_2 {e2:.2e} (bound {bound(e_ref[0]):.2e})  e_max {emax:.2e} (bound {bound(e_ref[1]):.2e})")
    fails = [f"{n} {e:.2e}" for n, e, b in (("e_2", e2, e_ref[0]), ("e_max", emax, e_ref[1])) if e > bound(b)]
    assert not fails, f"{what}: {fails}"


def check_loss(what, loss, loss64, e_ref_loss):
    loss, loss64 = float(loss), float(loss64)
    assert math.isfinite(loss), (what, loss)
    e = abs(loss - loss64) / abs(loss64)
    print(f"{what}: loss {loss:.9g} vs {loss64:.9g}  e_loss {e:.2e} (bound {bound(e_ref_loss):.2e})")
    assert e <= bound(e_ref_loss), f"{what}: e_loss {e:.2e}"


def measured(x32, x64):
    """[2-norm, max] distance of torch's f32 CPU evaluation to its f64 one"""
    return list(dist(x32, x64))


def gpu_leaf(t):
    return t.float().to(DEV).requires_grad_(True)


# ---------------------------------------------------------------------------------------------- 1. softmax + concat
def _cat_formula(image, z, G):
    """-> (out, dz) of out = cat([image, softmax(z)], 1), L = sum(out * G), in the dtype of z"""
    z = z.clone().requires_grad_(True)
    p = z.softmax(1)
    out = p if image is None else torch.cat([image.to(z.dtype), p], 1)
    (out * G.to(z.dtype)).sum().backward()
    return out.detach(), z.grad


def _softmax_cat_check(Kc, Ci, N, H, W):
    """rows h < 3 are all-zero logits"""
    from cyhip.functions import SoftmaxCatFn
    gen = torch.Generator().manual_seed(100 * Kc + Ci)
    z = torch.randn(N, Kc, H, W, generator=gen) * (torch.rand(N, 1, H, W, generator=gen) * 4)
    z[:, :, :3] = 0
    image = torch.rand(N, Ci, H, W, generator=gen) if Ci else None
    G = torch.randn(N, Ci + Kc, H, W, generator=gen)
    out64, dz64 = _cat_formula(None if image is None else image.double(), z.double(), G)
    out32, dz32 = _cat_formula(image, z, G)
    zg = gpu_leaf(z)
    out = SoftmaxCatFn.apply(None if image is None else image.to(DEV), zg)
    assert out.shape == (N, Ci + Kc, H, W)
    (out * G.to(DEV)).sum().backward()
    check_tensor(f"softmax+cat K {Kc} Ci {Ci} fwd", out, out64, measured(out32, out64))
    check_tensor(f"softmax+cat K {Kc} Ci {Ci} bwd", zg.grad, dz64, measured(dz32, dz64))
    if Ci:
        assert torch.equal(out[:, :Ci].cpu(), image)  # the image columns are copies
    assert torch.equal(out[:, Ci:, :3].cpu(), torch.full((N, Kc, 3, W), 1.0 / Kc).float())  # a zero row: exactly 1 / K


@pytest.mark.parametrize("Ci", dc.CAT_CI)
@pytest.mark.parametrize("Kc", dc.CAT_K)
def test_softmax_cat_kernel(Kc, Ci):
    """npix = 286 = 2 x 13 x 11: one full block plus a tail; Ci up to CI_MAX"""
    _softmax_cat_check(Kc, Ci, *dc.CAT_SMALL_NHW)


@pytest.mark.parametrize("Kc,Ci", [c[:2] for c in dc.CAT_PAST_CAP])
def test_softmax_cat_kernel_past_the_grid_cap(Kc, Ci):
    """525 625 pixels: the grid-stride loops of both kernels go round a second time, in each of their three forms"""
    _softmax_cat_check(Kc, Ci, 1, dc.CAT_SIDE, dc.CAT_SIDE)


# ---------------------------------------------------------------------------------------------- 2. BatchNorm + LeakyReLU
def _bn_formula(x, gamma, beta, rm, rv, dy):
    """training-mode batch_norm + leaky_relu in the dtype of x -> (y, running_mean, running_var, dx, dgamma, dbeta)"""
    x, gamma, beta = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    rm, rv = rm.clone(), rv.clone()
    y = F.leaky_relu(F.batch_norm(x, rm, rv, gamma, beta, True, MOMENTUM, EPS), SLOPE)
    (y * dy).sum().backward()
    return y.detach(), rm, rv, x.grad, gamma.grad, beta.grad


@pytest.mark.parametrize("M,C", list(dc.BN_SHAPES))
def test_bn_lrelu_kernels(M, C):
    """column 0 is exactly constant, column 1 sits at 1e3 (what a one-pass f32 variance would get wrong); what each
    shape reaches (16- and 4-byte row accesses, column tiles, the capped row chunks): tests/disc_flat_cases.py"""
    from cyhip.functions import BNLeakyReLUFn
    gen = torch.Generator().manual_seed(7 * M + C)
    x = torch.randn(M, C, generator=gen) * (0.5 + torch.rand(1, C, generator=gen)) + torch.randn(1, C, generator=gen)
    x[:, 0] = 0.75
    x[:, 1] += 1e3
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)
    rm, rv = 0.3 * torch.randn(C, generator=gen), 0.5 + torch.rand(C, generator=gen)
    dy = torch.randn(M, C, generator=gen)
    names = ("y", "running_mean", "running_var", "dx", "dgamma", "dbeta")
    ref64 = _bn_formula(x.double(), gamma.double(), beta.double(), rm.double(), rv.double(), dy.double())
    ref32 = _bn_formula(x, gamma, beta, rm, rv, dy)
    # the kernels see the rows as a [1, C, M, 1] map with NHWC memory: the same [M][C] rows
    xg, gg, bg = (gpu_leaf(t) for t in (x.t().reshape(1, C, M, 1), gamma, beta))
    rmg, rvg, nbt = rm.to(DEV), rv.to(DEV), torch.tensor(5, device=DEV)
    y = BNLeakyReLUFn.apply(xg, gg, bg, rmg, rvg, nbt, True, MOMENTUM, EPS, SLOPE)
    (y * dy.t().reshape(1, C, M, 1).to(DEV)).sum().backward()
    got = (y.reshape(C, M).t(), rmg, rvg, xg.grad.reshape(C, M).t(), gg.grad, bg.grad)
    assert int(nbt) == 6
    # the constant column (invstd = 316 in dx), the column at 1e3 (running_mean = 100) and the ordinary columns are
    # compared apart: each against its own norm and maximum, so that neither special column hides the others
    for cols, tag in ((slice(0, 1), "constant column"), (slice(1, 2), "column at 1e3"), (slice(2, None), "other columns")):
        for name, g, r32, r64 in zip(names, got, ref32, ref64):
            check_tensor(f"BN+LReLU {M}x{C} {name}, {tag}", g[..., cols], r64[..., cols],
                         measured(r32[..., cols], r64[..., cols]))
    assert torch.equal(got[0][:, 0].cpu(), torch.full((M,), 1.0) * F.leaky_relu(beta[0], SLOPE))  # constant column


def test_bn_lrelu_eval_mode_uses_the_running_statistics():
    from cyhip.functions import BNLeakyReLUFn
    gen = torch.Generator().manual_seed(31)
    M, C = 60, 24
    x, dy = torch.randn(M, C, generator=gen), torch.randn(M, C, generator=gen)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)
    rm, rv = 0.3 * torch.randn(C, generator=gen), 0.5 + torch.rand(C, generator=gen)

    def formula(dt):
        xs, g, b = (t.to(dt).clone().requires_grad_(True) for t in (x, gamma, beta))
        y = F.leaky_relu(F.batch_norm(xs, rm.to(dt), rv.to(dt), g, b, False, MOMENTUM, EPS), SLOPE)
        (y * dy.to(dt)).sum().backward()
        return y.detach(), xs.grad, g.grad, b.grad

    r64, r32 = formula(torch.float64), formula(torch.float32)
    xg, gg, bg = (gpu_leaf(t) for t in (x.t().reshape(1, C, M, 1), gamma, beta))
    rmg, rvg, nbt = rm.to(DEV), rv.to(DEV), torch.tensor(2, device=DEV)
    y = BNLeakyReLUFn.apply(xg, gg, bg, rmg, rvg, nbt, False, MOMENTUM, EPS, SLOPE)
    (y * dy.t().reshape(1, C, M, 1).to(DEV)).sum().backward()
    assert int(nbt) == 2 and torch.equal(rmg.cpu(), rm) and torch.equal(rvg.cpu(), rv)
    got = (y.reshape(C, M).t(), xg.grad.reshape(C, M).t(), gg.grad, bg.grad)
    for name, g, a, b in zip(("y", "dx", "dgamma", "dbeta"), got, r32, r64):
        check_tensor(f"BN+LReLU eval {name}", g, b, measured(a, b))
    # detached parameters: the sums are not needed and not computed; the data gradient has the same bits
    x2 = gpu_leaf(x.t().reshape(1, C, M, 1))
    y2 = BNLeakyReLUFn.apply(x2, gg.detach(), bg.detach(), rmg, rvg, nbt, False, MOMENTUM, EPS, SLOPE)
    (y2 * dy.t().reshape(1, C, M, 1).to(DEV)).sum().backward()
    assert torch.equal(y2, y) and torch.equal(x2.grad, xg.grad)


# ---------------------------------------------------------------------------------------------- 3. plain LeakyReLU
def _lrelu_check(n, on_device):
    """`on_device` puts the f32 input [1, 1, n, 1] on the GPU as a leaf"""
    from cyhip.functions import LeakyReLUFn
    gen = torch.Generator().manual_seed(n)
    x, dy = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    x[0] = -1.5
    if n > 4:
        x[1], x[2], x[-1] = 0.0, -0.0, -0.0
    want = torch.where(x.double() > 0, x.double(), x.double() * SLOPE)
    dwant = torch.where(x.double() > 0, dy.double(), dy.double() * SLOPE)
    xc = x.clone().requires_grad_(True)
    y32 = F.leaky_relu(xc, SLOPE)
    (y32 * dy).sum().backward()
    xg = on_device(x.reshape(1, 1, n, 1))
    y = LeakyReLUFn.apply(xg, SLOPE)
    (y * dy.reshape(1, 1, n, 1).to(DEV)).sum().backward()
    check_tensor(f"LeakyReLU n {n} fwd", y.reshape(n), want, measured(y32.detach(), want))
    check_tensor(f"LeakyReLU n {n} bwd", xg.grad.reshape(n), dwant, measured(xc.grad, dwant))
    if n > 4:
        yc = y.reshape(n).cpu()
        assert yc[1] == 0 and not torch.signbit(yc[1]) and yc[2] == 0 and torch.signbit(yc[2]) and torch.signbit(yc[-1])
        gz = xg.grad.reshape(n).cpu()
        assert torch.equal(gz[[1, 2, -1]], (dy[[1, 2, -1]] * torch.tensor(SLOPE)))  # a zero input: the slope side


@pytest.mark.parametrize("n", list(dc.LRELU_ALIGNED))
def test_leaky_relu_kernels(n):
    """16-byte aligned buffers: the vector kernel over n // 4 vectors, the scalar kernel over the tail"""
    def aligned(x):
        xg = gpu_leaf(x)
        assert xg.data_ptr() % 16 == 0
        return xg

    _lrelu_check(n, aligned)


def test_leaky_relu_scalar_kernel_alone_past_the_grid_cap():
    """the input is a view one float into its allocation: no 16-byte access is possible, the scalar kernel runs as the
    whole launch, forward and backward, and past its cap"""
    n = dc.LRELU_MISALIGNED

    def misaligned(x):
        xg = dc.one_float_in(n, DEV)
        xg.copy_(x.reshape(n))
        xg = xg.reshape(x.shape).requires_grad_(True)
        assert xg.data_ptr() % 16 == 4 and xg.is_leaf
        return xg

    _lrelu_check(n, misaligned)


# ---------------------------------------------------------------------------------------------- 4. sigmoid + BCE
def _bce64(s, label, scale):
    """-> (loss, dloss * scale / ds), f64: mean of min(softplus(-+s), 100); 0 where clamped"""
    s = s.double()
    t = -s if label == 1 else s
    sp = F.softplus(t, beta=1.0, threshold=1e9)
    loss = torch.minimum(sp, torch.tensor(100.0, dtype=torch.float64)).mean()
    d = torch.sigmoid(s) - label if label == 0 else -torch.sigmoid(-s)
    return loss, torch.where(sp > 100.0, torch.zeros_like(d), d) * scale / s.numel()


def _bce_check(what, fx, s, label):
    from cyhip.functions import SigmoidBCEFn
    sg = gpu_leaf(s)
    loss = SigmoidBCEFn.apply(sg, float(label))
    (1.7 * loss).backward()
    l64, g64 = _bce64(s, label, 1.7)
    e = fx.e_ref("gen")
    check_loss(what, loss.detach(), l64, e[2])
    check_tensor(what + " grad", sg.grad, g64, e)
    return loss.detach().cpu(), sg.grad.cpu()


@pytest.mark.parametrize("label", [1, 0])
@pytest.mark.parametrize("n", list(dc.BCE_SIZES))
def test_sigmoid_bce_kernels(fx, n, label):
    gen = torch.Generator().manual_seed(10 * n + label)
    s = (torch.rand(n, generator=gen) * 24 - 12).reshape(1, 1, n, 1)
    _bce_check(f"sigmoid+BCE n {n} label {label}", fx, s, label)


@pytest.mark.parametrize("label", [1, 0])
def test_sigmoid_bce_far_scores(fx, label):
    """+-20: 1 - sigmoid(s) is not formed, so softplus(-20) = 2.06e-9 survives (the f32 reference path rounds
    sigmoid(20) to 1); +-120: the clamp at 100 and the zero gradient there"""
    s20 = torch.tensor([20.0, -20.0, 0.5, -3.0, 7.0, -7.0]).reshape(1, 1, 6, 1)
    loss, _ = _bce_check(f"sigmoid+BCE +-20 label {label}", fx, s20, label)
    only = torch.tensor([20.0 if label == 1 else -20.0]).reshape(1, 1, 1, 1)
    tiny, _ = _bce_check(f"sigmoid+BCE one score label {label}", fx, only, label)
    assert 2.0e-9 < float(tiny) < 2.1e-9
    s120 = torch.tensor([120.0, -120.0, 1.0, -2.0, 100.0, -100.0, 101.0, -101.0]).reshape(1, 1, 8, 1)
    loss, grad = _bce_check(f"sigmoid+BCE +-120 label {label}", fx, s120, label)
    clamped = [1, 7] if label == 1 else [0, 6]  # -s (label 1) or s (label 0) beyond 100
    g = grad.reshape(8)
    assert all(float(g[i]) == 0.0 for i in clamped), g
    assert float(g[2]) != 0.0 and float(g[3]) != 0.0, g
    assert float(loss) > 200.0 / 8  # two clamped terms of exactly 100 each, and more


def test_two_runs_of_the_kernels_give_the_same_bits():
    from cyhip.functions import BNLeakyReLUFn, SigmoidBCEFn
    gen = torch.Generator().manual_seed(77)
    M, C = 3000, 128
    x, dy = torch.randn(1, C, M, 1, generator=gen), torch.randn(1, C, M, 1, generator=gen).to(DEV)
    s = torch.randn(1, 1, 70000, 1, generator=gen) * 5
    runs = []
    for _ in range(2):
        xg, gg, bg = gpu_leaf(x), gpu_leaf(torch.ones(C)), gpu_leaf(torch.zeros(C))
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        y = BNLeakyReLUFn.apply(xg, gg, bg, rm, rv, None, True, MOMENTUM, EPS, SLOPE)
        (y * dy).sum().backward()
        sg = gpu_leaf(s)
        loss = SigmoidBCEFn.apply(sg, 0.0)
        loss.backward()
        runs.append([t.detach().cpu() for t in (y, rm, rv, xg.grad, gg.grad, bg.grad, loss, sg.grad)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_two_runs_past_the_caps_give_the_same_bits():
    """capped row chunks of the BatchNorm sums; f64 partials of more than one trip in the BCE forward"""
    from cyhip.functions import BNLeakyReLUFn, SigmoidBCEFn
    gen = torch.Generator().manual_seed(78)
    M, C = dc.SAME_BITS_BN
    x, dy = torch.randn(1, C, M, 1, generator=gen), torch.randn(1, C, M, 1, generator=gen).to(DEV)
    scores = [torch.randn(1, 1, n, 1, generator=gen) * 5 for n in dc.SAME_BITS_BCE]
    runs = []
    for _ in range(2):
        xg, gg, bg = gpu_leaf(x), gpu_leaf(torch.ones(C)), gpu_leaf(torch.zeros(C))
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        y = BNLeakyReLUFn.apply(xg, gg, bg, rm, rv, None, True, MOMENTUM, EPS, SLOPE)
        (y * dy).sum().backward()
        out = [y, rm, rv, xg.grad, gg.grad, bg.grad]
        for s, label in zip(scores, (0.0, 1.0)):
            sg = gpu_leaf(s)
            loss = SigmoidBCEFn.apply(sg, label)
            loss.backward()
            out += [loss, sg.grad]
        runs.append([t.detach().cpu() for t in out])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- 5. the module
def _discriminator(fx, arm, train=True):
    from contrastyou.arch.discriminator import Discriminator
    dis = Discriminator(5 if arm else K, HIDDEN)
    dis.load_state_dict(fx.sd(arm), strict=True)
    dis.to(DEV)
    return dis.train(train)


@pytest.mark.parametrize("arm", ARMS, ids=[arm_tag(a) for a in ARMS])
@pytest.mark.parametrize("case", list(CASES))
def test_discriminator_step_against_the_reference(fx, gen64, case, arm):
    """the three discriminator forwards of one step in the step's order: generator pass with the gradient on the
    logits, then the two detached passes with the parameter gradients; the buffers after the three"""
    from cyhip.functions import SigmoidBCEFn
    key = f"{case}_{arm_tag(arm)}"
    image, lab, unl = fx.inputs(case)
    img = image.to(DEV) if arm else None
    dis = _discriminator(fx, arm)
    z = gpu_leaf(unl)
    gen = SigmoidBCEFn.apply(dis.scores_from_logits(img, z, param_grads=False), 1.0)
    gen.backward()
    assert all(p.grad is None for p in dis.parameters())  # detached parameters: nothing accumulated
    l64, g64 = gen64[(case, arm)]
    check_loss(f"{key} generator_err", gen.detach(), l64, fx.e_ref("gen")[2])
    check_tensor(f"{key} d generator_err / d logits", z.grad, g64, fx.e_ref("gen"))
    s_lab = dis.scores_from_logits(img, lab.to(DEV))
    s_unl = dis.scores_from_logits(img, unl.to(DEV))
    assert tuple(s_lab.shape) == SCORE_SHAPE[case]
    loss = SigmoidBCEFn.apply(s_lab, 1.0) + SigmoidBCEFn.apply(s_unl, 0.0)
    loss.backward()
    check_tensor(f"{key} output labeled", torch.sigmoid(s_lab), fx.t(f"{key}_out_lab64"), fx.e_ref("out"))
    check_tensor(f"{key} output unlabeled", torch.sigmoid(s_unl), fx.t(f"{key}_out_unl64"), fx.e_ref("out"))
    check_loss(f"{key} disc_loss", loss.detach(), fx[f"{key}_dis_loss64"], fx.e_ref("dis")[2])
    grads = dict(dis.named_parameters())
    assert list(grads) == list(PARAMS)
    for name in PARAMS:
        check_tensor(f"{key} d disc_loss / d {name}", grads[name].grad, fx.t(f"{key}_dis_g64_{name}"), fx.e_ref("dis"))
    bufs = dict(dis.named_buffers())
    assert list(bufs) == list(BUFFERS)
    for name in BUFFERS:
        want = fx.t(f"{key}_buf64_{name}")
        if name.endswith("num_batches_tracked"):
            assert int(bufs[name]) == int(want) == 3 and bufs[name].dtype == torch.int64
        else:
            check_tensor(f"{key} {name}", bufs[name], want, fx.e_ref("buf"))
    rows = tuple(b.shape[0] for b in (dis._main[3].weight, dis._main[6].weight, dis._main[9].weight))
    assert rows == (2 * HIDDEN, 4 * HIDDEN, 8 * HIDDEN) and BN_ROWS[case][0] == image.shape[0] * (image.shape[2] // 4) * (
        image.shape[3] // 4)


@pytest.mark.parametrize("arm", ARMS, ids=[arm_tag(a) for a in ARMS])
def test_generator_pass_with_parameter_gradients_gives_the_same_logit_gradient(fx, arm):
    """`param_grads=False` (what the epocher's G step uses) changes nothing but the work that is skipped"""
    from cyhip.functions import SigmoidBCEFn
    image, _, unl = fx.inputs("b")
    img = image.to(DEV) if arm else None
    got = []
    for flag in (False, True):
        dis = _discriminator(fx, arm)
        z = gpu_leaf(unl)
        SigmoidBCEFn.apply(dis.scores_from_logits(img, z, param_grads=flag), 1.0).backward()
        got.append(z.grad.clone())
        assert all((p.grad is not None) == flag for p in dis.parameters())
    assert torch.equal(got[0], got[1])


@pytest.mark.parametrize("arm", ARMS, ids=[arm_tag(a) for a in ARMS])
def test_scores_from_logits_is_scores_of_the_concatenation(fx, arm):
    """Bit for bit against `scores` of a concatenation built from the same softmax arithmetic (the fused kernel without
    the image): the layout / concat check.  Bit equality with `scores(torch.cat([image, logits.softmax(1)], 1))` is not
    reachable: torch's softmax kernel evaluates another exp and another division, so its probabilities differ from the
    fused kernel's in the last bit.  Both forms are therefore held to the f64 CPU value of torch's own layers under the
    "out" bound max(4 * e_ref, 1e-6), each on its own."""
    from cyhip.functions import SoftmaxCatFn
    image, lab, _ = fx.inputs("b")
    img, z = image.to(DEV), lab.to(DEV)
    dis = _discriminator(fx, arm, train=False)
    p64 = lab.double().softmax(1)
    want = replica(fx.sd(arm), arm).eval()(torch.cat([image.double(), p64], 1) if arm else p64).detach()
    with torch.no_grad():
        fused = dis.scores_from_logits(img if arm else None, z)
        prob = SoftmaxCatFn.apply(None, z)
        assert torch.equal(fused, dis.scores(torch.cat([img, prob], 1) if arm else prob))
        torch_cat = torch.cat([img, z.softmax(1)], 1) if arm else z.softmax(1)
        plain = dis.scores(torch_cat)
        check_tensor(f"sigmoid(scores_from_logits) vs f64 ({arm_tag(arm)})", torch.sigmoid(fused), want,
                     fx.e_ref("out"))
        check_tensor(f"sigmoid(scores(torch softmax + cat)) vs f64 ({arm_tag(arm)})", torch.sigmoid(plain), want,
                     fx.e_ref("out"))
        assert torch.equal(dis(torch_cat), torch.sigmoid(plain))


@pytest.mark.parametrize("arm", ARMS, ids=[arm_tag(a) for a in ARMS])
@pytest.mark.parametrize("case", list(CASES))
def test_eval_mode_against_torch_in_f64(fx, case, arm):
    """running statistics of the fixture's step (not the initial 0 / 1) in both; torch's layers on the CPU in f64"""
    key = f"{case}_{arm_tag(arm)}"
    image, lab, _ = fx.inputs(case)
    sd = fx.sd(arm)
    for name in BUFFERS:
        sd[name] = fx.t(f"{key}_buf64_{name}")
    p = lab.double().softmax(1)
    want = replica(sd, arm).eval()(torch.cat([image.double(), p], 1) if arm else p).detach()
    from contrastyou.arch.discriminator import Discriminator
    dis = Discriminator(5 if arm else K, HIDDEN)
    dis.load_state_dict(sd, strict=True)
    dis.to(DEV).eval()
    before = {k: v.clone() for k, v in dis.named_buffers()}
    with torch.no_grad():
        x = torch.cat([image, lab.softmax(1)], 1) if arm else lab.softmax(1)
        got = dis(x.to(DEV))
    check_tensor(f"{key} eval output", got, want, fx.e_ref("out"))
    assert all(torch.equal(v, before[k]) for k, v in dis.named_buffers())


def test_cpu_tensors_are_refused(fx):
    dis = _discriminator(fx, True)
    image, lab, _ = fx.inputs("a")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dis.scores_from_logits(image, lab)


# ---------------------------------------------------------------------------------------------- 6. the epocher
class _Raises:
    """an unlabeled loader that must never be iterated"""
    dataset = Loader.dataset

    def __len__(self):
        return 1

    def __iter__(self):
        raise AssertionError("the unlabeled loader was iterated")


def _batch(image, gen, views=2):
    n, _, H, W = image.shape
    tgt = torch.randint(0, K, (n, 1, H, W), generator=gen)
    return {"img": [image] * views, "gt": [tgt] * views, "filename": [[f"f{i}" for i in range(n)]] * views,
            "partition": [[str(i % 3) for i in range(n)]] * views,
            "scan_num": [[f"patient{i // 2:03d}_{i % 2:02d}" for i in range(n)]] * views}


def _epocher(model, dis, lab_loader, unl_loader, reg_weight, arm, steps=1, lr=1e-3):
    from contrastyou.losses.kl import KL_div
    from contrastyou.optim import RAdam
    from semi_seg.epochers.comparable import AdversarialEpocher
    opt = RAdam([{"params": list(model.parameters())}], lr=lr, weight_decay=1e-4)
    dopt = RAdam([{"params": list(dis.parameters())}], lr=lr, weight_decay=1e-4)
    ep = AdversarialEpocher(model=model, optimizer=opt, labeled_loader=lab_loader, unlabeled_loader=unl_loader,
                            sup_criterion=KL_div(), num_batches=steps, cur_epoch=0, device=DEV, two_stage=False,
                            disable_bn=False, discriminator=dis, disc_optimizer=dopt, reg_weight=reg_weight,
                            dis_consider_image=arm, scaler=torch.amp.GradScaler("cuda", enabled=False))
    ep.init()
    return ep


@pytest.mark.parametrize("case,arm", [("a", True), ("b", False)])
def test_one_epocher_batch_against_the_fixture(fx, gen64, case, arm):
    from contrastyou.losses.kl import KL_div
    from semi_seg.epochers.epocher import _sup_loss
    key = f"{case}_{arm_tag(arm)}"
    image, lab, unl = fx.inputs(case)
    gen = torch.Generator().manual_seed(5)
    lab_batch, unl_batch = _batch(image, gen), _batch(image, gen)
    model = StoredLogits([lab.to(DEV), unl.to(DEV)]).to(DEV)
    dis = _discriminator(fx, arm)
    before = {k: v.detach().clone() for k, v in dis.named_parameters()}
    ep = _epocher(model, dis, Loader([lab_batch]), Loader([unl_batch]), 0.5, arm)
    ep.run()
    torch.cuda.synchronize()
    m = ep.get_metric()
    print(key, m["adv_reg"], m["semi"]["sup_loss"])
    assert model.calls == 2 and "reg_loss" not in m["semi"] and m["adv_reg"]["reg_weight"] == 0.5
    l64, g64 = gen64[(case, arm)]
    check_loss(f"{key} gen_loss meter", m["adv_reg"]["gen_loss"], l64, fx.e_ref("gen")[2])
    check_loss(f"{key} dis_loss meter", m["adv_reg"]["dis_loss"], fx[f"{key}_dis_loss64"], fx.e_ref("dis")[2])
    # the unlabeled logits take reg_weight * d generator_err, the labeled ones the supervised gradient alone
    check_tensor(f"{key} gradient on the unlabeled logits", model.logits[1].grad, 0.5 * g64, fx.e_ref("gen"))
    z = gpu_leaf(lab)
    sup = _sup_loss(KL_div(), z, lab_batch["gt"][0].to(DEV), K)
    sup.backward()
    assert torch.equal(model.logits[0].grad, z.grad)
    assert abs(m["semi"]["sup_loss"] - float(sup.detach())) <= 1e-6 * abs(float(sup.detach()))
    for name, p in dis.named_parameters():
        check_tensor(f"{key} {name}.grad", p.grad, 0.5 * fx.t(f"{key}_dis_g64_{name}").double(), fx.e_ref("dis"))
        assert not torch.equal(p.detach(), before[name]), f"{name} did not move"
    assert all(int(b) == 3 for n, b in dis.named_buffers() if n.endswith("num_batches_tracked"))


def test_zero_weight_never_touches_the_discriminator_or_the_unlabeled_loader(fx):
    image, lab, unl = fx.inputs("a")
    gen = torch.Generator().manual_seed(6)
    model = StoredLogits([lab.to(DEV)]).to(DEV)
    dis = _discriminator(fx, True)
    before = {k: v.detach().clone() for k, v in dis.state_dict().items()}
    ep = _epocher(model, dis, Loader([_batch(image, gen)]), _Raises(), 0.0, True)
    ep.run()
    torch.cuda.synchronize()
    m = ep.get_metric()
    assert m["adv_reg"] == {"dis_loss": 0.0, "gen_loss": 0.0, "reg_weight": 0.0}, m["adv_reg"]
    assert model.calls == 1 and model.logits[0].grad is not None and math.isfinite(m["semi"]["sup_loss"])
    after = dis.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert all(p.grad is None for p in dis.parameters())


# ---------------------------------------------------------------------------------------------- 7. a real network
def _real_run(sd0, lab, unl):
    from contrastyou.arch import UNet
    from contrastyou.arch.discriminator import Discriminator
    model = UNet(input_dim=1, num_classes=K, max_channel=128, momentum=0.1)
    model.load_state_dict(sd0)
    model.to(DEV)
    torch.manual_seed(3)
    dis = Discriminator(1 + K, 8).to(DEV)
    first = {"unet": {k: v.detach().clone().cpu() for k, v in model.state_dict().items()},
             "dis": {k: v.detach().clone().cpu() for k, v in dis.state_dict().items()}}
    ep = _epocher(model, dis, Loader(lab), Loader(unl), 0.1, True, steps=2, lr=3e-3)
    ep.run()
    torch.cuda.synchronize()
    last = {"unet": {k: v.detach().float().cpu() for k, v in model.state_dict().items()},
            "dis": {k: v.detach().float().cpu() for k, v in dis.state_dict().items()}}
    return first, last, ep.get_metric()


def test_two_batches_on_a_small_unet_are_finite_move_both_networks_and_repeat_bit_for_bit():
    from oracle import unet as ou
    sd0 = ou.init_state_dict(1, K, 128, seed=14)
    g = torch.Generator().manual_seed(21)
    lab, unl = [blob_batch(2, 64, K, g) for _ in range(2)], [blob_batch(2, 64, K, g) for _ in range(2)]
    first, last, m = _real_run(sd0, lab, unl)
    print(m["adv_reg"], m["semi"])
    def leaves(v):
        return [x for u in v.values() for x in leaves(u)] if isinstance(v, dict) else [v]

    values = leaves(m)  # every meter of every group: lr, sup_loss, sup_dice.*, gen_loss, dis_loss, reg_weight
    assert len(values) >= 4 + K and set(m) == {"semi", "adv_reg"} and set(m["semi"]) == {"lr", "sup_loss", "sup_dice"}
    assert all(math.isfinite(v) for v in values), m
    assert m["adv_reg"]["gen_loss"] > 0 and m["adv_reg"]["dis_loss"] > 0
    for net in ("unet", "dis"):
        assert all(torch.isfinite(v).all() for v in last[net].values())
        moved = [k for k, v in last[net].items() if k.endswith("weight") and not torch.equal(v, first[net][k].float())]
        assert len(moved) == sum(k.endswith("weight") for k in last[net]), (net, len(moved))
    assert int(last["dis"]["_main.3.num_batches_tracked"]) == 6
    _, again, m2 = _real_run(sd0, lab, unl)
    for net in ("unet", "dis"):
        for k in last[net]:
            assert torch.equal(last[net][k], again[net][k]), (net, k)
    assert m["adv_reg"] == m2["adv_reg"]
