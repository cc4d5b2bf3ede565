"""The cross-correlation family on the GPU (csrc/cy_cc.hip and the host classes on it) against tests/golden/cc.npz
(the reference's modules in f32 and f64, tests/golden/gen_goldens_cc.py) and against an f64 CPU evaluation written
here from the formulas.

Tolerance rule (one for the whole file).  The loss cancels (I2_sum - I_sum^2 / k^2) and clamps, so two correct f32
evaluations differ; the yardstick is the reference's own f32-to-f64 distance on the fixture's inputs:
    e(x) = |x - x64| relative: 2-norm for gradients, element-wise maximum over max|grad64|, |.| / |loss64| for the loss
    require e_hip <= max(4 * e_ref, 1e-6), e_ref = the largest value over the fixture's cases of the same kind
(a different summation order moves such an error by a small factor; the floor is f32 resolution), and independently
the project's own f32 bounds: loss within 1e-5 relative, gradients within 2e-4 of max|grad64|.
Clamp flips: a window whose cross / I_var / J_var lies within a factor 2 of eps in f64 may clamp differently in
f32; the pixels within k // 2 of such a window may be left out, at most 2 % of a case's pixels (asserted).
Every figure is printed before it is asserted.
"""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cc_fixture import decode, softmax_f32
from test_gpu_hooks_dice import Loader, blob_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
FLOOR, FACTOR = 1e-6, 4.0
LOSS_BOUND, GRAD_BOUND = 1e-5, 2e-4
FLIP_CAP = 0.02
# a map value is a chain of < 20 f32 roundings of quantities <= 1 plus sqrtf / logf / powf at <= 2 ulp each, compared
# with an f64 value stored rounded to f32: 64 ulp of 1.0
MAP_BOUND = 64 * 2.0 ** -24


@pytest.fixture(scope="module")
def fx(golden_dir):
    data = np.load(golden_dir / "cc.npz")

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

        softmax_f32 = staticmethod(softmax_f32)

    return Fx()


def bound(e_ref):
    return max(FACTOR * float(e_ref), FLOOR)


def cpu64(t):
    return t.detach().double().cpu()


# ---------------------------------------------------------------------------------------------- f64 formulas (CPU)
def box(x, k):
    return F.avg_pool2d(x, k, stride=1, padding=k // 2, count_include_pad=True) * (k * k)


def ccloss64(I, J, k, eps=EPS):
    """-> (loss, the three raw (unclamped) window terms)"""
    n = k * k
    sI, sJ = box(I, k), box(J, k)
    cross = box(I * J, k) - sI * sJ / n
    ivar = box(I * I, k) - sI * sI / n
    jvar = box(J * J, k) - sJ * sJ / n
    cc = cross.clamp_min(eps) ** 2 / (ivar.clamp_min(eps) * jvar.clamp_min(eps))
    return -cc.mean(), (cross.detach(), ivar.detach(), jvar.detach())


def minmax64(x, slicewise):
    dims = (1, 2, 3) if slicewise else (0, 1, 2, 3)
    lo, hi = x.detach().amin(dim=dims, keepdim=True), x.detach().amax(dim=dims, keepdim=True)
    return (x - lo) / (hi - lo + 1e-6)


def edge64(image, power, size=None):
    image = image.double()
    if size is not None and tuple(image.shape[-2:]) != tuple(size):
        image = F.interpolate(image, size=tuple(size), mode="bilinear")
    d = ((image - image.roll(1, 2)) ** 2 + (image - image.roll(1, 3)) ** 2).sqrt().mean(1, keepdim=True)
    return minmax64(d, True) ** power


def entropy64(prob, slicewise):
    return minmax64(-(prob * (prob + 1e-16).log()).sum(1, keepdim=True), slicewise)


def flip_mask(raw_terms, k, eps=EPS):
    """[n, 1, H, W] bool: pixels within k // 2 of a window with a raw term inside (eps / 2, 2 eps)"""
    near = torch.zeros_like(raw_terms[0], dtype=torch.bool)
    for t in raw_terms:
        near |= (t > eps / 2) & (t < 2 * eps)
    return F.max_pool2d(near.double(), k, stride=1, padding=k // 2) > 0


def check(what, loss, loss64, grads, e_ref, mask=None):
    """grads: [(name, got, grad64)], each [n, C, H, W]; mask: [n, 1, H, W] pixels left out"""
    loss = float(loss.detach())
    e_loss = abs(loss - float(loss64)) / abs(float(loss64))
    print(f"{what}: loss {loss:.9g} vs {float(loss64):.9g}  e_loss {e_loss:.2e} (bound {bound(e_ref[2]):.2e})")
    out = 0.0
    if mask is not None:
        out = mask.double().mean().item()
        print(f"{what}: pixels left out for clamp flips {100 * out:.3f} %")
    fails = []
    if e_loss > bound(e_ref[2]) or e_loss > LOSS_BOUND:
        fails.append(f"loss {e_loss:.2e}")
    for name, got, g64 in grads:
        got, g64 = cpu64(got), cpu64(g64)
        assert got.shape == g64.shape, (name, got.shape, g64.shape)
        d = got - g64
        if mask is not None:
            d = d * (~mask)
        if g64.abs().max() == 0:
            e2 = emax = float(d.abs().max())
        else:
            e2, emax = float(d.norm() / g64.norm()), float(d.abs().max() / g64.abs().max())
        print(f"{what}: {name} e_2 {e2:.2e} (bound {bound(e_ref[0]):.2e})  e_max {emax:.2e} "
              f"(bound {min(bound(e_ref[1]), GRAD_BOUND):.2e})")
        if e2 > bound(e_ref[0]) or emax > bound(e_ref[1]) or emax > GRAD_BOUND:
            fails.append(f"{name} e_2 {e2:.2e} e_max {emax:.2e}")
    assert out <= FLIP_CAP, f"{what}: {100 * out:.2f} % of the pixels near a clamp flip"
    assert not fails, f"{what}: {fails}"


def gpu_leaf(t):
    return t.float().to(DEV).requires_grad_(True)


# ---------------------------------------------------------------------------------------------- fixture cases
@pytest.mark.parametrize("win", [3, 5, 7, 9])
def test_ccloss_against_the_reference(fx, win):
    """case (a): CCLoss alone, both inputs requiring a gradient"""
    from contrastyou.losses.cross_correlation import CCLoss
    I, J = fx.dec("a_I_u16"), fx.dec("a_J_u16")
    i_, j_ = gpu_leaf(I), gpu_leaf(J)
    loss = CCLoss(win=(win, win)).to(DEV)(i_, j_)
    loss.backward()
    _, raw = ccloss64(I.double(), J.double(), win)
    check(f"a win {win}", loss, fx[f"a{win}_loss64"], [("dI", i_.grad, fx.t(f"a{win}_gI64")),
                                                     ("dJ", j_.grad, fx.t(f"a{win}_gJ64"))],
          fx.e_ref("a"), flip_mask(raw, win))


def _bc_case(fx, tag):
    power, win, size = fx["bc_cases"][["b0", "b1", "c0"].index(tag)]
    prob = fx.softmax_f32(fx.dec("bc_logits_i8d4"))
    image = fx.dec(f"bc_img{int(size)}_u8")
    return float(power), int(win), prob, image


@pytest.mark.parametrize("tag", ["b0", "b1", "c0"])
def test_cc_loss_per_head_against_the_reference(fx, tag):
    """cases (b) (ccblock.py: per-slice extrema) and (c) (cc.py: batch-wide extrema of the entropy map); the image at
    the map's size and at twice the size (resize path); image 0 has a flat band under a saturated prediction"""
    from contrastyou.losses.cross_correlation import CCLoss
    from semi_seg.hooks.cc import _CrossCorrelationLogitEpocherHook
    from semi_seg.hooks.ccblock import _CrossCorrelationHook
    power, win, prob, image = _bc_case(fx, tag)
    if tag.startswith("b"):
        head = _CrossCorrelationHook(weight=1.0, kernel_size=win, diff_power=power).cc_loss_per_head
    else:
        head = _CrossCorrelationLogitEpocherHook(cc_criterion=CCLoss(win=(win, win)), mi_criterion=None, cc_weight=1.0,
                                                 mi_weight=0.0, diff_power=power).cc_loss_per_head
    p_ = gpu_leaf(prob)
    loss, diff_image, diff_pred = head(image=image.to(DEV), predict_simplex=p_)
    loss.backward()
    assert diff_image.shape == diff_pred.shape == (prob.shape[0], 1, *prob.shape[-2:])
    assert not diff_image.requires_grad
    I64, J64 = entropy64(prob.double(), tag.startswith("b")), edge64(image, power, prob.shape[-2:])
    if tag == "b0":  # (the fixture keeps the maps of this case; the others are held to the f64 formulas below)
        for name, got, want in (("diff_image", diff_image, fx.t(f"{tag}_diff_image64")),
                                ("diff_tf_softmax", diff_pred, fx.t(f"{tag}_diff_pred64"))):
            err = (cpu64(got) - want.double()).abs().max().item()
            print(f"{tag}: {name} max abs err {err:.2e} (bound {MAP_BOUND:.2e})")
            assert err <= MAP_BOUND, (tag, name, err)
    else:
        assert (cpu64(diff_image) - J64).abs().max().item() <= MAP_BOUND
        assert (cpu64(diff_pred) - I64).abs().max().item() <= MAP_BOUND
    _, raw = ccloss64(I64, J64, win)
    check(f"{tag} power {power} win {win} image {image.shape[-1]}", loss, fx[f"{tag}_loss64"],
          [("dp", p_.grad, fx.t(f"{tag}_g64"))], fx.e_ref(tag[0]), flip_mask(raw, win))


def _close(a, b, rel, what):
    """the rule of tests/test_gpu_next_rows.py: max abs error against rel * max|b|"""
    a, b = cpu64(a), cpu64(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale, err = b.abs().max().item() + 1e-30, (a - b).abs().max().item()
    print(f"{what}: max err {err:.3e} (bound {rel * scale:.3e})")
    assert err <= rel * scale, f"{what}: max err {err:.3e} > {rel:.1e} * {scale:.3e}"


def nhwc(t):
    return t.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


@pytest.mark.parametrize("head_type", ["linear", "mlp"])
def test_projector_against_the_reference(fx, head_type):
    """case (d): weights loaded by state_dict name; probabilities to 1e-5, gradients to 1e-4 of the golden's maximum
    (the bounds the DenseClusterHead tests use)"""
    from contrastyou.projectors import CrossCorrelationProjector
    head = CrossCorrelationProjector(input_dim=16, num_clusters=6, head_type=head_type, normalize=False,
                                     num_subheads=2, hidden_dim=24)
    names = list(fx[f"d_{head_type}_names"])
    assert sorted(head.state_dict()) == names
    head.load_state_dict({k: fx.t(f"d_{head_type}_w_{k}") for k in names}, strict=True)
    head = head.to(DEV)
    x = nhwc(fx.dec("d_feat_i8d32")).requires_grad_(True)
    probs = head(x)
    assert len(probs) == 2
    sum((p * fx.t(f"d_{head_type}_coef{i}").to(DEV)).sum() for i, p in enumerate(probs)).backward()
    for i, p in enumerate(probs):
        _close(p, fx.t(f"d_{head_type}_prob{i}"), 1e-5, f"{head_type} prob{i}")
    _close(x.grad, fx.t(f"d_{head_type}_dx"), 1e-4, f"{head_type} dx")
    for k, p in head.named_parameters():
        _close(p.grad, fx.t(f"d_{head_type}_g_{k}"), 1e-4, f"{head_type} d{k}")


class _Tap:
    def __init__(self, feats):
        self.feats = feats

    def bind(self):
        pass

    def tail(self, rows):
        return self.feats[-rows:]


class _Epocher:
    cur_epoch, cur_batch_num = 1, 1


def _composed_hook(fx, feats):
    from contrastyou.projectors import CrossCorrelationProjector
    from semi_seg.hooks.ccblock import (_CrossCorrelationHook, _MIHook, _ProjectorEpocherGeneralHook,
                                        _RedundancyReduction)
    ccw, k, power, miw, lamda, pad, rrw, alpha = fx["e_params"]
    proj = CrossCorrelationProjector(input_dim=16, num_clusters=6, head_type="linear", normalize=False, num_subheads=2)
    proj.load_state_dict({n: fx.t(f"e_w_{n}") for n in proj.state_dict()}, strict=True)
    proj = proj.to(DEV)
    tiny = [_MIHook(weight=float(miw), lamda=float(lamda), padding=int(pad)),
            _CrossCorrelationHook(weight=float(ccw), kernel_size=int(k), diff_power=float(power)),
            _RedundancyReduction(weight=float(rrw), alpha=float(alpha))]
    hook = _ProjectorEpocherGeneralHook(name="e", extractor=_Tap(feats), projector=proj, dist_hooks=tiny)
    for h in tiny:
        h.hook = hook
    hook._epocher, hook._epocher_init = _Epocher(), True
    return hook, proj


def test_composed_epocher_hook_against_the_reference(fx):
    """case (e): cc + mi + rr on hand-made features through an identity affine_transformer"""
    feats = nhwc(fx.dec("e_feat_i8d32")).requires_grad_(True)
    img = fx.dec("e_img_u8").to(DEV)
    hook, proj = _composed_hook(fx, feats)
    loss = hook._call_implementation(unlabeled_image_tf=img, unlabeled_logits_tf=torch.zeros(2, 1),
                                     affine_transformer=lambda t: t, unlabeled_image=img, seed=1)
    loss.backward()
    grads = [("dfeat", feats.grad, fx.t("e_gfeat64"))]
    grads += [(f"d{n}", p.grad, fx.t(f"e_g64_{n}")) for n, p in proj.named_parameters()]
    check("e cc+mi+rr", loss, fx["e_loss64"], grads, fx.e_ref("e"))


# ---------------------------------------------------------------------------------------------- own f64 evaluation
def _fields(gen, n, K, H, W, smooth=7):
    pad = smooth - 1
    logits = F.avg_pool2d(torch.rand(n, K, H + pad, W + pad, generator=gen), smooth, stride=1).sub(0.5).mul(40)
    logits = logits + torch.randn(n, K, H, W, generator=gen)
    image = F.avg_pool2d(torch.rand(n, 1, H + 4, W + 4, generator=gen), 5, stride=1)
    return logits.double().softmax(1).float(), image


def _chain_gpu(prob, image, power, win, slicewise=True):
    from contrastyou.losses.cross_correlation import CCLoss
    from semi_seg.hooks.ccblock import EdgeMapCache, cc_loss_per_head
    p_ = gpu_leaf(prob)
    loss, di, dp = cc_loss_per_head(CCLoss(win=(win, win)), image.to(DEV), p_, power, slicewise, EdgeMapCache())
    loss.backward()
    return loss.detach(), p_.grad, di, dp


def _chain_cpu64(prob, image, power, win, slicewise=True):
    p = prob.double().requires_grad_(True)
    I, J = entropy64(p, slicewise), edge64(image, power, prob.shape[-2:])
    loss, raw = ccloss64(I, J, win)
    loss.backward()
    return loss.detach(), p.grad, I.detach(), J, raw


@pytest.mark.parametrize("win", [3, 7])
def test_production_size_against_f64_formulas(fx, win):
    """16 x 224 x 224, K = 10: the whole chain (edge map, entropy map, CCLoss) and CCLoss alone with both gradients"""
    from contrastyou.losses.cross_correlation import CCLoss
    gen = torch.Generator().manual_seed(500 + win)
    prob, image = _fields(gen, 16, 10, 224, 224)
    loss, dp, di, dpred = _chain_gpu(prob, image, 0.75, win)
    loss64, dp64, I64, J64, raw = _chain_cpu64(prob, image, 0.75, win)
    for name, got, want in (("diff_image", di, J64), ("diff_tf_softmax", dpred, I64)):
        err = (cpu64(got) - want).abs().max().item()
        print(f"224 win {win}: {name} max abs err {err:.2e} (bound {MAP_BOUND:.2e})")
        assert err <= MAP_BOUND, (name, err)
    check(f"224 chain win {win}", loss, loss64, [("dp", dp, dp64)], fx.e_ref("b"), flip_mask(raw, win))
    # CCLoss alone on the f32 maps the chain produced, both inputs requiring a gradient
    I, J = dpred.detach().clone().requires_grad_(True), di.detach().clone().requires_grad_(True)
    la = CCLoss(win=(win, win))(I, J)
    la.backward()
    i64, j64 = cpu64(I).requires_grad_(True), cpu64(J).requires_grad_(True)
    la64, raw = ccloss64(i64, j64, win)
    la64.backward()
    check(f"224 CCLoss win {win}", la, la64, [("dI", I.grad, i64.grad), ("dJ", J.grad, j64.grad)], fx.e_ref("a"),
          flip_mask(raw, win))


@pytest.mark.parametrize("n,K,H,W,win,power", [
    (2, 5, 5, 40, 7, 0.75),    # H smaller than the window
    (2, 4, 33, 3, 5, 0.75),    # W smaller than the window (and K % 4 == 0: 16-byte rows)
    (1, 3, 3, 3, 15, 0.75),    # the whole map inside one window; 16 x 16 tile of the widest windows
    (3, 6, 45, 70, 9, 0.75),   # not multiples of the tile
    (2, 7, 50, 37, 13, 1.0),   # 16 x 16 tile, diff_power 1
    (2, 5, 40, 44, 3, 0.0),    # diff_power 0: the edge map is all ones
    (2, 8, 64, 96, 11, 0.5),   # the largest window on the 32 x 32 tile
])
def test_odd_shapes_and_powers(fx, n, K, H, W, win, power):
    gen = torch.Generator().manual_seed(H * 1000 + W)
    prob, image = _fields(gen, n, K, H, W, smooth=3)
    for slicewise in (True, False):
        loss, dp, di, dpred = _chain_gpu(prob, image, power, win, slicewise)
        loss64, dp64, I64, J64, raw = _chain_cpu64(prob, image, power, win, slicewise)
        assert (cpu64(di) - J64).abs().max().item() <= MAP_BOUND
        assert (cpu64(dpred) - I64).abs().max().item() <= MAP_BOUND
        check(f"{n}x{K}x{H}x{W} win {win} power {power} slicewise {slicewise}", loss, loss64, [("dp", dp, dp64)],
              fx.e_ref("b" if slicewise else "c"), flip_mask(raw, win))


def test_constant_slices_and_multi_channel_images(fx):
    """a slice whose entropy map is constant (max = min) and one whose image is constant; a 3-channel image"""
    gen = torch.Generator().manual_seed(77)
    prob, image = _fields(gen, 3, 5, 40, 48, smooth=3)
    prob[1] = 0.2           # uniform prediction: constant entropy
    image[2] = 0.5          # flat image: no edges
    image = image.repeat(1, 3, 1, 1) * torch.tensor([1.0, 0.5, 0.25]).view(1, 3, 1, 1)
    loss, dp, di, dpred = _chain_gpu(prob, image, 0.75, 5)
    loss64, dp64, I64, J64, raw = _chain_cpu64(prob, image, 0.75, 5)
    assert torch.isfinite(dp).all() and torch.isfinite(loss)
    assert (cpu64(di) - J64).abs().max().item() <= MAP_BOUND
    assert dpred[1].abs().max().item() == 0 and di[2].abs().max().item() == 0
    check("constant slices", loss, loss64, [("dp", dp, dp64)], fx.e_ref("b"), flip_mask(raw, 5))


def test_two_runs_give_the_same_bits():
    from contrastyou.losses.cross_correlation import CCLoss
    gen = torch.Generator().manual_seed(5)
    prob, image = _fields(gen, 4, 10, 100, 90)
    runs = []
    for _ in range(2):
        loss, dp, di, dpred = _chain_gpu(prob, image, 0.75, 7)
        I, J = dpred.detach().clone().requires_grad_(True), di.detach().clone().requires_grad_(True)
        la = CCLoss(win=(7, 7))(I, J)
        la.backward()
        torch.cuda.synchronize()
        runs.append([t.detach().cpu() for t in (loss, dp, di, dpred, la, I.grad, J.grad)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- launch counts
# kernel launches behind each entry point, as include/contrastyou_hip.h and DESIGN.md ("Cross-correlation hooks")
# state them: NOT observed here -- what the tests below observe are the entry-point calls; a kernel added inside an
# entry point would have to be caught by reading its host function (csrc/cy_cc.hip, one or two launches each)
LAUNCHES = {"cy_cc_edge_map": 2, "cy_entropy_map_fwd": 2, "cy_entropy_map_bwd": 1, "cy_ccloss_fwd": 2,
            "cy_ccloss_bwd": 1, "cy_bilinear_fwd": 1}


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


def test_launch_count_of_one_cross_correlation_hook_call(monkeypatch):
    """DESIGN.md section 3, "Cross-correlation hooks": one _CrossCorrelationHook call = the edge map once (2 launches, + 1 when the image is
    resized) and, per head, 4 launches forward and 2 backward"""
    from semi_seg.hooks.ccblock import _CrossCorrelationHook
    gen = torch.Generator().manual_seed(6)
    prob, image = _fields(gen, 2, 10, 56, 56)
    image2 = F.avg_pool2d(torch.rand(2, 1, 116, 116, generator=gen), 5, stride=1)
    for img, resize in ((image, 0), (image2, 1)):
        tiny = _CrossCorrelationHook(weight=1.0, kernel_size=5)
        p1, p2 = gpu_leaf(prob), gpu_leaf(prob.roll(1, 1))
        img = img.to(DEV)
        count = _Count(monkeypatch)
        loss = tiny(image=img, input1=p1, input2=p2, saver=None, save_image_condition=False, cur_epoch=0,
                    cur_batch_num=0)
        fwd = count.take()
        loss.backward()
        bwd = count.take()
        monkeypatch.undo()
        want_fwd = {"cy_cc_edge_map": 1, "cy_entropy_map_fwd": 2, "cy_ccloss_fwd": 2}
        if resize:
            want_fwd["cy_bilinear_fwd"] = 1
        assert fwd == want_fwd, fwd
        assert bwd == {"cy_ccloss_bwd": 2, "cy_entropy_map_bwd": 2}, bwd
        assert sum(LAUNCHES[k] * v for k, v in fwd.items()) == 2 + resize + 2 * 4
        assert sum(LAUNCHES[k] * v for k, v in bwd.items()) == 2 * 2
        assert tiny.diff_image[0] is tiny.diff_image[1]  # one edge map for both heads


def test_launch_count_of_one_projector_epocher_hook_call(fx, monkeypatch):
    """the composed hook (cc + mi + rr, 2 sub-heads): the edge map still once; 4 heads x (4 forward + 2 backward)"""
    feats = nhwc(fx.dec("e_feat_i8d32")).requires_grad_(True)
    img = fx.dec("e_img_u8").to(DEV)
    hook, _ = _composed_hook(fx, feats)
    count = _Count(monkeypatch)
    loss = hook._call_implementation(unlabeled_image_tf=img, unlabeled_logits_tf=torch.zeros(2, 1),
                                     affine_transformer=lambda t: t, unlabeled_image=img, seed=1)
    fwd = count.take()
    loss.backward()
    bwd = count.take()
    monkeypatch.undo()
    print("composed hook, entry points forward:", fwd, "backward:", bwd)
    cc_fwd = {k: v for k, v in fwd.items() if k in LAUNCHES}
    cc_bwd = {k: v for k, v in bwd.items() if k in LAUNCHES}
    assert cc_fwd == {"cy_bilinear_fwd": 1, "cy_cc_edge_map": 1, "cy_entropy_map_fwd": 4, "cy_ccloss_fwd": 4}, cc_fwd
    assert cc_bwd == {"cy_ccloss_bwd": 4, "cy_entropy_map_bwd": 4}, cc_bwd
    assert sum(LAUNCHES[k] * v for k, v in cc_fwd.items()) == 3 + 4 * 4
    assert sum(LAUNCHES[k] * v for k, v in cc_bwd.items()) == 4 * 2


# ---------------------------------------------------------------------------------------------- semi-supervised steps
HOOK_PARAMS = {"cc": dict(weight=1.0, kernel_size=5, diff_power=0.75),
               "mi": dict(weight=0.1, lamda=1.0, padding=0),
               "rr": dict(weight=0.1, alpha=0.5)}


def _semi_run(feature_name, lab, unl, sd0, *, with_hook=True, graph=None, bf16=False, steps=1, K=4, max_channel=256):
    from contrastyou.amp import BF16Scaler
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.losses.kl import KL_div
    from contrastyou.optim import RAdam
    from cyhip import graphed
    from semi_seg.epochers import SemiSupervisedEpocher
    from semi_seg.hooks import create_cross_correlation_hooks2
    default = graphed.GRAPH_STEP
    if graph is not None:
        graphed.GRAPH_STEP = graph
    try:
        type(TrainerHook).names.clear()
        model = UNet(input_dim=1, num_classes=K, max_channel=max_channel, momentum=0.1)
        model.load_state_dict(sd0)
        model.to(DEV)
        torch.manual_seed(3)
        hook = create_cross_correlation_hooks2(model=model, feature_name=feature_name, num_clusters=8,
                                               head_type="linear", num_subheads=2, hook_params=HOOK_PARAMS).to(DEV)
        groups = [{"params": list(model.parameters())}]
        if list(hook.parameters()):
            groups.append({"params": list(hook.parameters())})
        opt = RAdam(groups, lr=3e-3, weight_decay=1e-4)
        scaler = BF16Scaler() if bf16 else torch.amp.GradScaler("cuda", enabled=False)
        ep = SemiSupervisedEpocher(model=model, optimizer=opt, labeled_loader=Loader(lab), unlabeled_loader=Loader(unl),
                                   sup_criterion=KL_div(), num_batches=steps, cur_epoch=0, device=DEV, two_stage=True,
                                   disable_bn=False, scaler=scaler, accumulate_iter=1)
        ep.init()
        random.seed(9)
        before = {k: v.detach().clone() for k, v in hook.state_dict()["module_state"].items()}
        if with_hook:
            with ep.register_hook(hook()):
                ep.run()
        else:
            ep.run()
        torch.cuda.synchronize()
        replayed = any(isinstance(v, graphed.GraphedTwoPass) for v in model.__dict__.get("_cy_graphed", {}).values())
        after = {k: v.detach().clone() for k, v in hook.state_dict()["module_state"].items()}
        return ({k: v.detach().float().cpu() for k, v in model.state_dict().items()}, ep.get_metric(), replayed,
                before, after)
    finally:
        graphed.GRAPH_STEP = default


def _batches(steps, n=4, hw=32, K=4, seed=21):
    g = torch.Generator().manual_seed(seed)
    return [blob_batch(n, hw, K, g) for _ in range(steps)], [blob_batch(n, hw, K, g) for _ in range(steps)]


@pytest.mark.parametrize("feature_name", ["Up_conv2", "Deconv_1x1"])
def test_hooks_in_a_semi_supervised_step(feature_name):
    """one f32 step with and without the hook from the same state: finite losses, filled meters, and the hook's
    gradient reaches every projector parameter and every network parameter upstream of the tap -- those move
    differently than without the hook -- while what lies behind the tap moves exactly as without it"""
    from oracle import unet as ou
    sd0 = ou.init_state_dict(1, 4, 256, seed=14)  # Up_conv2 has 16 channels at max_channel=256
    lab, unl = _batches(1)
    sd_h, m_h, _, before, after = _semi_run(feature_name, lab, unl, sd0, graph=False)
    sd_0, m_0, _, _, _ = _semi_run(feature_name, lab, unl, sd0, with_hook=False, graph=False)
    group = m_h[f"cc_{feature_name}"]
    names = ("cc", "mi", "rr") if feature_name == "Up_conv2" else ("cc_ls", "mi_ls")
    print(feature_name, {k: group[k] for k in names}, "reg_loss", m_h["semi"]["reg_loss"])
    for k in names:
        assert np.isfinite(group[k]) and group[k] != 0, (k, group[k])
    assert np.isfinite(m_h["semi"]["reg_loss"]) and m_h["semi"]["reg_loss"] != 0
    assert m_0["semi"]["reg_loss"] == 0
    if feature_name == "Up_conv2":
        assert before and all(not torch.equal(before[k], after[k]) for k in before), "a projector parameter stood still"
    params = [k for k in sd_h if k.endswith((".weight", ".bias"))]
    behind_tap = [k for k in params if "Deconv_1x1" in k] if feature_name == "Up_conv2" else []
    assert feature_name != "Up_conv2" or behind_tap
    for k in params:
        if k in behind_tap:
            assert torch.equal(sd_h[k], sd_0[k]), f"{k} lies behind the tap and must not see the hook"
        else:
            assert not torch.equal(sd_h[k], sd_0[k]), f"{k} received no gradient from the hook"
        assert torch.isfinite(sd_h[k]).all()


@pytest.mark.parametrize("feature_name", ["Up_conv2", "Deconv_1x1"])
def test_graph_replayed_steps_equal_eager_steps(feature_name):
    """the pattern of test_hip_graph_replay_of_the_two_passes_equals_eager_steps: the hooks run in the eager section
    between the two graph replays; four steps either way end in the same bits"""
    from oracle import unet as ou
    sd0 = ou.init_state_dict(1, 4, 256, seed=14)  # Up_conv2 has 16 channels at max_channel=256
    lab, unl = _batches(4)
    sd_e, m_e, rep_e, _, hook_e = _semi_run(feature_name, lab, unl, sd0, graph=False, bf16=True, steps=4)
    sd_g, m_g, rep_g, _, hook_g = _semi_run(feature_name, lab, unl, sd0, graph=True, bf16=True, steps=4)
    assert rep_g and not rep_e, "the second run must have captured and replayed the passes"
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k
    for k in hook_e:
        assert torch.equal(hook_e[k], hook_g[k]), k
    assert m_e["semi"]["reg_loss"] == m_g["semi"]["reg_loss"] and np.isfinite(m_e["semi"]["reg_loss"])
    assert m_e[f"cc_{feature_name}"] == m_g[f"cc_{feature_name}"]
