"""The IMSAT kernels (csrc/cy_imsat.hip), their autograd functions, losses and hooks on the GPU, against
tests/golden/imsat.npz (the reference in f32 and f64, tests/golden/gen_goldens_imsat.py) and against float64 torch on
the CPU (tests/imsat_cases.py, the formulas of include/contrastyou_hip.h).

Tolerance: max(4 * the reference's own largest f32-to-f64 distance of that kind over the fixture, 1e-6), read from the
npz; how each kind is measured is in tests/imsat_fixture.py.  No element is left out of any comparison, and every
figure is printed before it is asserted.  Outputs of the `ops` level are written into slices of buffers filled with a
guard value, which must be intact afterwards.
"""
import math

import numpy as np
import pytest
import torch

import imsat_cases as ic
import imsat_fixture as fx
from test_gpu_hooks_dice import Loader, blob_batch
from test_gpu_semi_baselines import _Epocher, identity

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, PAD = 777.25, 8


@pytest.fixture(scope="module")
def npz(golden_dir):
    return fx.load(golden_dir)


@pytest.fixture(scope="module")
def tol(npz):
    t = fx.tolerances(npz)
    print("tolerances", t)
    return t


class Guarded:
    """a float buffer filled with the guard value; `take(n, offset)` gives a view of n floats that starts PAD + offset
    floats in; `intact()` checks everything outside the views handed out"""

    def __init__(self, total):
        self.buf = torch.full((total,), GUARD, device=DEV)
        self.mask = torch.ones(total, dtype=torch.bool, device=DEV)
        self.at = 0

    def take(self, n, offset=0):
        start = self.at + PAD + offset
        self.at = (start + n + PAD + 3) // 4 * 4  # the next view starts 16-byte aligned again
        assert self.at <= self.buf.numel()
        self.mask[start:start + n] = False
        return self.buf[start:start + n]

    def intact(self):
        return bool((self.buf[self.mask] == GUARD).all())


def gpu_leaf(t):
    return t.detach().to(DEV).clone().requires_grad_(True)


def up(g):
    return torch.tensor(g, dtype=torch.float32, device=DEV)


def rows_fwd_bwd(p_dev, upstreams, offset=0):
    """ops.imsat_fwd / _bwd on rows [R, K] with every output in a guarded slice -> (out, coef, mean, [dp per g])"""
    from cyhip import ops
    R, K = p_dev.shape
    mem = Guarded(2 + 2 * K + len(upstreams) * R * K + 32 * (3 + len(upstreams)))
    out, coef, mean = ops.imsat_fwd(p_dev, mem.take(2, offset), mem.take(K, offset), mem.take(K, offset))
    grads = [ops.imsat_bwd(p_dev, coef, up(g), mem.take(R * K, offset).view(R, K)) for g in upstreams]
    torch.cuda.synchronize()
    assert mem.intact(), "a guard value next to an output was overwritten"
    return out.cpu(), coef.cpu(), mean.cpu(), [g.cpu() for g in grads]


def coef64(p_cpu):
    rows = p_cpu.double().movedim(1, -1).reshape(-1, p_cpu.shape[1])
    m = rows.mean(0)
    return m, -(torch.log(m + fx.EPS) + m / (m + fx.EPS)) / rows.shape[0]


# ---------------------------------------------------------------------------------------------- 1. the fixture, ops
@pytest.mark.parametrize("tag", fx.all_cases())
def test_fixture_rows_through_ops(npz, tol, tag):
    from cyhip import functions
    p = fx.case_probs(npz, tag)
    rows = functions._imsat_rows(p.to(DEV))
    upstreams = ic.UPSTREAMS + ((-fx.LAMDA, 1.0),)
    out, coef, mean, grads = rows_fwd_bwd(rows, upstreams)
    ic.check_entropies(out, (npz[f"{tag}_marg64"], npz[f"{tag}_cond64"]), tol, f"{tag} vs npz")
    m64, c64 = coef64(p)
    ic.check_grad(mean, m64, tol, f"{tag} means")
    ic.check_grad(coef, c64, tol, f"{tag} coefficients")
    for g, got in zip(upstreams, grads):
        marg, cond, want = ic.ref_rows(p, g)
        ic.check_entropies(out, (marg, cond), tol, f"{tag} vs f64")
        ic.check_grad(functions._imsat_grad(got, (p.shape, p.dtype)), want, tol, f"{tag} upstream {g}")
    ic.check_grad(functions._imsat_grad(grads[-1], (p.shape, p.dtype)), torch.from_numpy(npz[f"{tag}_g64"]), tol,
                  f"{tag} gradient vs npz")
    if tag == fx.ONEHOT[0]:
        # p = 0 adds exactly 0 (so cond is exactly 0 for one-hot rows) and its gradient entry is -log(eps) / R
        assert float(out[1]) == 0.0
        zero = (p == 0)
        got = grads[2][zero] * p.shape[0] / 3.0
        assert float((got + math.log(1e-8)).abs().max()) <= 2e-6 * abs(math.log(1e-8))


# ---------------------------------------------------------------------------------------------- 2. functions, losses
@pytest.mark.parametrize("tag", fx.all_cases())
def test_fixture_rows_through_functions_and_losses(npz, tol, tag):
    from contrastyou.losses.discreteMI import IMSATLoss, imsat_loss, imsat_with_entropy
    from cyhip.functions import IMSATFn
    p = fx.case_probs(npz, tag)
    for g in ic.UPSTREAMS:
        x = gpu_leaf(p)
        marg, cond = IMSATFn.apply(x)
        (g[0] * marg + g[1] * cond).backward()
        m64, c64, want = ic.ref_rows(p, g)
        ic.check_entropies((marg, cond), (m64, c64), tol, f"IMSATFn {tag}")
        assert x.grad.shape == p.shape
        ic.check_grad(x.grad, want, tol, f"IMSATFn {tag} upstream {g}")
    scale = abs(float(npz[f"{tag}_cond64"])) + fx.LAMDA * abs(float(npz[f"{tag}_marg64"]))
    calls = [lambda t: imsat_loss(t, lamda=fx.LAMDA)] + ([IMSATLoss(lamda=fx.LAMDA)] if p.dim() == 2 else [])
    for fn in calls:
        x = gpu_leaf(p)
        loss = fn(x)
        loss.backward()
        ic.check_value(loss, npz[f"{tag}_loss64"], scale, tol, f"imsat_loss {tag}")
        ic.check_grad(x.grad, torch.from_numpy(npz[f"{tag}_g64"]), tol, f"imsat_loss {tag}")
    marg, cond = imsat_with_entropy(p.to(DEV))
    ic.check_entropies((marg, cond), (npz[f"{tag}_marg64"], npz[f"{tag}_cond64"]), tol, f"imsat_with_entropy {tag}")


# ---------------------------------------------------------------------------------------------- 3. two views
def pair_fwd_bwd(a, b, upstreams, offset=0):
    from cyhip import ops
    R, K = a.shape
    mem = Guarded(5 + 4 * K + 2 * len(upstreams) * R * K + 32 * (3 + 2 * len(upstreams)))
    out, coef, mean = ops.imsat_pair_fwd(a, b, mem.take(5, offset), mem.take(2 * K, offset), mem.take(2 * K, offset))
    grads = [ops.imsat_pair_bwd(a, b, coef, up(g), mem.take(R * K, offset).view(R, K),
                                mem.take(R * K, offset).view(R, K)) for g in upstreams]
    torch.cuda.synchronize()
    assert mem.intact(), "a guard value next to an output was overwritten"
    return out.cpu(), coef.cpu(), mean.cpu(), [(x.cpu(), y.cpu()) for x, y in grads]


def check_pair(a_cpu, b_cpu, out, grads, upstreams, tol, what):
    for g, (d1, d2) in zip(upstreams, grads):
        want, w1, w2 = ic.ref_pair(a_cpu, b_cpu, g)
        ic.check_entropies(out[:4], want[:4], tol, f"{what} entropies")
        e = abs(float(out[4]) - float(want[4])) / float(want[4]) if float(want[4]) else abs(float(out[4]))
        print(f"{what}: mse {e:.2e}")
        assert e <= tol["scalar"]
        ic.check_grad(d1, w1, tol, f"{what} dx1 upstream {g}")
        ic.check_grad(d2, w2, tol, f"{what} dx2 upstream {g}")


@pytest.mark.parametrize("tag", fx.PAIR_CASES)
def test_fixture_pairs(npz, tol, tag):
    from contrastyou.losses.discreteMI import IMSATLoss
    from cyhip.functions import IMSATPairFn
    p1, p2 = fx.probs(fx.decode(npz[f"{tag}_z_i8d8"])), fx.probs(fx.decode(npz[f"{tag}_z2_i8d8"]))
    out, coef, mean, grads = pair_fwd_bwd(p1.to(DEV), p2.to(DEV), ic.PAIR_UPSTREAMS)
    check_pair(p1, p2, out, grads, ic.PAIR_UPSTREAMS, tol, f"pair {tag}")
    for p, c, m in ((p1, coef[0], mean[0]), (p2, coef[1], mean[1])):
        m64, c64 = coef64(p)
        ic.check_grad(m, m64, tol, f"pair {tag} means")
        ic.check_grad(c, c64, tol, f"pair {tag} coefficients")
    for g in ic.PAIR_UPSTREAMS:
        a, b = gpu_leaf(p1), gpu_leaf(p2)
        outs = IMSATPairFn.apply(a, b)
        sum(w * o for w, o in zip(g, outs)).backward()
        want, w1, w2 = ic.ref_pair(p1, p2, g)
        ic.check_entropies(outs[:4], want[:4], tol, f"IMSATPairFn {tag}")
        ic.check_grad(a.grad, w1, tol, f"IMSATPairFn {tag} dx1")
        ic.check_grad(b.grad, w2, tol, f"IMSATPairFn {tag} dx2")
    a, b = gpu_leaf(p1), gpu_leaf(p2)
    crit = IMSATLoss(lamda=fx.LAMDA)
    loss = crit(a, b)
    loss.backward()
    want, _, _ = ic.ref_pair(p1, p2, ic.PAIR_UPSTREAMS[0])
    scale = 0.5 * float(want[1] + want[3] + fx.LAMDA * (want[0] + want[2]))
    ic.check_value(loss, npz[f"{tag}_pair_loss64"], scale, tol, f"IMSATLoss pair {tag}")
    ic.check_grad(a.grad, torch.from_numpy(npz[f"{tag}_pair_g1_64"]), tol, f"IMSATLoss pair {tag} dx1")
    ic.check_grad(b.grad, torch.from_numpy(npz[f"{tag}_pair_g2_64"]), tol, f"IMSATLoss pair {tag} dx2")
    joint = crit.get_joint_matrix()
    assert isinstance(joint, np.ndarray) and joint.shape == (p1.shape[1],) * 2
    ic.check_grad(torch.from_numpy(joint), torch.from_numpy(npz[f"{tag}_pair_joint64"]), tol, f"joint {tag}")


# ---------------------------------------------------------------------------------------------- 4. alignment
@pytest.mark.parametrize("K,R", ic.ALIGN_SHAPES)
@pytest.mark.parametrize("offset", sorted(ic.OFFSET_ALIGN))
def test_inputs_and_outputs_at_every_alignment(tol, K, R, offset):
    p = ic.seeded_rows(K, R, seed=K + R)
    q = ic.seeded_rows(K, R, seed=K + R + 1)
    big = torch.zeros(2 * (R * K + 8), device=DEV)
    a = big[offset:offset + R * K].view(R, K).copy_(p)
    start = (offset + R * K + 3) // 4 * 4 + 4
    b = big[start:start + R * K].view(R, K).copy_(q)  # 16-byte aligned: the pair runs at the smaller alignment
    assert a.data_ptr() % 16 == (4 * offset) % 16 and b.data_ptr() % 16 == 0
    out, _, _, grads = rows_fwd_bwd(a, ic.UPSTREAMS[:1], offset)
    marg, cond, want = ic.ref_rows(p, ic.UPSTREAMS[0])
    ic.check_entropies(out, (marg, cond), tol, f"rows K {K} R {R} offset {offset}")
    ic.check_grad(grads[0], want, tol, f"rows K {K} R {R} offset {offset}")
    out, _, _, grads = pair_fwd_bwd(a, b, ic.PAIR_UPSTREAMS[1:], offset)
    check_pair(p, q, out, grads, ic.PAIR_UPSTREAMS[1:], tol, f"pair K {K} R {R} offset {offset}")


@pytest.mark.parametrize("K,R", ic.HALVES)
def test_the_two_halves_of_one_tensor(tol, K, R):
    from cyhip.functions import IMSATPairFn
    both = ic.seeded_rows(K, 2 * R, seed=K * R)
    x = gpu_leaf(both)
    a, b = torch.chunk(x, 2, dim=0)
    assert (b.data_ptr() - a.data_ptr()) == 4 * R * K and (R * K) % 2 == 1
    g = ic.PAIR_UPSTREAMS[0]
    outs = IMSATPairFn.apply(a, b)
    sum(w * o for w, o in zip(g, outs)).backward()
    want, w1, w2 = ic.ref_pair(both[:R], both[R:], g)
    ic.check_entropies(outs[:4], want[:4], tol, f"halves K {K} R {R}")
    ic.check_grad(x.grad, torch.cat([w1, w2]), tol, f"halves K {K} R {R}")
    out, _, _, grads = pair_fwd_bwd(a.detach(), b.detach(), (g,))
    check_pair(both[:R], both[R:], out, grads, (g,), tol, f"halves (ops) K {K} R {R}")


# ---------------------------------------------------------------------------------------------- 5. past the grid caps
def _cap_ids():
    from cyhip import ops
    return ic.cap_cases(ops.imsat_plan)


@pytest.mark.parametrize("form,K,R,align", _cap_ids())
def test_past_the_grid_caps(tol, form, K, R, align):
    from cyhip import ops
    off = {16: 0, 8: 2, 4: 1}[align]
    p = ic.seeded_rows(K, R, seed=K)
    if form == "logits":
        z = ic.seeded_logits((R, K), seed=K + 1)
        big = torch.zeros(R * K + 4, device=DEV)
        zd = big[off:off + R * K].copy_(z.flatten()).view(1, 1, R, K).permute(0, 3, 1, 2)
        out, coef, _ = ops.softmax_imsat_fwd(zd)
        d = ops.softmax_imsat_bwd(zd, coef, up(ic.UPSTREAMS[0]))
        marg, cond, want = ic.ref_logits(z, ic.UPSTREAMS[0])
        ic.check_entropies(out.cpu(), (marg, cond), tol, f"logits K {K} npix {R} align {align}")
        ic.check_grad(d.permute(0, 2, 3, 1).reshape(R, K), want, tol, f"logits K {K} npix {R}")
        return
    big = torch.zeros(2 * (R * K + 8), device=DEV)
    a = big[off:off + R * K].view(R, K).copy_(p)
    if form == "rows":
        out, _, _, grads = rows_fwd_bwd(a, ic.UPSTREAMS[:1], off)
        marg, cond, want = ic.ref_rows(p, ic.UPSTREAMS[0])
        ic.check_entropies(out, (marg, cond), tol, f"rows K {K} R {R} align {align}")
        ic.check_grad(grads[0], want, tol, f"rows K {K} R {R} align {align}")
    else:
        q = torch.roll(p, 1, dims=0)
        start = (R * K + 7) // 4 * 4 + off
        b = big[start:start + R * K].view(R, K).copy_(q)
        out, _, _, grads = pair_fwd_bwd(a, b, ic.PAIR_UPSTREAMS[1:], off)
        check_pair(p, q, out, grads, ic.PAIR_UPSTREAMS[1:], tol, f"pair K {K} R {R} align {align}")


# ---------------------------------------------------------------------------------------------- 6. from logits
class _Calls:
    def __init__(self, monkeypatch):
        from cyhip import _lib
        self.names, real = [], _lib.call
        monkeypatch.setattr(_lib, "call", lambda name, *a: (self.names.append(name), real(name, *a))[1])


@pytest.mark.parametrize("K", ic.LOGIT_K + ic.LOGIT_COMPOSED_K)
@pytest.mark.parametrize("npix", ic.LOGIT_NPIX)
def test_from_logits(monkeypatch, tol, K, npix):
    from cyhip.functions import softmax_imsat
    shape = (1, K, 1, 1) if npix == 1 else (1, K, 1, 257) if npix == 257 else (3, K, 19, 19)
    z = ic.seeded_logits(shape, seed=K * npix)
    for i, g in enumerate(ic.UPSTREAMS):
        x = gpu_leaf(z if i < 2 else z.contiguous(memory_format=torch.channels_last))
        calls = _Calls(monkeypatch)
        marg, cond = softmax_imsat(x)
        (g[0] * marg + g[1] * cond).backward()
        monkeypatch.undo()
        m64, c64, want = ic.ref_logits(z, g)
        ic.check_entropies((marg, cond), (m64, c64), tol, f"logits K {K} npix {npix}")
        ic.check_grad(x.grad, want, tol, f"logits K {K} npix {npix} upstream {g}")
        if K in ic.LOGIT_COMPOSED_K:
            assert calls.names == ["cy_group_softmax_fwd", "cy_imsat_fwd", "cy_imsat_bwd", "cy_group_softmax_bwd"]
        else:
            assert calls.names == ["cy_softmax_imsat_fwd", "cy_softmax_imsat_bwd"]


# ---------------------------------------------------------------------------------------------- 7. determinism
def test_two_runs_give_the_same_bits():
    from cyhip.functions import IMSATFn, IMSATPairFn, softmax_imsat
    p, q = ic.seeded_rows(40, 3001, seed=1), ic.seeded_rows(40, 3001, seed=2)
    z = ic.seeded_logits((3, 5, 37, 41), seed=3)
    runs = []
    for _ in range(2):
        got = []
        a, b, x = gpu_leaf(p), gpu_leaf(q), gpu_leaf(z)
        marg, cond = IMSATFn.apply(a)
        (marg - 0.5 * cond).backward()
        got += [marg.detach().cpu(), cond.detach().cpu(), a.grad.cpu()]
        a = gpu_leaf(p)
        outs = IMSATPairFn.apply(a, b)
        sum(w * o for w, o in zip((1.0, 0.5, -1.0, 2.0, 3.0), outs)).backward()
        got += [o.detach().cpu() for o in outs] + [a.grad.cpu(), b.grad.cpu()]
        marg, cond = softmax_imsat(x)
        (cond - marg).backward()
        got += [marg.detach().cpu(), cond.detach().cpu(), x.grad.cpu()]
        runs.append(got)
    for u, v in zip(*runs):
        assert torch.equal(u, v)


# ---------------------------------------------------------------------------------------------- 8. dynamic weight
def test_dynamic_weight_follows_the_reference_without_a_host_sync(npz, tol):
    from contrastyou.losses.discreteMI import IMSATDynamicWeight
    p = fx.case_probs(npz, fx.DYN_CASE)
    scale = float(npz[f"{fx.DYN_CASE}_cond64"]) + fx.DYN_LAMDA * float(npz[f"{fx.DYN_CASE}_marg64"])
    off = IMSATDynamicWeight(lamda=fx.DYN_LAMDA, use_dynamic=False).to(DEV)
    loss = off(p.to(DEV))
    ic.check_value(loss, npz["dyn_off_loss64"], scale, tol, "dynamic weight off")
    assert float(off.dynamic_weight) == float(npz["dyn_off_w64"]) == fx.DYN_LAMDA
    dyn = IMSATDynamicWeight(lamda=fx.DYN_LAMDA, use_dynamic=True).to(DEV)
    xs = [gpu_leaf(p) for _ in range(fx.DYN_CALLS)]
    torch.cuda.synchronize()
    losses, weights = [], []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i, x in enumerate(xs):
            loss = dyn(x)
            if i == 0:
                loss.backward()
            losses.append(loss.detach())
            weights.append(dyn.dynamic_weight.clone())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert dyn.dynamic_weight.is_cuda and list(dyn.state_dict()) == ["dynamic_weight"]
    for i in range(fx.DYN_CALLS):
        ic.check_value(losses[i], npz["dyn_loss64"][i], scale, tol, f"dynamic weight call {i}")
        e = abs(float(weights[i]) - float(npz["dyn_w64"][i])) / float(npz["dyn_w64"][i])
        print(f"dynamic weight after call {i}: {float(weights[i]):.9g} vs {float(npz['dyn_w64'][i]):.9g}  e {e:.2e}")
        assert e <= tol["scalar"]
    ic.check_grad(xs[0].grad, torch.from_numpy(npz["dyn_g64"]), tol, "dynamic weight gradient")


# ---------------------------------------------------------------------------------------------- 9. the epocher hooks
def test_output_hook_against_the_reference(npz, tol):
    from semi_seg.hooks.midl import IMSATTrainHook
    from contrastyou.hooks.base import TrainerHook
    type(TrainerHook).names.clear()
    try:
        ep = _Epocher()
        hook = ep.adopt(IMSATTrainHook(weight=fx.HOOK_OUT["weight"])())
    finally:
        type(TrainerHook).names.clear()
    a, b = gpu_leaf(fx.decode(npz["out_tf_logits_i8d8"])), gpu_leaf(fx.decode(npz["out_logits_tf_i8d8"]))
    value = hook(unlabeled_tf_logits=a, unlabeled_logits_tf=b, seed=1, affine_transformer=identity)
    value.backward()
    ic.check_value(value, npz["out_value64"], npz["out_scale64"], tol, "output hook")
    ic.check_grad(a.grad, torch.from_numpy(npz["out_g_tf_logits64"]), tol, "output hook d tf_logits")
    ic.check_grad(b.grad, torch.from_numpy(npz["out_g_logits_tf64"]), tol, "output hook d logits_tf")
    meters = ep.summary(hook)
    ic.check_value(meters["mi"], npz["out_meter_mi64"][0], npz["out_scale64"] / fx.HOOK_OUT["weight"], tol, "meter mi")


class _Stored:
    """stand-in for the feature extractor: the stored features, as the tap would hold them after the forward pass"""

    def __init__(self, feat):
        self.feat = feat

    def bind(self):
        pass

    remove = clear = bind

    def set_enable(self, enable=True):
        pass

    def tail(self, rows):
        return self.feat[-rows:]


def test_intermediate_hook_against_the_reference(npz):
    from contrastyou.losses.discreteMI import IMSATLoss
    from contrastyou.projectors.heads import DenseClusterHead
    from oracle import next_rows as onr
    from semi_seg.hooks.discretemi import _DiscreteIMSATEpochHook
    tol = fx.tolerances(npz, mid=True)
    print("tolerances (intermediate hook)", tol)
    h = fx.HOOK_MID
    sds = onr.init_cluster_sds(h["C"], h["clusters"], h["subheads"], True, seed=h["seed"])
    head = DenseClusterHead(input_dim=h["C"], num_clusters=h["clusters"], num_subheads=h["subheads"],
                            head_type="linear", T=1, normalize=False)
    head.load_state_dict({f"_headers.{i}.{k}": v for i, s in enumerate(sds) for k, v in s.items()}, strict=True)
    head.to(DEV)
    feat = gpu_leaf(fx.decode(npz["mid_feat_i8d8"]))
    ep = _Epocher()
    hook = ep.adopt(_DiscreteIMSATEpochHook(
        name="imsat_mid", weight=h["weight"], extractor=_Stored(feat), projector=head, criterion=IMSATLoss(lamda=1.0),
        cons_criterion=torch.nn.MSELoss(), cons_weight=h["cons_weight"]))
    images = torch.zeros(h["n_unl"], 1, 8, 8, device=DEV)
    value = hook(unlabeled_image=images, unlabeled_image_tf=images, affine_transformer=identity, seed=1)
    value.backward()
    ic.check_value(value, npz["mid_value64"], npz["mid_scale64"], tol, "intermediate hook")
    ic.check_grad(feat.grad, torch.from_numpy(npz["mid_g_feat64"]), tol, "intermediate hook d features")
    names = [n for n, _ in head.named_parameters()]
    assert sorted(f"mid_g_{n}64" for n in names) == sorted(k for k in npz if k.startswith("mid_g__headers"))
    for n, q in head.named_parameters():
        ic.check_grad(q.grad, torch.from_numpy(npz[f"mid_g_{n}64"]), tol, f"intermediate hook d {n}")
    meters = ep.summary(hook)
    ic.check_value(meters["mi"], npz["mid_meter_mi64"][0], npz["mid_scale64"] / h["weight"], tol, "meter mi")
    ic.check_value(meters["cons"], npz["mid_meter_cons64"][0], npz["mid_meter_cons64"][0], tol, "meter cons")


class _StepTrainer:
    def __init__(self, model, max_epoch):
        self._model, self._max_epoch = model, max_epoch


def _one_step(sd0, lab, unl, weight):
    """one SemiSupervisedEpocher step on the 128-channel toy U-Net, with IMSATTrainHook(weight) (None: no hook) ->
    (state dict after the step, metrics)"""
    import random
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from contrastyou.losses.kl import KL_div
    from contrastyou.optim import RAdam
    from semi_seg.epochers import SemiSupervisedEpocher
    from semi_seg.hooks import IMSATTrainHook
    type(TrainerHook).names.clear()
    try:
        model = UNet(input_dim=1, num_classes=4, max_channel=128, momentum=0.1)
        model.load_state_dict(sd0)
        model.to(DEV)
        trainer = _StepTrainer(model, max_epoch=10)
        opt = RAdam([{"params": list(model.parameters())}], lr=3e-3, weight_decay=1e-4)
        ep = SemiSupervisedEpocher(model=model, optimizer=opt, labeled_loader=Loader(lab), unlabeled_loader=Loader(unl),
                                   sup_criterion=KL_div(), num_batches=1, cur_epoch=0, device=DEV, two_stage=True,
                                   disable_bn=False, scaler=torch.amp.GradScaler("cuda", enabled=False),
                                   accumulate_iter=1)
        ep.init(trainer)
        random.seed(9)
        torch.manual_seed(3)
        if weight is None:
            ep.run()
        else:
            hook = IMSATTrainHook(weight=weight).to(DEV)
            hook.register_trainer(trainer)
            with ep.register_hook(hook()):
                ep.run()
        torch.cuda.synchronize()
        return {k: v.detach().float().cpu() for k, v in model.state_dict().items()}, ep.get_metric()
    finally:
        type(TrainerHook).names.clear()


def test_a_semi_supervised_step_with_the_output_hook():
    """the hook's term reaches the network: a finite loss, and the step ends in other weights than without the hook
    (the same batches, seeds and optimiser: only the gradient of the logits differs)"""
    from oracle import unet as ou
    sd0 = ou.init_state_dict(1, 4, 128, seed=14)
    g = torch.Generator().manual_seed(21)
    lab, unl = [blob_batch(4, 32, 4, g)], [blob_batch(4, 32, 4, g)]
    with_hook, m = _one_step(sd0, lab, unl, 0.1)
    without, _ = _one_step(sd0, lab, unl, None)
    print(m["imsat"], "reg_loss", m["semi"]["reg_loss"])
    assert np.isfinite(m["semi"]["reg_loss"]) and m["semi"]["reg_loss"] != 0
    assert np.isfinite(m["imsat"]["mi"])
    assert all(torch.isfinite(v).all() for v in with_hook.values())
    assert any(not torch.equal(with_hook[k], without[k]) for k in sd0 if k.endswith(".weight"))
