"""The kernels that run in every training step (csrc/cy_misc.hip: affine_fwd_kernel, affine_bwd_kernel, ema_kernel,
radam_kernel) and contrastyou/optim/fused_radam.py against the same operation in float64 on the CPU, written out in
plain torch expressions on the values the kernel actually reads: 16-bit inputs are rounded to the storage type first,
scalars to f32, because the kernels take them as `float`.  The cases are the tables of tests/step_kernel_cases.py;
tests/test_step_kernel_coverage.py proves on the CPU that they reach what they claim.

Exact where the operation is exact (the forward is a pure gather), a bound derived from the number of f32 roundings
where it is a short sum (backward, EMA), and 4 x a measured yardstick where the device's function accuracy is not
derivable (powf, the RAdam step as a whole).  Output buffers are NaN before the call, slices are surrounded by guard
elements that must survive bit for bit, and every figure is printed before it is asserted."""
import copy
import ctypes as C
import functools

import pytest
import torch

from tests import step_kernel_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"
TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CODE = {"f32": 0, "bf16": 1, "f16": 2}
# significand bits behind the leading one, smallest normal exponent
FMT = {"f32": (23, -126), "bf16": (7, -126), "f16": (10, -14)}
U32 = 2.0 ** -24   # unit roundoff of f32
NAN = float("nan")


def _ops():
    from cyhip import ops
    return ops


def nhwc(t, dtype):
    """CPU NCHW tensor -> GPU tensor of `dtype` with NHWC memory"""
    return t.to(dtype).to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def affine_call(kind, t, theta, gamma=None):
    """cy_affine_nearest_fwd / _bwd into an output that is NaN before the call (ops.affine_* allocate theirs uninitialised,
    where a block of the caching allocator can still hold an earlier, correct result)"""
    from cyhip import _lib, ops
    assert ops.is_nhwc(t) and theta.is_cuda and theta.dtype == torch.float32 and theta.is_contiguous()
    N, Cc, H, W = t.shape
    out = torch.full((N, H, W, Cc), NAN, dtype=t.dtype, device=DEV).permute(0, 3, 1, 2)
    code = ops.dtype_code(t.dtype)
    if kind == "fwd":
        _lib.call("cy_affine_nearest_fwd", t.data_ptr(), out.data_ptr(), theta.data_ptr(), ops._ptr(gamma), N, Cc, H, W,
                  code, ops._stream())
    else:
        _lib.call("cy_affine_nearest_bwd", t.data_ptr(), out.data_ptr(), theta.data_ptr(), N, Cc, H, W, code,
                  ops._stream())
    return out


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def ulp(ref, dt):
    """spacing of the storage type `dt` at |ref| (float64 tensor); 0 for f32, whose rounding the bounds carry themselves"""
    if dt == "f32":
        return torch.zeros_like(ref)
    p, emin = FMT[dt]
    e = torch.frexp(ref.abs())[1].double() - 1.0   # floor(log2 |ref|)
    e = torch.where(ref == 0, torch.full_like(e, float(emin)), e).clamp_min(float(emin))
    return torch.exp2(e - p)


def theta_tensor(thetas):
    return torch.tensor([t.rows for t in thetas], dtype=torch.float32)


# ================================================================ affine: references
@functools.lru_cache(maxsize=None)
def source_index(names, H, W):
    from oracle.losses import affine_source_index
    thetas = [sc.THETAS[sc.THETA_NAMES.index(n)] for n in names]
    return affine_source_index(theta_tensor(thetas), H, W)


def scatter_reference(dout64, src, valid):
    """the adjoint of the gather, as an explicit scatter in float64: (dx, k = contributions per input pixel,
    sum of |terms| per input element).  dout64 [N, C, H, W]"""
    N, Cc, H, W = dout64.shape
    dx = torch.zeros(N, H * W, Cc, dtype=torch.float64)
    mag = torch.zeros(N, H * W, Cc, dtype=torch.float64)
    k = torch.zeros(N, H * W, dtype=torch.float64)
    rows = dout64.permute(0, 2, 3, 1).reshape(N, H * W, Cc)
    for n in range(N):
        v = valid[n]
        dx[n].index_add_(0, src[n][v], rows[n][v])
        mag[n].index_add_(0, src[n][v], rows[n][v].abs())
        k[n].index_add_(0, src[n][v], torch.ones(int(v.sum()), dtype=torch.float64))
    back = lambda t: t.view(N, H, W, Cc).permute(0, 3, 1, 2)  # noqa: E731
    return back(dx), k.view(N, 1, H, W), back(mag)


def affine_inputs(geom, dt, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(*geom, generator=g) * 2 - 1).to(TD[dt])
    dout = (torch.rand(*geom, generator=g) * 2 - 1).to(TD[dt])
    return x, dout


def check_forward(out, x, thetas, dt, what):
    from oracle.losses import affine_nearest
    ref = affine_nearest(x.double(), theta_tensor(thetas)).to(TD[dt])
    got = out.cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    print(f"{what}: {int((got != ref).sum())} of {ref.numel()} elements differ; {int((ref != 0).sum())} non-zero")
    assert not bool(torch.isnan(got.float()).any()), f"{what}: NaN left in the output"
    assert torch.equal(got, ref), f"{what}: {int((got != ref).sum())} elements differ from the gather"


def check_backward(dx, dout, thetas, dt, what):
    N, Cc, H, W = dout.shape
    src, valid = source_index(tuple(t.name for t in thetas), H, W)
    ref, k, mag = scatter_reference(dout.double(), src, valid)
    got = dx.cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    # rounding of the f32 sum to the storage type, and k f32 additions; a pixel nothing maps onto must hold an exact zero
    bound = torch.where(k == 0, torch.zeros_like(ref), ulp(ref, dt) / 2 + k * U32 * mag)
    err = (got - ref).abs()
    over = err > bound
    worst = (err - bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}  max bound {bound.max().item():.3e}  max k {int(k.max())}  "
          f"pixels with k = 0: {int((k == 0).sum())}  err - bound <= {worst:.3e}")
    assert not bool(torch.isnan(got).any()), f"{what}: NaN in dx"
    assert not bool(over.any()), (f"{what}: {int(over.sum())} elements past ulp/2 + k 2^-24 sum|terms|; the worst has "
                                 f"err {err[over].max().item():.3e}; per image {over.flatten(1).sum(1).tolist()} "
                                 f"under {[t.name for t in thetas]}")


AFFINE_PARAMS = [pytest.param(g, k, dt, id=f"{sc.ident(g)}-{sc.THETAS[k].name}-{dt}")
                 for g in sc.AFFINE_GEOMS for k in range(len(sc.THETAS)) for dt in sc.TYPES]


# ================================================================ 1. affine forward, no gamma
@pytest.mark.parametrize("geom,k,dt", AFFINE_PARAMS)
def test_affine_forward_is_the_gather(geom, k, dt):
    thetas = sc.batch_thetas(k, geom.N)
    x, _ = affine_inputs(geom, dt, seed=100 + k)
    out = affine_call("fwd", nhwc(x, TD[dt]), theta_tensor(thetas).to(DEV))
    check_forward(out, x, thetas, dt, f"forward {sc.ident(geom)} {[t.name for t in thetas]} {dt}")


# ================================================================ 2. affine backward
@pytest.mark.parametrize("geom,k,dt", AFFINE_PARAMS)
def test_affine_backward_is_the_scatter(geom, k, dt):
    thetas = sc.batch_thetas(k, geom.N)
    _, dout = affine_inputs(geom, dt, seed=100 + k)
    dx = affine_call("bwd", nhwc(dout, TD[dt]), theta_tensor(thetas).to(DEV))
    check_backward(dx, dout, thetas, dt, f"backward {sc.ident(geom)} {[t.name for t in thetas]} {dt}")


def test_affine_autograd_function_routes_to_both_kernels():
    """AffineFn is the only autograd definition of the op: its backward is the scatter of its forward (through
    ops.affine_fwd / ops.affine_bwd, which allocate their own outputs)"""
    from cyhip.functions import AffineFn
    geom, dt = sc.AFFINE_GEOMS[0], "f32"
    thetas = sc.batch_thetas(2, geom.N)
    x, dout = affine_inputs(geom, dt, seed=7)
    xg = nhwc(x, TD[dt]).requires_grad_(True)
    out = AffineFn.apply(xg, theta_tensor(thetas).to(DEV), None)
    out.backward(nhwc(dout, TD[dt]))
    check_forward(out.detach(), x, thetas, dt, "AffineFn forward")
    check_backward(xg.grad, dout, thetas, dt, "AffineFn backward")


# ================================================================ 3. gamma
def gamma_inputs(geom, dt, seed=31):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(*geom, generator=g)
    x.view(-1)[0::17] = 0.0   # exact zeros and ones in every image
    x.view(-1)[5::17] = 1.0
    return x.to(TD[dt]), torch.tensor(sc.GAMMAS, dtype=torch.float32)


def gamma_reference(x, gam, thetas):
    from oracle.losses import affine_nearest
    return affine_nearest(x.double() ** gam.double().view(-1, 1, 1, 1), theta_tensor(thetas))


def yardstick_gamma():
    """max relative error of torch's CPU f32 `x ** g` against float64 on the inputs of the gamma test (run by hand;
    the result is recorded in tests/step_kernel_cases.py)"""
    worst = 0.0
    for geom in sc.GAMMA_GEOMS:
        for dt in sc.TYPES:
            x, gam = gamma_inputs(geom, dt)
            ref = x.double() ** gam.double().view(-1, 1, 1, 1)
            got = (x.float() ** gam.view(-1, 1, 1, 1)).double()
            nz = ref != 0
            worst = max(worst, ((got - ref).abs()[nz] / ref.abs()[nz]).max().item())
            assert bool((got[~nz] == 0).all())
    return worst


@pytest.mark.parametrize("dt", sc.TYPES)
@pytest.mark.parametrize("geom", sc.GAMMA_GEOMS, ids=sc.ident)
def test_affine_forward_with_gamma(geom, dt):
    assert geom.N == len(sc.GAMMAS)
    thetas = sc.batch_thetas(1, geom.N, sc.PRODUCTION_THETAS)
    x, gam = gamma_inputs(geom, dt)
    assert bool((x == 0).any()) and bool((x == 1).any())
    out = affine_call("fwd", nhwc(x, TD[dt]), theta_tensor(thetas).to(DEV), gam.to(DEV))
    ref = gamma_reference(x, gam, thetas)
    got = out.cpu().double()
    err = (got - ref).abs()
    nz = ref != 0
    rel = (err[nz] / ref.abs()[nz]).max().item()
    bound = sc.GAMMA_BOUND * ref.abs() + ulp(ref, dt) / 2
    print(f"gamma {sc.ident(geom)} {dt}: max relative err {rel:.3e} (yardstick {sc.GAMMA_YARDSTICK:.2e}, f32 bound "
          f"{sc.GAMMA_BOUND:.2e}); ones {int((ref == 1).sum())} zeros {int((ref == 0).sum())}")
    assert bool((ref == 1).any()) and bool(nz.any())
    assert not bool(torch.isnan(got).any())
    assert not bool((err > bound).any()), f"gamma {sc.ident(geom)} {dt}: {int((err > bound).sum())} elements past the bound"


# ================================================================ 4. past the cap
def test_affine_past_the_grid_cap():
    geom, dt = sc.AFFINE_CAP, sc.AFFINE_CAP_TYPE
    thetas = sc.batch_thetas(0, geom.N, sc.PRODUCTION_THETAS[2:])   # three rotated production thetas
    x, dout = affine_inputs(geom, dt, seed=5)
    th = theta_tensor(thetas).to(DEV)
    out = affine_call("fwd", nhwc(x, TD[dt]), th)
    dx = affine_call("bwd", nhwc(dout, TD[dt]), th)
    check_forward(out, x, thetas, dt, f"forward past the cap {sc.ident(geom)}")
    check_backward(dx, dout, thetas, dt, f"backward past the cap {sc.ident(geom)}")


# ================================================================ 5. EMA
@functools.lru_cache(maxsize=None)
def flat_inputs(n, seed):
    """four guarded f32 buffers of n + SLICE_OFF + GUARD elements: p / teacher, grad / student, m, v >= 0"""
    g = torch.Generator().manual_seed(seed)
    total = n + sc.SLICE_OFF + sc.GUARD
    p = torch.rand(total, generator=g) * 2 - 1
    s = torch.rand(total, generator=g) * 2 - 1
    m = (torch.rand(total, generator=g) * 2 - 1) * 0.5
    v = torch.rand(total, generator=g)
    v[sc.SLICE_OFF::7] = 0.0   # moments that have seen no gradient yet
    return p, s, m, v


def sl(t, n):
    return t[sc.SLICE_OFF:sc.SLICE_OFF + n]


def guards_intact(after, before, n, what):
    a, b = bits(after), bits(before)
    lo, hi = sc.SLICE_OFF, sc.SLICE_OFF + n
    assert torch.equal(a[:lo], b[:lo]), f"{what}: the elements before the slice were written"
    assert torch.equal(a[hi:], b[hi:]), f"{what}: the elements behind the slice were written"


def f32_scalar(v):
    return torch.tensor(v, dtype=torch.float32)


@pytest.mark.parametrize("wd", sc.EMA_WDS)
@pytest.mark.parametrize("alpha", sc.EMA_ALPHAS)
@pytest.mark.parametrize("n", sc.ELEMENT_COUNTS)
def test_ema_on_a_slice(n, alpha, wd):
    ops = _ops()
    t0, s0, _, _ = flat_inputs(n, 21)
    tg, sg = t0.to(DEV), s0.to(DEV)
    ops.ema_update(sl(tg, n), sl(sg, n), alpha, wd)
    # the kernel's scalars: alpha, 1 - alpha and keep = 1 - wd, each an f32 value
    a = f32_scalar(alpha)
    a64, b64, keep = a.double(), (f32_scalar(1.0) - a).double(), (f32_scalar(1.0) - f32_scalar(wd)).double()
    t, s = sl(t0, n).double(), sl(s0, n).double()
    ref = (a64 * t + b64 * s) * keep
    # at most four f32 roundings (two products, the sum, the final product; a contracted product saves one), doubled
    bound = 8 * U32 * ((a64 * t).abs() + (b64 * s).abs())
    err = (sl(tg, n).cpu().double() - ref).abs()
    print(f"ema n {n} alpha {alpha} wd {wd}: max err {err.max().item():.3e}  max err / bound "
          f"{(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert not bool((err > bound).any()), f"{int((err > bound).sum())} of {n} elements past 8 * 2^-24 (|a t| + |(1-a) s|)"
    guards_intact(tg, t0, n, "teacher")
    assert torch.equal(bits(sg), bits(s0)), "the student buffer was written"


# ================================================================ 6. RAdam kernel
def radam_scalars(s):
    return {k: sc.f32(getattr(s, k)) for k in ("beta1", "beta2", "eps", "wd", "lr")}


def radam_reference(p, g, m, v, s, step):
    """float64 transcription of torch.optim.RAdam (decoupled_weight_decay=False), one step from (p, m, v) at `step`"""
    h = radam_scalars(s)
    b1, b2 = h["beta1"], h["beta2"]
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    if h["wd"] != 0:
        g = g + h["wd"] * p
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    hat = m / bc1
    rho_inf = 2.0 / (1.0 - b2) - 1.0
    rho_t = rho_inf - 2.0 * step * b2 ** step / bc2
    if rho_t > 5.0:
        rect = ((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t)) ** 0.5
        p = p - hat * h["lr"] * rect * (bc2 ** 0.5 / (v.sqrt() + h["eps"]))
    else:
        p = p - hat * h["lr"]
    return {"p": p, "exp_avg": m, "exp_avg_sq": v}


def radam_torch_f32(p, g, m, v, s, step):
    """the yardstick's side: torch.optim.RAdam in f32 on the CPU, walked to `step` by setting its state"""
    h = radam_scalars(s)
    q = torch.nn.Parameter(p.clone())
    q.grad = g.clone()
    opt = torch.optim.RAdam([q], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["wd"],
                            foreach=False)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    return {"p": q.detach(), "exp_avg": opt.state[q]["exp_avg"], "exp_avg_sq": opt.state[q]["exp_avg_sq"]}


def radam_errors(got, ref):
    return {k: ((got[k].double() - ref[k]).abs().max() / ref[k].abs().max().clamp_min(1e-300)).item() for k in ref}


def yardstick_radam():
    """max over radam_cases() of max|err| / max|ref| per output of torch's f32 CPU step (run by hand; the result is
    recorded in tests/step_kernel_cases.py)"""
    worst = {"p": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}
    for s, step, n in sc.radam_cases():
        p, g, m, v = (sl(t, n) for t in flat_inputs(n, 22))
        e = radam_errors(radam_torch_f32(p, g, m, v, s, step), radam_reference(p, g, m, v, s, step))
        worst = {k: max(worst[k], e[k]) for k in worst}
    return worst


@pytest.mark.parametrize("s,step,n", [pytest.param(s, st, n, id=f"{s.name}-step{st}-n{n}")
                                      for s, st, n in sc.radam_cases()])
def test_radam_step_on_a_slice(s, step, n):
    ops = _ops()
    host = flat_inputs(n, 22)
    ref = radam_reference(*(sl(t, n) for t in host), s, step)

    def run():
        p, g, m, v = (t.to(DEV) for t in host)
        ops.radam_step(sl(p, n), sl(g, n), sl(m, n), sl(v, n), s.lr, s.beta1, s.beta2, s.eps, s.wd, step)
        return p, g, m, v

    p, g, m, v = run()
    got = {"p": sl(p, n).cpu(), "exp_avg": sl(m, n).cpu(), "exp_avg_sq": sl(v, n).cpu()}
    err = radam_errors(got, ref)
    print(f"radam {s.name} step {step} (rectified: {sc.rectified(s.beta2, step)}) n {n}: " +
          "  ".join(f"{k} {err[k]:.3e} (bound {sc.RADAM_BOUND[k]:.2e})" for k in err))
    for k in err:
        assert not bool(torch.isnan(got[k]).any()), k
        assert err[k] <= sc.RADAM_BOUND[k], f"{k}: {err[k]:.3e} of max|ref| > {sc.RADAM_BOUND[k]:.2e}"
    for name, after, before in (("param", p, host[0]), ("exp_avg", m, host[2]), ("exp_avg_sq", v, host[3])):
        guards_intact(after, before, n, name)
    assert torch.equal(bits(g), bits(host[1])), "the gradient buffer was written"
    p2, _, m2, v2 = run()
    assert torch.equal(bits(p2), bits(p)) and torch.equal(bits(m2), bits(m)) and torch.equal(bits(v2), bits(v)), \
        "a second call on identical inputs gave different bits"


# ================================================================ 7. FusedRAdam end to end
def fused_hypers():
    return dict(lr=sc.f32(sc.FUSED_LR), betas=(sc.f32(0.9), sc.f32(0.999)), eps=sc.f32(1e-8),
                weight_decay=sc.f32(sc.FUSED_WD))


def fused_loss(params, targets, step):
    """a small quadratic; the second parameter takes no part in it for the first FUSED_SKIP_UNTIL steps"""
    w, b, u = params
    loss = ((w - targets[0]) ** 2).sum() + 0.5 * ((u * u).sum() - (u * targets[2]).sum())
    if step > sc.FUSED_SKIP_UNTIL:
        loss = loss + ((w.sum(0) + b - targets[1]) ** 2).sum()
    return loss


def fused_run(opt, params, targets, first, last, each_step):
    for step in range(first, last + 1):
        opt.zero_grad()
        fused_loss(params, targets, step).backward()
        each_step(step, "grads")
        opt.step()
        each_step(step, "stepped")


def test_fused_radam_against_torch_radam_and_state_dict_round_trip():
    from contrastyou.optim.fused_radam import FusedRAdam
    g = torch.Generator().manual_seed(41)
    init = [torch.rand(*shp, generator=g) * 2 - 1 for shp in sc.FUSED_SHAPES]
    targets = [torch.rand(*shp, generator=g) * 2 - 1 for shp in sc.FUSED_SHAPES]
    tg = [t.to(DEV) for t in targets]
    params = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    opt = FusedRAdam(params, **fused_hypers())
    refs = [torch.nn.Parameter(t.clone().double()) for t in init]
    ref_opt = torch.optim.RAdam(refs, foreach=False, **fused_hypers())
    history, snapshot = {}, {}

    def each_step(step, when):
        flat, st = opt._flat[0], opt._flat_state[0]
        if when == "grads":
            assert flat.offsets == [0, 35, 42, 63]
            touched = flat.touched()
            assert touched == [True, step > sc.FUSED_SKIP_UNTIL, True], (step, touched)
            for i, r in enumerate(refs):   # the same gradients, copied from the flat buffer
                a, b = flat.offsets[i], flat.offsets[i + 1]
                r.grad = flat.grad[a:b].cpu().double().view(r.shape) if touched[i] else None
            ref_opt.step()
            return
        want_steps = [int(ref_opt.state[r]["step"]) if r in ref_opt.state and ref_opt.state[r] else 0 for r in refs]
        assert st["steps"] == want_steps, (step, st["steps"], want_steps)
        assert want_steps[1] == max(0, step - sc.FUSED_SKIP_UNTIL), "the second parameter's count lags"
        # both sides consume the same gradients, so they part only by the rounding of each optimizer step; the
        # moments forget at rates beta < 1, so the parts add up at most linearly: step count x the one-step bound
        for i, (p, r) in enumerate(zip(params, refs)):
            err = (p.detach().cpu().double() - r.detach()).abs().max().item()
            tol = step * sc.RADAM_BOUND["p"] * r.detach().abs().max().item()
            print(f"FusedRAdam step {step} parameter {i}: err {err:.3e}  bound {tol:.3e}")
            assert err <= tol, f"step {step} parameter {i}: {err:.3e} > {tol:.3e}"
        history[step] = [p.detach().clone() for p in params]
        if step == sc.FUSED_RESUME_AFTER:   # what a checkpoint holds: a copy, not the live moments
            snapshot["state"] = copy.deepcopy(opt.state_dict())
            snapshot["params"] = [p.detach().clone() for p in params]

    fused_run(opt, params, tg, 1, sc.FUSED_STEPS, each_step)
    assert bits(params[1]).ne(bits(init[1])).any(), "the skipped parameter moved once it took part"
    assert torch.equal(bits(history[sc.FUSED_SKIP_UNTIL][1]), bits(init[1])), "a skipped parameter must not move"

    # resume from the state of step 6 with a fresh optimizer over cloned parameters: bit-equal to the uninterrupted run
    params2 = [torch.nn.Parameter(t.clone()) for t in snapshot["params"]]
    opt2 = FusedRAdam(params2, **fused_hypers())
    opt2.load_state_dict(snapshot["state"])

    def each_step2(step, when):
        if when == "stepped":
            for i, (p, h) in enumerate(zip(params2, history[step])):
                assert torch.equal(bits(p), bits(h)), f"resumed run differs at step {step}, parameter {i}"

    fused_run(opt2, params2, tg, sc.FUSED_RESUME_AFTER + 1, sc.FUSED_STEPS, each_step2)
    assert opt2._flat_state[0]["steps"] == opt._flat_state[0]["steps"]
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(bits(opt2._flat_state[0][k]), bits(opt._flat_state[0][k])), k


# ================================================================ 8. rejections
def test_rejections_return_the_exact_code():
    from cyhip import _lib
    lib = _lib.load()
    buf = C.create_string_buffer(64)   # a refused call launches nothing, so host memory does
    p = C.addressof(buf)
    seen = []

    def expect(what, got, want):
        assert what in sc.REJECTS, what
        assert got == want, f"{what}: {got}, expected {want}"
        seen.append(what)

    expect("radam step 0", lib.cy_radam_step(p, p, p, p, 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, None), sc.ERR_ARG)
    expect("radam n 0", lib.cy_radam_step(p, p, p, p, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None), sc.ERR_ARG)
    expect("ema n 0", lib.cy_ema_update(p, p, 0, 0.5, 0.0, None), sc.ERR_ARG)
    expect("affine fwd dtype 7", lib.cy_affine_nearest_fwd(p, p, p, None, 1, 1, 1, 1, 7, None), sc.ERR_DTYPE)
    expect("affine bwd dtype 7", lib.cy_affine_nearest_bwd(p, p, p, 1, 1, 1, 1, 7, None), sc.ERR_DTYPE)
    for dt in sc.TYPES:
        assert lib.cy_affine_nearest_fwd(p, p, p, None, 1, 0, 1, 1, CODE[dt], None) == sc.ERR_ARG, dt
        assert lib.cy_affine_nearest_bwd(p, p, p, 1, 0, 1, 1, CODE[dt], None) == sc.ERR_ARG, dt
    expect("affine fwd C 0", lib.cy_affine_nearest_fwd(p, p, p, None, 1, 0, 1, 1, 0, None), sc.ERR_ARG)
    expect("affine bwd C 0", lib.cy_affine_nearest_bwd(p, p, p, 1, 0, 1, 1, 0, None), sc.ERR_ARG)
    assert sorted(seen) == sorted(sc.REJECTS)


def test_affine_backward_through_gamma_is_refused():
    from cyhip.functions import AffineFn
    geom = sc.GAMMA_GEOMS[0]
    x, gam = gamma_inputs(geom, "f32")
    xg = nhwc(x, torch.float32).requires_grad_(True)
    out = AffineFn.apply(xg, theta_tensor(sc.batch_thetas(0, geom.N, sc.PRODUCTION_THETAS)).to(DEV), gam.to(DEV))
    with pytest.raises(RuntimeError, match="gamma"):
        out.sum().backward()
