"""Parity of the BatchNorm, pool and upsample kernels (csrc/cy_norm_act.hip with cy_bn_acc.h) on every branch of their
launch plan and past every launch cap.  The cases are those of tests/norm_act_cases.py; tests/test_norm_act_plan_coverage.py
checks on the CPU, from cy_norm_act_plan, that they reach what they claim.  Everything goes through the C ABI
(_lib.call) on flat NHWC buffers.

Reference: float64 torch on the CPU (on the device for the seven capped cases), on inputs already rounded to the
storage type.

Elementwise outputs are judged per element: |got_i - ref_i| <= r * |ref_i| + y_i, with r one unit in the last place of
the storage type (2^-7 bf16, 2^-10 f16, 0 f32; r * |ref_i| is no less than the fixed step of the type below its normal range,
2^-24 for f16) and y_i four times the error a plain float32 torch evaluation of the same
formula makes AT THAT ELEMENT against the float64 reference on the same inputs.  Where float32 happens to land on the
exact value that error is zero, and a kernel whose fused multiply-add chain rounds otherwise there could not pass, so
the error has a floor of half a float32 unit in the last place of the formula's terms at that element:
    y_i = 4 * max(|f32_i - ref_i|, 2^-24 * m_i),   m_i = |scale y| + |shift|  (apply),  |scale dz| + |k1 y| + |k0|  (backward)
The kernels compute in float32 whatever the storage type, so the floor holds for all three types.  Both float32 and
float64 evaluations take the ReLU mask from the sign of the exact scale * y + shift (what fmaf gives), so a flipped
mask cannot inflate y.  y is computed at run time from torch alone, never from the kernels.
The dy of the whole backward (reduce, finalize, apply against autograd) also depends on the two float32 sums, whose own
bound is chain * 2^-23 * sum |term| (below); that bound, carried through dy = scale * (dz - sum dz / n - xhat * sum(dz
xhat) / n), is added for those two checks: |scale| / n * chain * 2^-23 * (sum |dz| + |xhat_i| * sum |dz xhat|).

Per-channel sums (partial rows, accumulators, dgamma, dbeta) are compared with the float64 sums of dz and dz * xhat
within chain * 2^-23 * sum |term|, `chain` being the longest float32 addition chain the plan reports.  Two allowances
come on top, from the number formats: an accumulator adds partial_rows * 2^-44 (the resolution of its low limb, once per
adding workgroup); parameter gradients ADDED into old f32 values and read back as new - old add
2^-22 * (|old| + |sum|) (the sum's rounding to f32 and the rounding of the f32 addition, two units of 2^-24 each way).
Values that come out of float64 arithmetic rounded once to f32 (finalize, fold coefficients) get 2^-23 of their magnitude.

Exact results (pool routing and ties, the single rounding of g + add, the upsample sum, pooled outputs, fused against
unfused dx, run against run) are compared without tolerance.  Every launch runs twice, into two NaN-filled buffers with
guard bands, and must write every element, nothing else, and the same bits."""
import ctypes as C

import pytest
import torch

from tests import norm_act_cases as nc
from tests.bn_acc_checks import acc_encode, words_sums

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 2048  # elements before and after every output
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 0.0}
# ... which below the smallest normal number is a fixed step: f16 values under 2^-14 are 2^-24 apart (bf16: 2^-133)
STEP = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24, torch.float32: 0.0}
SENTINEL = 0x5A5A5A5A5A5A5A5A
WORST = {}  # kernel -> (worst error / bound, case)


def _lib():
    from cyhip import _lib as m
    return m


def code(dt):
    from cyhip import ops
    return ops.dtype_code(dt)


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    lines = [f"{k}: worst error / bound {v[0]:.3f} ({v[1]})" for k, v in sorted(WORST.items())]
    print("\n" + "\n".join(lines))


def note(kernel, ratio, what):
    if ratio > WORST.get(kernel, (-1.0, ""))[0]:
        WORST[kernel] = (float(ratio), what)


# ---------------------------------------------------------------- outputs with guard bands, run twice
def guarded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def twice(launch, specs, what):
    """launch(*views) twice into fresh NaN-filled buffers; every element written, guards intact, same bits"""
    runs = []
    for _ in range(2):
        pairs = [guarded(n, dt) for n, dt in specs]
        launch(*[v for _, v in pairs])
        torch.cuda.synchronize()
        for (buf, v), (n, _) in zip(pairs, specs):
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), f"{what}: guard band written"
            assert not bool(torch.isnan(v).any()), f"{what}: output element not written (or NaN)"
        runs.append([v for _, v in pairs])
    for a, b in zip(*runs):
        assert bits_equal(a, b), f"{what}: two runs differ"
    return runs[0]


def bits_equal(a, b):
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def new_acc(R, Cc, words=None):
    """a zeroed (or given) accumulator [R][4][C] + R flags between sentinel words; (buffer, view, BnAcc)"""
    n = R * 4 * Cc + R
    buf = torch.full((n + 32,), SENTINEL, dtype=torch.int64, device=DEV)
    v = buf[16:16 + n]
    v.zero_()
    if words is not None:
        v[:R * 4 * Cc] = words.reshape(-1).to(DEV)
    return buf, v, _lib().BnAcc(v.data_ptr(), R, Cc)


def acc_read(buf, R, Cc, what):
    assert bool((buf[:16] == SENTINEL).all()) and bool((buf[-16:] == SENTINEL).all()), f"{what}: wrote around the accumulator"
    v = buf[16:-16].cpu()
    assert int(v[R * 4 * Cc:].abs().sum()) == 0, f"{what}: flag set"
    return words_sums(v[:R * 4 * Cc].view(R, 4, Cc))


def widen(t):
    """[n, C] -> the left half of a [n, 2C] tensor whose right half is NaN (a row stride of 2C)"""
    n, Cc = t.shape
    w = torch.full((n, 2 * Cc), float("nan"), dtype=t.dtype, device=t.device)
    w[:, :Cc] = t
    return w


# ---------------------------------------------------------------- criteria
def assert_elementwise(got, ref, f32, mag, dt, kernel, what, extra=None):
    """per element: |got - ref| <= max(ULP * |ref|, STEP) + 4 * max(|f32 - ref|, 2^-24 * mag) (+ extra)"""
    ref = ref.double()
    y = 4.0 * torch.maximum((f32.double() - ref).abs(), 2.0 ** -24 * mag.double())
    bound = (ULP[dt] * ref.abs()).clamp_min(STEP[dt]) + y
    if extra is not None:
        bound = bound + extra
    err = (got.double() - ref).abs()
    bad = err > bound
    rat = torch.where(bound > 0, err / bound.clamp_min(1e-300), (err > 0).double() * 1e30).flatten()
    ratio, at = rat.max().item(), int(rat.argmax())
    note(kernel, ratio, what)
    assert not bool(bad.any()), (f"{what}: {kernel} off at {int(bad.sum())} of {bad.numel()} elements, worst error / bound "
                                 f"{ratio:.3g} at {at}: got {got.flatten()[at].item():.9g}, float64 {ref.flatten()[at].item():.9g}, "
                                 f"float32 {f32.flatten()[at].item():.9g}, terms {mag.flatten()[at].item():.3g}")


def check_apply(got, y, c64, c32, dt, kernel, what):
    """got against relu(scale * y + shift): c64 / c32 = (scale, shift) for the float64 / float32 evaluation"""
    mag = (c64[0].double() * y.double()).abs() + c64[1].double().abs()
    assert_elementwise(got, apply_ref(y, c64[0], c64[1], torch.float64), apply_ref(y, c32[0], c32[1], torch.float32), mag,
                       dt, kernel, what)


def check_bwd(got, da, y, sc, sh, k64, k32, dt, kernel, what):
    """got against scale * dz + k1 * y + k0: k64 / k32 = (k1, k0) for the float64 / float32 evaluation"""
    dz = torch.where(mask_of(y, sc, sh), da.double(), torch.zeros((), dtype=torch.float64, device=y.device))
    mag = (sc.double() * dz).abs() + (k64[0].double() * y.double()).abs() + k64[1].double().abs()
    assert_elementwise(got, bwd_apply_ref(da, y, sc, sh, k64[0], k64[1], torch.float64),
                       bwd_apply_ref(da, y, sc, sh, k32[0], k32[1], torch.float32), mag, dt, kernel, what)


def assert_sums(got, ref, absum, chain, kernel, what, extra=0.0):
    """got, ref, absum: [2, C] float64 (the sums of dz and dz * xhat; the sums of |term|)"""
    bound = chain * 2.0 ** -23 * absum + extra
    err = (got.double().cpu() - ref.cpu()).abs()
    ratio = (err / bound.cpu().clamp_min(1e-300)).max().item()
    note(kernel, ratio, what)
    assert ratio <= 1.0, f"{what}: {kernel} sums off, worst error / bound {ratio:.3g} (chain {chain})"


def assert_rounded_once(got, ref, slack, kernel, what):
    """got: f32 results of float64 arithmetic rounded once; ref float64; slack: float64 cancellation allowance"""
    bound = 2.0 ** -23 * ref.abs() + slack
    err = (got.double().cpu() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.max().item() > 0 else 0.0
    note(kernel, ratio, what)
    assert ratio <= 1.0, f"{what}: {kernel} worst error / bound {ratio:.3g}"


# ---------------------------------------------------------------- references (any device; t = float64 or float32)
def mask_of(y, sc, sh):
    return (sc.double() * y.double() + sh.double()) > 0  # the sign of the exact value, as fmaf gives it


def apply_ref(y, sc, sh, t):
    return torch.relu(sc.to(t) * y.to(t) + sh.to(t))


def bwd_apply_ref(da, y, sc, sh, k1, k0, t):
    dz = torch.where(mask_of(y, sc, sh), da.to(t), torch.zeros((), dtype=t, device=y.device))
    return sc.to(t) * dz + k1.to(t) * y.to(t) + k0.to(t)


def fold_coefs(s1, s2, count, gamma, beta, eps, t):
    """[5, C] scale, shift, mean, invstd, unbiased variance from the two sums, in type t"""
    s1, s2 = s1.to(t), s2.to(t)
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0)
    istd = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    g = torch.ones_like(mean) if gamma is None else gamma.to(t)
    b = torch.zeros_like(mean) if beta is None else beta.to(t)
    unb = var * (count / (count - 1.0) if count > 1 else 1.0)
    return torch.stack([g * istd, b - mean * g * istd, mean, istd, unb])


def bwd_fold_coefs(t1, t2, sc, mu, istd, count, batch_stats, t):
    """(k1, k0) of dy = scale * dz + k1 * y + k0"""
    if not batch_stats:
        return torch.zeros_like(t1.to(t)), torch.zeros_like(t1.to(t))
    k1 = -sc.to(t) * istd.to(t) * t2.to(t) / count
    return k1, -sc.to(t) * t1.to(t) / count - k1 * mu.to(t)


def reduce_ref(da, y, sc, sh, mu, istd):
    """float64 sums [2, C] of dz and dz * xhat, and of their magnitudes"""
    dz = torch.where(mask_of(y, sc, sh), da.double(), torch.zeros((), dtype=torch.float64, device=y.device))
    t2 = dz * ((y.double() - mu.double()) * istd.double())
    return torch.stack([dz.sum(0), t2.sum(0)]), torch.stack([dz.abs().sum(0), t2.abs().sum(0)])


def pool_bwd_ref(x, g, add, N, h, w, Cc):
    """first maximum in scan order takes the gradient; a single rounding of g + add"""
    xv = x.view(N, h, 2, w, 2, Cc).permute(0, 1, 3, 5, 2, 4).reshape(N, h, w, Cc, 4).float()
    eq = xv == xv.max(-1, keepdim=True).values
    first = eq & (eq.cumsum(-1) == 1)
    o = torch.where(first, g.view(N, h, w, Cc, 1).float(), torch.zeros((), device=x.device))
    o = o.reshape(N, h, w, Cc, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N * 4 * h * w, Cc)
    if add is not None:
        o = o + add.float()
    return o.to(x.dtype)


def up_bwd_ref(dup, N, h, w, Cc):
    v = dup.view(N, h, 2, w, 2, Cc).float()
    return ((v[:, :, 0, :, 0] + v[:, :, 0, :, 1]) + (v[:, :, 1, :, 0] + v[:, :, 1, :, 1])).reshape(N * h * w, Cc).to(dup.dtype)


def maxpool_of(out, N, h, w, Cc):
    return out.view(N, h, 2, w, 2, Cc).float().amax((2, 4)).reshape(N * h * w, Cc).to(out.dtype)


def coefs(Cc, gen, dev="cpu"):
    """per-channel f32 inputs: scale, shift, mean, invstd, k1, k0"""
    r = lambda: torch.rand(Cc, generator=gen)  # noqa: E731
    n = lambda: torch.randn(Cc, generator=gen)  # noqa: E731
    out = [r() + 0.5, n() * 0.5, n() * 0.3, r() + 0.5, n() * 0.1, n() * 0.1]
    out[0][::3] *= -1.0  # negative gammas too
    return [t.to(dev) for t in out]


def rnd(n, Cc, dt, gen, relu=False):
    t = torch.randn(n, Cc, generator=gen)
    return (torch.relu(t) if relu else t).to(dt)


# ---------------------------------------------------------------- launches
def k_apply(y, sc, sh, npix, Cc, dt, odt, what):
    def go(out):
        _lib().call("cy_bn_relu_apply", y.data_ptr(), sc.data_ptr(), sh.data_ptr(), out.data_ptr(), npix, Cc, code(dt),
                    code(odt), stream())
    return twice(go, [(npix * Cc, odt)], what)[0].view(npix, Cc)


def k_apply_pool(y, sc, sh, N, h, w, Cc, dt, what):
    def go(out, pooled):
        _lib().call("cy_bn_relu_apply_pool", y.data_ptr(), sc.data_ptr(), sh.data_ptr(), out.data_ptr(), pooled.data_ptr(),
                    N, h, w, Cc, code(dt), code(dt), stream())
    out, pooled = twice(go, [(N * 4 * h * w * Cc, dt), (N * h * w * Cc, dt)], what)
    return out.view(-1, Cc), pooled.view(-1, Cc)


def fold_struct(acc, gamma, beta, count, eps, coef):
    L = _lib()
    return L.BnFold(acc.acc, acc.R, acc.C, None if gamma is None else gamma.data_ptr(),
                    None if beta is None else beta.data_ptr(), float(count), float(eps), 0, coef.data_ptr())


def k_apply_fold(y, f, npix, Cc, dt, odt, what):
    def go(out, coef):
        f.coef = coef.data_ptr()
        _lib().call("cy_bn_relu_apply_fold", y.data_ptr(), C.byref(f), out.data_ptr(), npix, code(dt), code(odt), stream())
    out, coef = twice(go, [(npix * Cc, odt), (5 * Cc, torch.float32)], what)
    return out.view(npix, Cc), coef.view(5, Cc)


def k_apply_pool_fold(y, f, N, h, w, Cc, dt, what):
    def go(out, pooled, coef):
        f.coef = coef.data_ptr()
        _lib().call("cy_bn_relu_apply_pool_fold", y.data_ptr(), C.byref(f), out.data_ptr(), pooled.data_ptr(), N, h, w,
                    code(dt), code(dt), stream())
    out, pooled, coef = twice(go, [(N * 4 * h * w * Cc, dt), (N * h * w * Cc, dt), (5 * Cc, torch.float32)], what)
    return out.view(-1, Cc), pooled.view(-1, Cc), coef.view(5, Cc)


def k_bwd_apply(da, ld, y, sc, sh, k1, k0, npix, Cc, dt, what):
    coef = torch.cat([k1, k0]).contiguous()

    def go(dy):
        _lib().call("cy_bn_relu_bwd_apply", da.data_ptr(), ld, y.data_ptr(), sc.data_ptr(), sh.data_ptr(), coef.data_ptr(),
                    dy.data_ptr(), npix, Cc, code(dt), stream())
    return twice(go, [(npix * Cc, dt)], what)[0].view(npix, Cc)


def k_bwd_apply_fold(da, ld, y, coef5, acc, count, batch_stats, dg, db, accumulate, npix, Cc, dt, what):
    """dg / db: None, or f32 [C] tensors the launch writes or adds into (restored before the second run)"""
    keep = [None if t is None else t.clone() for t in (dg, db)]
    outs = []

    def go(dy):
        for t, k in zip((dg, db), keep):
            if t is not None:
                t.copy_(k)
        _lib().call("cy_bn_relu_bwd_apply_fold", da.data_ptr(), ld, y.data_ptr(), coef5.data_ptr(), C.byref(acc), float(count),
                    int(batch_stats), None if dg is None else dg.data_ptr(), None if db is None else db.data_ptr(),
                    int(accumulate), dy.data_ptr(), npix, Cc, code(dt), stream())
        outs.append([None if t is None else t.clone() for t in (dg, db)])
    dy = twice(go, [(npix * Cc, dt)], what)[0].view(npix, Cc)
    for a, b in zip(*outs):
        assert a is None or bits_equal(a, b), f"{what}: parameter gradients differ between two runs"
    return dy


def k_reduce(da, ld, y, sc, sh, mu, istd, npix, Cc, dt, P, what):
    def go(part):
        _lib().call("cy_bn_relu_bwd_reduce", da.data_ptr(), ld, y.data_ptr(), sc.data_ptr(), sh.data_ptr(), mu.data_ptr(),
                    istd.data_ptr(), part.data_ptr(), npix, Cc, code(dt), stream())
    return twice(go, [(P * 2 * Cc, torch.float32)], what)[0].view(P, 2, Cc)


def k_reduce_acc(da, ld, y, coef5, R, npix, Cc, dt, what):
    res = []
    for _ in range(2):
        buf, v, acc = new_acc(R, Cc)
        _lib().call("cy_bn_relu_bwd_reduce_acc", da.data_ptr(), ld, y.data_ptr(), coef5.data_ptr(), C.byref(acc), npix, Cc,
                    code(dt), stream())
        torch.cuda.synchronize()
        res.append(buf)
    assert torch.equal(res[0], res[1]), f"{what}: two runs leave different accumulator words"
    return torch.stack(acc_read(res[0], R, Cc, what))


def k_pool_bwd(x, g, add, ld_add, N, h, w, Cc, dt, what):
    def go(dx):
        _lib().call("cy_maxpool2_bwd", x.data_ptr(), g.data_ptr(), None if add is None else add.data_ptr(), ld_add,
                    dx.data_ptr(), N, h, w, Cc, code(dt), stream())
    return twice(go, [(N * 4 * h * w * Cc, dt)], what)[0].view(-1, Cc)


def k_pool_bwd_bn(x, g, add, ld_add, y, sc, sh, mu, istd, N, h, w, Cc, dt, P, what):
    def go(dx, part):
        _lib().call("cy_maxpool2_bwd_bn", x.data_ptr(), g.data_ptr(), None if add is None else add.data_ptr(), ld_add,
                    dx.data_ptr(), y.data_ptr(), sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), istd.data_ptr(),
                    part.data_ptr(), N, h, w, Cc, code(dt), stream())
    dx, part = twice(go, [(N * 4 * h * w * Cc, dt), (P * 2 * Cc, torch.float32)], what)
    return dx.view(-1, Cc), part.view(P, 2, Cc)


def k_pool_bwd_bn_acc(x, g, add, ld_add, y, coef5, R, N, h, w, Cc, dt, what):
    bufs = []

    def go(dx):
        buf, v, acc = new_acc(R, Cc)
        _lib().call("cy_maxpool2_bwd_bn_acc", x.data_ptr(), g.data_ptr(), None if add is None else add.data_ptr(), ld_add,
                    dx.data_ptr(), y.data_ptr(), coef5.data_ptr(), C.byref(acc), N, h, w, Cc, code(dt), stream())
        bufs.append(buf)
    dx = twice(go, [(N * 4 * h * w * Cc, dt)], what)[0].view(-1, Cc)
    assert torch.equal(bufs[0], bufs[1]), f"{what}: two runs leave different accumulator words"
    return dx, torch.stack(acc_read(bufs[0], R, Cc, what))


def k_up_bwd(dup, ld, N, h, w, Cc, dt, what):
    def go(dx):
        _lib().call("cy_upsample2_bwd", dup.data_ptr(), ld, dx.data_ptr(), N, h, w, Cc, code(dt), stream())
    return twice(go, [(N * h * w * Cc, dt)], what)[0].view(-1, Cc)


def k_up_bwd_bn_acc(dup, ld, y, coef5, R, N, h, w, Cc, dt, what):
    bufs = []

    def go(dx):
        buf, v, acc = new_acc(R, Cc)
        _lib().call("cy_upsample2_bwd_bn_acc", dup.data_ptr(), ld, dx.data_ptr(), y.data_ptr(), coef5.data_ptr(), C.byref(acc),
                    N, h, w, Cc, code(dt), stream())
        bufs.append(buf)
    dx = twice(go, [(N * h * w * Cc, dt)], what)[0].view(-1, Cc)
    assert torch.equal(bufs[0], bufs[1]), f"{what}: two runs leave different accumulator words"
    return dx, torch.stack(acc_read(bufs[0], R, Cc, what))


def make_acc_words(s1, s2, R, gen):
    """the two float64 sums [C] spread unevenly, with mixed signs, over R replicas: int64 words [R][4][C] and the sums a
    consumer reads from them"""
    Cc = s1.numel()
    wgt = torch.randn(R, 1, Cc, generator=gen, dtype=torch.float64) * 3.0
    wgt[-1] = 1.0 - wgt[:-1].sum(0)
    words = acc_encode(torch.stack([s1, s2])[None] * wgt)
    return words, words_sums(words)


# ================================================================ the backward reduce
@pytest.mark.parametrize("c", nc.REDUCE_CASES, ids=nc.case_id)
def test_reduce_against_float64_sums(c):
    dt, npix, Cc = nc.torch_dtype(c.dtype), c.npix, c.C
    p = nc.reduce_plan(c)
    what = nc.case_id(c)
    gen = torch.Generator().manual_seed(npix * 7 + Cc)
    da, y = rnd(npix, Cc, dt, gen), rnd(npix, Cc, dt, gen)
    sc, sh, mu, istd, _, _ = coefs(Cc, gen)
    ref, absum = reduce_ref(da, y, sc, sh, mu, istd)
    dda, dy_ = da.to(DEV), y.to(DEV)
    dsc, dsh, dmu, dis = (t.to(DEV) for t in (sc, sh, mu, istd))
    P = p["partial_rows"]
    part = k_reduce(dda, Cc, dy_, dsc, dsh, dmu, dis, npix, Cc, dt, P, what)
    kernel = "bwd_reduce deep" if p["deep"] else "bwd_reduce"
    assert_sums(part.double().sum(0), ref, absum, p["chain"], kernel, what)
    # every row holds the sums of its own pixels; the trailing workgroups without pixels write zeros
    per = p["pixels_per_workgroup"]
    full = P - p["empty_workgroups"]
    if p["empty_workgroups"]:
        assert int(part[full:].count_nonzero()) == 0, f"{what}: an empty workgroup wrote something else than zeros"
    for b in sorted({0, full - 1}):
        r, a = reduce_ref(da[b * per:(b + 1) * per], y[b * per:(b + 1) * per], sc, sh, mu, istd)
        assert_sums(part[b].double(), r, a, p["chain"], kernel, f"{what} row {b}")
    # a row stride of 2 C (the other columns NaN) changes nothing
    wide = widen(dda)
    assert bits_equal(k_reduce(wide, 2 * Cc, dy_, dsc, dsh, dmu, dis, npix, Cc, dt, P, what + " ld_da=2C"), part)
    # the same sums into an accumulator of R replicas
    coef5 = torch.stack([dsc, dsh, dmu, dis, torch.zeros_like(dsc)]).contiguous()
    R = max(1, min(8, 2048 // Cc if Cc <= 2048 else 1))
    got = k_reduce_acc(wide, 2 * Cc, dy_, coef5, R, npix, Cc, dt, what + " acc")
    assert_sums(got, ref, absum, p["chain"], kernel + " acc", what, extra=P * 2.0 ** -44)


# ================================================================ every elementwise launch on the small geometry
@pytest.mark.parametrize("c", nc.EW_CASES, ids=nc.case_id)
def test_elementwise_small(c):
    dt, N, H, W, Cc = nc.torch_dtype(c.dtype), c.N, c.H, c.W, c.C
    h, w, npix = H // 2, W // 2, c.N * c.H * c.W
    what = nc.case_id(c)
    gen = torch.Generator().manual_seed(Cc * 31 + N)
    y, da = rnd(npix, Cc, dt, gen), rnd(npix, Cc, dt, gen)
    sc, sh, mu, istd, k1, k0 = coefs(Cc, gen)
    dev = lambda *ts: [t.to(DEV) for t in ts]  # noqa: E731
    dy_, dda = dev(y, da)
    dsc, dsh, dmu, dis, dk1, dk0 = dev(sc, sh, mu, istd, k1, k0)

    # ---- apply, plain and pooled, and the mixed-type form
    out = k_apply(dy_, dsc, dsh, npix, Cc, dt, dt, what)
    check_apply(out.cpu(), y, (sc, sh), (sc, sh), dt, "apply", what)
    out2, pooled = k_apply_pool(dy_, dsc, dsh, N, h, w, Cc, dt, what)
    assert bits_equal(out2, out), f"{what}: pooled apply's full-size output differs from the plain apply"
    assert torch.equal(pooled, maxpool_of(out, N, h, w, Cc)), f"{what}: pooled output is not max_pool2d of the stored output"
    if c.mixed:
        o32 = k_apply(dy_, dsc, dsh, npix, Cc, dt, torch.float32, what + "->f32")
        check_apply(o32.cpu(), y, (sc, sh), (sc, sh), torch.float32, "apply mixed", what)

    # ---- the same on an accumulator (R = 2) holding the float64 sums of y
    gamma, beta = (torch.rand(Cc, generator=gen) + 0.5), torch.randn(Cc, generator=gen) * 0.5
    words, (s1, s2) = make_acc_words(y.double().sum(0), (y.double() ** 2).sum(0), 2, gen)
    abuf, _, acc = new_acc(2, Cc, words)
    dgamma_, dbeta_ = dev(gamma, beta)
    f = fold_struct(acc, dgamma_, dbeta_, npix, 1e-5, torch.empty(5 * Cc, device=DEV))
    c64 = fold_coefs(s1, s2, float(npix), gamma, beta, 1e-5, torch.float64)
    c32 = fold_coefs(s1, s2, float(npix), gamma, beta, 1e-5, torch.float32)
    outf, coef = k_apply_fold(dy_, f, npix, Cc, dt, dt, what + " fold")
    check_apply(outf.cpu(), y, (c64[0], c64[1]), (c32[0], c32[1]), dt, "apply fold", what)
    assert_rounded_once(coef, c64, 1e-12 * (1 + c64.abs()), "fold coefficients", what)
    outf2, pooledf, coef2 = k_apply_pool_fold(dy_, f, N, h, w, Cc, dt, what + " pool fold")
    assert bits_equal(outf2, outf) and bits_equal(coef2, coef), f"{what}: pooled fold apply differs from the fold apply"
    assert torch.equal(pooledf, maxpool_of(outf, N, h, w, Cc))
    if c.mixed:
        o32, _ = k_apply_fold(dy_, f, npix, Cc, dt, torch.float32, what + " fold->f32")
        check_apply(o32.cpu(), y, (c64[0], c64[1]), (c32[0], c32[1]), torch.float32, "apply fold mixed", what)
    acc_read(abuf, 2, Cc, what)  # consumers only read

    # ---- backward apply on given coefficients, row stride C and 2 C
    dy = k_bwd_apply(dda, Cc, dy_, dsc, dsh, dk1, dk0, npix, Cc, dt, what)
    check_bwd(dy.cpu(), da, y, sc, sh, (k1, k0), (k1, k0), dt, "bwd_apply", what)
    assert bits_equal(k_bwd_apply(widen(dda), 2 * Cc, dy_, dsc, dsh, dk1, dk0, npix, Cc, dt, what + " ld_da=2C"), dy)

    # ---- the whole backward (reduce, finalize, apply; reduce into an accumulator, fold apply) against autograd
    backward_chain(c, y, da, gamma, beta, gen)

    # ---- max-pool backward: ties from a ReLU'd input, with and without the addend, row stride 2 C
    x, g, add = rnd(npix, Cc, dt, gen, relu=True), rnd(npix // 4, Cc, dt, gen), rnd(npix, Cc, dt, gen)
    dx_, dg_, dadd = dev(x, g, add)
    assert int((x.view(N, h, 2, w, 2, Cc).float().amax((2, 4)) == 0).sum()) > 0, "no all-zero window: no four-way tie"
    dx0 = k_pool_bwd(dx_, dg_, None, Cc, N, h, w, Cc, dt, what + " pool_bwd")
    assert torch.equal(dx0.cpu(), pool_bwd_ref(x, g, None, N, h, w, Cc)), f"{what}: max-pool backward routing"
    dx1 = k_pool_bwd(dx_, dg_, widen(dadd), 2 * Cc, N, h, w, Cc, dt, what + " pool_bwd add")
    assert torch.equal(dx1.cpu(), pool_bwd_ref(x, g, add, N, h, w, Cc)), f"{what}: max-pool backward with the addend"
    # ---- upsample backward: (a + b) + (c + d) in float32, rounded once
    up = k_up_bwd(widen(dda), 2 * Cc, N, h, w, Cc, dt, what + " up_bwd")
    assert torch.equal(up.cpu(), up_bwd_ref(da, N, h, w, Cc)), f"{what}: upsample backward"

    # ---- the fused-sum forms: same dx; sums over the stored gradient; refused where C/8 does not divide 256
    pp = nc.plan("pool_bwd_bn", N, h, w, Cc, c.dtype, 1)
    pu = nc.plan("up_bwd_bn", N, h, w, Cc, c.dtype, 1)
    coef5 = torch.stack([dsc, dsh, dmu, dis, torch.zeros_like(dsc)]).contiguous()
    ylo = y[: npix // 4].contiguous()
    L = _lib()
    if Cc in nc.FUSED_REFUSED_C:
        assert not pp["fused_ok"] and not pu["fused_ok"]
        dxb, part = guarded(npix * Cc, dt)[1], guarded(2 * Cc, torch.float32)[1]
        _, _, acc1 = new_acc(1, Cc)
        rc = L.load().cy_maxpool2_bwd_bn(dx_.data_ptr(), dg_.data_ptr(), None, Cc, dxb.data_ptr(), dy_.data_ptr(),
                                         dsc.data_ptr(), dsh.data_ptr(), dmu.data_ptr(), dis.data_ptr(), part.data_ptr(),
                                         N, h, w, Cc, code(dt), stream())
        ru = L.load().cy_upsample2_bwd_bn_acc(dda.data_ptr(), Cc, dxb.data_ptr(), ylo.to(DEV).data_ptr(), coef5.data_ptr(),
                                              C.byref(acc1), N, h, w, Cc, code(dt), stream())
        torch.cuda.synchronize()
        assert rc == ru == -2 and bool(torch.isnan(dxb).all()) and bool(torch.isnan(part).all()), "refused: nothing launched"
        return
    assert pp["fused_ok"] and pu["fused_ok"]
    dxf, part = k_pool_bwd_bn(dx_, dg_, widen(dadd), 2 * Cc, dy_, dsc, dsh, dmu, dis, N, h, w, Cc, dt, pp["partial_rows"],
                              what + " pool_bwd_bn")
    assert bits_equal(dxf, dx1), f"{what}: fused max-pool backward writes another dx"
    ref, absum = reduce_ref(dx1.cpu(), y, sc, sh, mu, istd)
    assert_sums(part.double().sum(0), ref, absum, pp["chain"], "pool_bwd_bn", what)
    dxa, got = k_pool_bwd_bn_acc(dx_, dg_, None, Cc, dy_, coef5, 1, N, h, w, Cc, dt, what + " pool_bwd_bn_acc")
    assert bits_equal(dxa, dx0)
    ref, absum = reduce_ref(dx0.cpu(), y, sc, sh, mu, istd)
    assert_sums(got, ref, absum, pp["chain"], "pool_bwd_bn acc", what, extra=pp["partial_rows"] * 2.0 ** -44)
    upf, got = k_up_bwd_bn_acc(widen(dda), 2 * Cc, ylo.to(DEV), coef5, 1, N, h, w, Cc, dt, what + " up_bwd_bn_acc")
    assert bits_equal(upf, up), f"{what}: fused upsample backward writes another dx"
    ref, absum = reduce_ref(up.cpu(), ylo, sc, sh, mu, istd)
    assert_sums(got, ref, absum, pu["chain"], "up_bwd_bn acc", what, extra=pu["partial_rows"] * 2.0 ** -44)


def backward_chain(c, y, da, gamma, beta, gen):
    """relu(batch_norm(y)) backward at da: dy against float64 autograd; the float32 evaluation is the backward formula
    scale * (dz - mean dz - xhat * mean(dz xhat)) written out in float32 on float32 statistics, with the float64
    forward's ReLU mask"""
    import torch.nn.functional as F
    dt, Cc, npix = nc.torch_dtype(c.dtype), c.C, y.shape[0]
    what = nc.case_id(c) + " chain"
    yy = y.double().requires_grad_(True)
    a64 = F.relu(F.batch_norm(yy, None, None, gamma.double(), beta.double(), True, 0.0, 1e-5))
    a64.backward(da.double())
    dy64, mask = yy.grad, a64.detach() > 0

    def formula(t):
        v, g = y.to(t), gamma.to(t)
        mean = v.mean(0)
        istd = torch.rsqrt(v.var(0, unbiased=False) + 1e-5)
        xhat = (v - mean) * istd
        dz = torch.where(mask, da.to(t), torch.zeros((), dtype=t))
        k1 = -g * istd * istd * (dz * xhat).mean(0)
        k0 = -g * istd * dz.mean(0) - k1 * mean
        carried = (g * istd).abs() / npix * (dz.abs().sum(0) + xhat.abs() * (dz * xhat).abs().sum(0))
        return g * istd * (dz - dz.mean(0) - xhat * (dz * xhat).mean(0)), (g * istd * dz).abs() + (k1 * v).abs() + k0.abs(), carried
    dy32, (_, mag, carried) = formula(torch.float32)[0], formula(torch.float64)
    # the forward coefficients, from float64 statistics, rounded to the f32 the kernels are handed
    y64 = y.double()
    c5 = fold_coefs(y64.sum(0), (y64 ** 2).sum(0), float(npix), gamma, beta, 1e-5, torch.float64).float()
    sc, sh, mu, istd = c5[0], c5[1], c5[2], c5[3]
    ref, absum = reduce_ref(da, y, sc, sh, mu, istd)
    d = lambda t: t.contiguous().to(DEV)  # noqa: E731
    dda, dy_, dsc, dsh, dmu, dis = d(da), d(y), d(sc), d(sh), d(mu), d(istd)
    p = nc.plan("bwd_reduce", 1, 1, npix, Cc, c.dtype)
    P = p["partial_rows"]
    part = k_reduce(dda, Cc, dy_, dsc, dsh, dmu, dis, npix, Cc, dt, P, what)
    assert_sums(part.double().sum(0), ref, absum, p["chain"], "bwd_reduce deep", what)

    def fin(coef, dg, db):
        _lib().call("cy_bn_bwd_finalize", part.data_ptr(), P, Cc, dsc.data_ptr(), dmu.data_ptr(), dis.data_ptr(), float(npix), 1,
                    dg.data_ptr(), db.data_ptr(), 0, coef.data_ptr(), stream())
    coef, dg, db = twice(fin, [(2 * Cc, torch.float32)] + [(Cc, torch.float32)] * 2, what + " bwd_finalize")
    assert_sums(torch.stack([db, dg]), ref, absum, p["chain"], "bwd_finalize dgamma dbeta", what)
    dy = k_bwd_apply(dda, Cc, dy_, dsc, dsh, coef[:Cc].contiguous(), coef[Cc:].contiguous(), npix, Cc, dt, what)
    carried = p["chain"] * 2.0 ** -23 * carried  # the sums' own bound, carried through to dy
    assert_elementwise(dy.cpu(), dy64, dy32, mag, dt, "backward chain dy", what, extra=carried)
    # the accumulator path: reduce into R = 4 replicas (2 where 4 C words exceed a consumer's budget), fold apply
    if Cc > 1024:
        return
    R = 4 if 4 * Cc <= 2048 else 2
    coef5 = d(c5)
    bufs = []
    for _ in range(2):
        buf, _, acc = new_acc(R, Cc)
        _lib().call("cy_bn_relu_bwd_reduce_acc", dda.data_ptr(), Cc, dy_.data_ptr(), coef5.data_ptr(), C.byref(acc), npix, Cc,
                    code(dt), stream())
        torch.cuda.synchronize()
        bufs.append(buf)
    assert torch.equal(bufs[0], bufs[1]), f"{what}: two reduce launches leave different accumulator words"
    old = torch.randn(2, Cc, generator=gen)
    dgo, dbo = d(old[0]), d(old[1])
    dyf = k_bwd_apply_fold(dda, Cc, dy_, coef5, acc, npix, 1, dgo, dbo, 1, npix, Cc, dt, what + " fold")
    assert_elementwise(dyf.cpu(), dy64, dy32, mag, dt, "backward chain dy (fold)", what, extra=carried)
    got = torch.stack([dbo.cpu().double() - old[1].double(), dgo.cpu().double() - old[0].double()])
    assert_sums(got, ref, absum, p["chain"], "bwd_apply fold dgamma dbeta", what,
                extra=2.0 ** -22 * (old.abs().flip(0).double() + ref.abs()) + P * 2.0 ** -44)


# ================================================================ past every launch cap (bf16; references on the device)
@pytest.mark.parametrize("b", nc.BIG_CASES, ids=nc.case_id)
def test_second_trip_of_every_capped_loop(b):
    dt, N, H, W, Cc = torch.bfloat16, b.N, b.H, b.W, b.C
    gen = torch.Generator(device=DEV).manual_seed(Cc + H)
    cgen = torch.Generator().manual_seed(Cc + H)
    sc, sh, mu, istd, k1, k0 = coefs(Cc, cgen, DEV)
    r = lambda n, relu=False: (torch.relu(torch.randn(n, Cc, device=DEV, generator=gen)) if relu  # noqa: E731
                                else torch.randn(n, Cc, device=DEV, generator=gen)).to(dt)
    n = N * H * W
    coef5 = torch.stack([sc, sh, mu, istd, torch.zeros_like(sc)]).contiguous()
    for kind in b.kinds:
        what = f"{b.name}:{kind}"
        p = nc.plan(kind, N, H, W, Cc, "bf16", b.fold)
        assert p["trips"] == 2 and p["status"] == 0
        if kind in ("apply", "bwd_apply") and not b.fold:
            y = r(n)
            if kind == "apply":
                out = k_apply(y, sc, sh, n, Cc, dt, dt, what)
                check_apply(out, y, (sc, sh), (sc, sh), dt, "apply", what)
            else:
                da = r(n)
                dy = k_bwd_apply(da, Cc, y, sc, sh, k1, k0, n, Cc, dt, what)
                check_bwd(dy, da, y, sc, sh, (k1, k0), (k1, k0), dt, "bwd_apply", what)
        elif kind in ("apply", "apply_pool", "bwd_apply") and b.fold:
            npix = n * 4 if kind == "apply_pool" else n
            y = r(npix)
            y64 = y.double()
            if kind == "bwd_apply":
                da = r(npix)
                ref, _ = reduce_ref(da, y, sc, sh, mu, istd)
                words, (t1, t2) = make_acc_words(ref[0].cpu(), ref[1].cpu(), b.fold, cgen)
                abuf, _, acc = new_acc(b.fold, Cc, words)
                k64 = bwd_fold_coefs(t1.to(DEV), t2.to(DEV), sc, mu, istd, float(npix), 1, torch.float64)
                k32 = bwd_fold_coefs(t1.to(DEV), t2.to(DEV), sc, mu, istd, float(npix), 1, torch.float32)
                dy = k_bwd_apply_fold(da, Cc, y, coef5, acc, npix, 1, None, None, 0, npix, Cc, dt, what)
                check_bwd(dy, da, y, sc, sh, k64, k32, dt, "bwd_apply fold", what)
                continue
            words, (s1, s2) = make_acc_words(y64.sum(0).cpu(), (y64 ** 2).sum(0).cpu(), b.fold, cgen)
            abuf, _, acc = new_acc(b.fold, Cc, words)
            f = fold_struct(acc, sc, sh, npix, 1e-5, torch.empty(5 * Cc, device=DEV))  # (gamma, beta) = (sc, sh)
            c64 = fold_coefs(s1.to(DEV), s2.to(DEV), float(npix), sc, sh, 1e-5, torch.float64)
            c32 = fold_coefs(s1.to(DEV), s2.to(DEV), float(npix), sc, sh, 1e-5, torch.float32)
            if kind == "apply":
                out, _ = k_apply_fold(y, f, npix, Cc, dt, dt, what)
            else:
                out, pooled, _ = k_apply_pool_fold(y, f, N, H, W, Cc, dt, what)
                assert torch.equal(pooled, maxpool_of(out, N, H, W, Cc)), f"{what}: pooled output"
            check_apply(out, y, (c64[0], c64[1]), (c32[0], c32[1]), dt, "apply fold" if kind == "apply" else "apply_pool fold", what)
        elif kind == "apply_pool":
            y = r(n * 4)
            out, pooled = k_apply_pool(y, sc, sh, N, H, W, Cc, dt, what)
            check_apply(out, y, (sc, sh), (sc, sh), dt, "apply_pool", what)
            assert torch.equal(pooled, maxpool_of(out, N, H, W, Cc)), f"{what}: pooled output"
        elif kind in ("pool_bwd", "pool_bwd_bn"):
            x, g, add = r(n * 4, True), r(n), r(n * 4)
            want = pool_bwd_ref(x, g, add, N, H, W, Cc)
            if kind == "pool_bwd":
                assert torch.equal(k_pool_bwd(x, g, add, Cc, N, H, W, Cc, dt, what), want), f"{what}: routing"
            else:
                y = r(n * 4)
                dx, part = k_pool_bwd_bn(x, g, add, Cc, y, sc, sh, mu, istd, N, H, W, Cc, dt, p["partial_rows"], what)
                assert torch.equal(dx, want), f"{what}: routing"
                ref, absum = reduce_ref(dx, y, sc, sh, mu, istd)
                assert_sums(part.double().sum(0), ref, absum, p["chain"], "pool_bwd_bn", what)
                dx, got = k_pool_bwd_bn_acc(x, g, add, Cc, y, coef5, b.fold, N, H, W, Cc, dt, what + " acc")
                assert torch.equal(dx, want)
                assert_sums(got, ref, absum, p["chain"], "pool_bwd_bn acc", what, extra=p["partial_rows"] * 2.0 ** -44)
        else:
            dup = r(n * 4)
            want = up_bwd_ref(dup, N, H, W, Cc)
            if kind == "up_bwd":
                assert torch.equal(k_up_bwd(dup, Cc, N, H, W, Cc, dt, what), want), f"{what}: upsample backward"
            else:
                y = r(n)
                dx, got = k_up_bwd_bn_acc(dup, Cc, y, coef5, b.fold, N, H, W, Cc, dt, what)
                assert torch.equal(dx, want)
                ref, absum = reduce_ref(dx, y, sc, sh, mu, istd)
                assert_sums(got, ref, absum, p["chain"], "up_bwd_bn acc", what, extra=p["partial_rows"] * 2.0 ** -44)


# ================================================================ accumulator consumers on their own, by replica count
@pytest.mark.parametrize("R", nc.FOLD_RS)
def test_accumulator_consumers_by_replica_count(R):
    N, H, W, Cc = nc.FOLD_GEOM
    h, w, npix = H // 2, W // 2, N * H * W
    dt = torch.float32
    what = f"R{R}"
    gen = torch.Generator().manual_seed(100 + R)
    y, da = rnd(npix, Cc, dt, gen), rnd(npix, Cc, dt, gen)
    gamma, beta = torch.rand(Cc, generator=gen) + 0.5, torch.randn(Cc, generator=gen) * 0.5
    d = lambda t: t.contiguous().to(DEV)  # noqa: E731
    dy_, dda, dgm, dbt = d(y), d(da), d(gamma), d(beta)
    # known sums, not those of y: the consumers must take them from the limbs and from nowhere else
    s1 = torch.randn(Cc, generator=gen, dtype=torch.float64) * 40.0
    s2 = s1 * s1 / npix + npix * (torch.rand(Cc, generator=gen, dtype=torch.float64) + 0.2)
    words, (s1, s2) = make_acc_words(s1, s2, R, gen)
    abuf, av, acc = new_acc(R, Cc, words)
    for null_gb in (False, True):
        g_, b_ = (None, None) if null_gb else (gamma, beta)
        f = fold_struct(acc, None if null_gb else dgm, None if null_gb else dbt, npix, 1e-5, torch.empty(5 * Cc, device=DEV))
        c64 = fold_coefs(s1, s2, float(npix), g_, b_, 1e-5, torch.float64)
        c32 = fold_coefs(s1, s2, float(npix), g_, b_, 1e-5, torch.float32)
        slack = 1e-12 * (1 + c64.abs())

        def go(coef):
            f.coef = coef.data_ptr()
            _lib().call("cy_bn_fold_coef", C.byref(f), stream())
        coef = twice(go, [(5 * Cc, torch.float32)], what + " fold_coef")[0].view(5, Cc)
        assert_rounded_once(coef, c64, slack, "fold_coef", f"{what} null_gb={null_gb}")
        out, coef_a = k_apply_fold(dy_, f, npix, Cc, dt, dt, what + " apply fold")
        assert_rounded_once(coef_a, c64, slack, "fold coefficients", what)
        # (three workgroups: the two that are not the leader derive the same coefficients, or their pixels are off)
        check_apply(out.cpu(), y, (c64[0], c64[1]), (c32[0], c32[1]), dt, "apply fold", what)
        out2, pooled, coef_p = k_apply_pool_fold(dy_, f, N, h, w, Cc, dt, what + " apply_pool fold")
        assert bits_equal(out2, out) and bits_equal(coef_p, coef_a)
        assert torch.equal(pooled, maxpool_of(out, N, h, w, Cc))
    # ---- backward: the same words read as the sums of dz and dz * xhat
    sc, sh, mu, istd, _, _ = coefs(Cc, gen)
    coef5 = d(torch.stack([sc, sh, mu, istd, torch.zeros(Cc)]))
    for batch_stats in (1, 0):
        k64 = bwd_fold_coefs(s1, s2, sc, mu, istd, float(npix), batch_stats, torch.float64)
        k32 = bwd_fold_coefs(s1, s2, sc, mu, istd, float(npix), batch_stats, torch.float32)
        for accumulate in (0, 1):
            old = torch.randn(2, Cc, generator=gen) * 30.0
            dg, db = d(old[0]), d(old[1])
            dy = k_bwd_apply_fold(widen(dda), 2 * Cc, dy_, coef5, acc, npix, batch_stats, dg, db, accumulate, npix, Cc, dt,
                                  f"{what} bwd_apply fold bs={batch_stats} acc={accumulate}")
            check_bwd(dy.cpu(), da, y, sc, sh, k64, k32, dt, "bwd_apply fold", what)
            base = old.double() if accumulate else torch.zeros(2, Cc, dtype=torch.float64)
            want = torch.stack([base[0] + s2.float().double(), base[1] + s1.float().double()])
            assert_rounded_once(torch.stack([dg, db]), want, 2.0 ** -24 * torch.stack([s2, s1]).abs(),
                                "bwd_apply fold dgamma dbeta", f"{what} acc={accumulate}")
        # null gradient pointers: nothing to write, the same dy
        dyn = k_bwd_apply_fold(dda, Cc, dy_, coef5, acc, npix, batch_stats, None, None, 0, npix, Cc, dt, what + " null grads")
        assert bits_equal(dyn, dy)
    acc_read(abuf, R, Cc, what)  # the consumers left the words and the flags alone
    # ---- one flag word set: every coefficient reads NaN
    av[R * 4 * Cc + R - 1] = 1
    f = fold_struct(acc, dgm, dbt, npix, 1e-5, torch.zeros(5 * Cc, device=DEV))
    for _ in range(2):  # (NaN outputs: not through twice(), which wants every element finite)
        cbuf, coef = guarded(5 * Cc, torch.float32)
        coef.zero_()
        f.coef = coef.data_ptr()
        _lib().call("cy_bn_fold_coef", C.byref(f), stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(coef).all()), f"{what}: a set flag word must turn every coefficient into NaN"
        coef.zero_()
        obuf, out = guarded(npix * Cc, dt)
        out.zero_()
        _lib().call("cy_bn_relu_apply_fold", dy_.data_ptr(), C.byref(f), out.data_ptr(), npix, code(dt), code(dt), stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(coef).all()), f"{what}: fold apply with a set flag"


# ================================================================ finalize kernels
def _partials(P, Cc, count, gen):
    """f32 partial rows [P][2][C] of sum x and sum x^2 over `count` values per channel.  With count < P (count = 1 at
    P > 1) every row still holds one value, on purpose: the launch is then told a count that is not the rows' own, the
    variance is whatever the clamp at zero leaves, and parity is against the float64 formula on the same rows -- what
    is exercised is the count = 1 arithmetic (no unbiasing), not a meaningful statistic"""
    x = torch.randn(max(count, P), Cc, generator=gen, dtype=torch.float64) * 1.5 + 0.7
    x = x[:count] if count >= P else x
    rows = torch.zeros(P, 2, Cc, dtype=torch.float64)
    idx = torch.arange(x.shape[0]) % P
    rows[:, 0].index_add_(0, idx, x)
    rows[:, 1].index_add_(0, idx, x * x)
    return rows.float()


@pytest.mark.parametrize("P", nc.FINALIZE_P)
def test_forward_finalize(P):
    Cc = nc.FINALIZE_C
    gen = torch.Generator().manual_seed(P)
    mom, eps = 0.1, 1e-5
    m64, e64 = float(torch.tensor(mom, dtype=torch.float32)), float(torch.tensor(eps, dtype=torch.float32))
    for count in (1, 4 * P + 3):
        part = _partials(P, Cc, count, gen)
        dpart = part.to(DEV)
        s = part.double().sum(0)
        for ubs in (0, 1):
            for upd in (0, 1):
                for null_gb in (False, True):
                    what = f"P{P} count={count} use_batch_stats={ubs} update_running={upd} null_gb={null_gb}"
                    gamma, beta = torch.rand(Cc, generator=gen) + 0.5, torch.randn(Cc, generator=gen)
                    rm, rv = torch.randn(Cc, generator=gen), torch.rand(Cc, generator=gen) + 0.5
                    dgm, dbt = gamma.to(DEV), beta.to(DEV)
                    rbuf = [guarded(Cc, torch.float32) for _ in range(2)]

                    def go(scale, shift, mean, invstd):
                        for (_, v), t in zip(rbuf, (rm, rv)):
                            v.copy_(t)
                        _lib().call("cy_bn_finalize", dpart.data_ptr(), P, Cc, float(count), None if null_gb else dgm.data_ptr(),
                                    None if null_gb else dbt.data_ptr(), rbuf[0][1].data_ptr(), rbuf[1][1].data_ptr(), mom, eps,
                                    ubs, upd, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(), stream())
                    got = torch.stack(twice(go, [(Cc, torch.float32)] * 4, what))
                    if ubs:
                        mean = s[0] / count
                        var = (s[1] / count - mean * mean).clamp_min(0)
                    else:
                        mean, var = rm.double(), rv.double()
                    istd = 1.0 / torch.sqrt(var + e64)
                    g = torch.ones(Cc, dtype=torch.float64) if null_gb else gamma.double()
                    b = torch.zeros(Cc, dtype=torch.float64) if null_gb else beta.double()
                    want = torch.stack([g * istd, b - mean * g * istd, mean, istd])
                    slack = 1e-12 * (1 + want.abs() + (mean * g * istd).abs())
                    assert_rounded_once(got, want, slack, "finalize", what)
                    run = torch.stack([rbuf[0][1], rbuf[1][1]])
                    for buf, _ in rbuf:
                        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + Cc:]).all())
                    if ubs and upd:
                        unb = var * count / (count - 1.0) if count > 1 else var
                        wr = torch.stack([(1.0 - m64) * rm.double() + m64 * mean, (1.0 - m64) * rv.double() + m64 * unb])
                        assert_rounded_once(run, wr, 1e-12 * (1 + wr.abs() + rm.abs().double()), "finalize running", what)
                    else:
                        assert torch.equal(run.cpu(), torch.stack([rm, rv])), f"{what}: running statistics touched"


@pytest.mark.parametrize("P", nc.BWD_FINALIZE_P)
def test_backward_finalize(P):
    Cc = nc.BWD_FINALIZE_C
    gen = torch.Generator().manual_seed(1000 + P)
    part = torch.randn(P, 2, Cc, generator=gen)
    dpart = part.to(DEV)
    t = part.double().sum(0)
    sc, _, mu, istd, _, _ = coefs(Cc, gen)
    dsc, dmu, dis = sc.to(DEV), mu.to(DEV), istd.to(DEV)
    for count in (1.0, 977.0):
        for bs in (0, 1):
            for accumulate in (0, 1):
                for null_grads in (False, True):
                    what = f"P{P} count={count} batch_stats={bs} accumulate={accumulate} null_grads={null_grads}"
                    old = torch.randn(2, Cc, generator=gen) * 20.0
                    gbuf = [guarded(Cc, torch.float32) for _ in range(2)]

                    def go(coef):
                        for (_, v), o in zip(gbuf, old):
                            v.copy_(o)
                        _lib().call("cy_bn_bwd_finalize", dpart.data_ptr(), P, Cc, dsc.data_ptr() if bs else None,
                                    dmu.data_ptr() if bs else None, dis.data_ptr() if bs else None, count, bs,
                                    None if null_grads else gbuf[0][1].data_ptr(), None if null_grads else gbuf[1][1].data_ptr(),
                                    accumulate, coef.data_ptr(), stream())
                    coef = twice(go, [(2 * Cc, torch.float32)], what)[0].view(2, Cc)
                    k1, k0 = bwd_fold_coefs(t[0], t[1], sc, mu, istd, count, bs, torch.float64)
                    slack = 1e-12 * (1 + (sc.double() * t[0] / count).abs() + (k1 * mu.double()).abs())
                    assert_rounded_once(coef, torch.stack([k1, k0]), slack, "bwd_finalize coefficients", what)
                    got = torch.stack([gbuf[0][1], gbuf[1][1]])
                    for buf, _ in gbuf:
                        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + Cc:]).all())
                    if null_grads:
                        assert torch.equal(got.cpu(), old), f"{what}: gradients written through null pointers' neighbours"
                        continue
                    base = old.double() if accumulate else torch.zeros(2, Cc, dtype=torch.float64)
                    want = torch.stack([base[0] + t[1].float().double(), base[1] + t[0].float().double()])
                    assert_rounded_once(got, want, 2.0 ** -24 * t.flip(0).abs(), "bwd_finalize dgamma dbeta", what)


def test_running_update_of_33_layers_in_two_launches():
    L, Cc = nc.RUNNING_LAYERS, nc.RUNNING_C
    gen = torch.Generator().manual_seed(33)
    coef = torch.randn(L, 5, Cc, generator=gen)
    coef[:, 4] = coef[:, 4].abs()
    rm, rv = torch.randn(L, Cc, generator=gen), torch.rand(L, Cc, generator=gen) + 0.5
    moms = [0.1 if i % 2 else 0.01 for i in range(L)]
    dcoef = coef.to(DEV)
    runs = []
    for _ in range(2):
        bufs = [(guarded(Cc, torch.float32), guarded(Cc, torch.float32)) for _ in range(L)]
        arr = (_lib().BnRunItem * L)()
        for i, (a, ((_, m), (_, v))) in enumerate(zip(arr, bufs)):
            m.copy_(rm[i]), v.copy_(rv[i])
            a.coef, a.running_mean, a.running_var, a.C, a.momentum = dcoef[i].data_ptr(), m.data_ptr(), v.data_ptr(), Cc, moms[i]
        _lib().call("cy_bn_running_update", arr, L, stream())
        torch.cuda.synchronize()
        for (bm, _), (bv, _) in bufs:
            for buf in (bm, bv):
                assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + Cc:]).all())
        runs.append(torch.stack([torch.stack([m, v]) for (_, m), (_, v) in bufs]).cpu())
    assert bits_equal(runs[0], runs[1])
    m64 = torch.tensor(moms, dtype=torch.float32).double()[:, None]
    want = torch.stack([(1.0 - m64) * rm.double() + m64 * coef[:, 2].double(),
                        (1.0 - m64) * rv.double() + m64 * coef[:, 4].double()], dim=1)
    assert_rounded_once(runs[0], want, 1e-12 * (1 + rm.abs().double()[:, None]), "running_update", "33 layers")
