"""Every host-side branch and every capped loop of the second backbone's kernels (csrc/cy_groupnorm.hip,
csrc/cy_unet2.hip) against the same operation in float64 on the CPU, written out in plain torch expressions on the
values the kernel actually reads (16-bit inputs are rounded to the storage type first).  The cases are the tables of
tests/unet2_cases.py; tests/test_unet2_plan_coverage.py proves on the CPU that they reach what they claim.

Every output and workspace buffer allocated here is filled with NaN before the call (padding columns with a sentinel
that must survive), no element is left out of a comparison, and every figure is printed before it is asserted.
Tolerances are relative to max|ref| and come from the case module."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import unet2_cases as uc

pytestmark = pytest.mark.gpu
DEV = "cuda"
TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CODE = {"f32": 0, "bf16": 1, "f16": 2}
NAN = float("nan")
SENTINEL = 512.0  # exact in every storage type
EPS = 1e-5


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a - b).abs().max().item(), b.abs().max().item()


def close(a, b, rel, what):
    err, m = rel_err(a, b)
    print(f"{what}: err {err:.3e}  max|ref| {m:.3e}  rel {err / (m + 1e-30):.3e}  bound {rel:.2e}")
    assert err <= rel * (m + 1e-30), f"{what}: {err:.3e} vs max {m:.3e} (bound {rel:.2e})"


def rel_only(a, b):
    err, m = rel_err(a, b)
    return err / (m + 1e-30)


def nan_buf(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def ws_buf(nbytes):
    return nan_buf(max((int(nbytes) + 3) // 4, 4))


def stream():
    from cyhip import ops
    return ops._stream()


def call(name, *args):
    from cyhip import _lib
    return _lib.call(name, *args)


def padded(payload, ld, fill):
    """[rows, C] -> device [rows, ld] with the payload in the first C columns and `fill` in the padding"""
    rows, Cc = payload.shape
    buf = torch.full((rows, ld), fill, dtype=payload.dtype, device=DEV)
    buf[:, :Cc] = payload.to(DEV)
    return buf


def out_buf(rows, Cc, ld, dtype):
    buf = torch.full((rows, ld), NAN, dtype=dtype, device=DEV)
    buf[:, Cc:] = SENTINEL
    return buf


def payload(buf, Cc, what):
    """the first C columns; the padding must still hold the sentinel"""
    assert bool((buf[:, Cc:] == SENTINEL).all()), f"{what}: padding columns were written"
    return buf[:, :Cc]


# ================================================================ GroupNorm + SiLU
def gn_inputs(c, dt, mod, seed, offset=False):
    g = torch.Generator().manual_seed(seed)
    N, HW, Cc = c.N, c.HW, c.C
    if c.fill == "const":
        y = torch.full((N * HW, Cc), 1.5)
        bias = torch.full((Cc,), 0.25)
    else:
        y = torch.randn(N * HW, Cc, generator=g)
        bias = 30.0 + 0.5 * torch.randn(Cc, generator=g) if offset else torch.randn(Cc, generator=g)
    inp = {"y": y.to(TD[dt]), "dz": torch.randn(N * HW, Cc, generator=g).to(TD[dt]), "bias": bias,
           "gamma": torch.rand(Cc, generator=g) + 0.5, "beta": torch.randn(Cc, generator=g), "ms": None, "mt": None}
    if mod:  # differs per image
        inp["ms"] = torch.randn(N, Cc, generator=g) * 0.5
        inp["mt"] = torch.randn(N, Cc, generator=g)
    return inp


def gn_reference(c, inp):
    """float64: u = y + bias, x^ = (u - mean_g) rstd_g, v = (gamma x^ + beta)(1 + s) + t, z = v sigmoid(v); and its adjoint"""
    N, HW, Cc, G = c.N, c.HW, c.C, c.G
    cg = Cc // G
    d = lambda t: t.double()  # noqa: E731
    u = (d(inp["y"]) + d(inp["bias"])).view(N, HW, G, cg)
    mean = u.mean(dim=(1, 3), keepdim=True)
    var = ((u - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    xh = ((u - mean) * rstd).reshape(N, HW, Cc)
    w = 1.0 + d(inp["ms"]) if inp["ms"] is not None else torch.ones(N, Cc, dtype=torch.float64)
    sh = d(inp["mt"]) if inp["mt"] is not None else torch.zeros(N, Cc, dtype=torch.float64)
    ge = (d(inp["gamma"]) * w).view(N, 1, Cc)
    be = (d(inp["beta"]) * w + sh).view(N, 1, Cc)
    v = xh * ge + be
    sg = torch.sigmoid(v)
    dv = d(inp["dz"]).view(N, HW, Cc) * (sg + v * sg * (1.0 - sg))
    dge, dbe = (dv * xh).sum(1), dv.sum(1)  # per image, of the effective gamma / beta
    dxh = (dv * ge).view(N, HW, G, cg)
    xg = xh.view(N, HW, G, cg)
    m1 = dxh.mean(dim=(1, 3), keepdim=True)
    m2 = (dxh * xg).mean(dim=(1, 3), keepdim=True)
    du = (rstd * (dxh - m1 - xg * m2)).reshape(N, HW, Cc)
    return {"out": (v * sg).reshape(N * HW, Cc), "mean_rstd": torch.stack((mean.view(N, G), rstd.view(N, G)), -1).reshape(-1),
            "du": du.reshape(N * HW, Cc), "dgamma": (w * dge).sum(0), "dbeta": (w * dbe).sum(0), "dbias": du.sum((0, 1)),
            "dms": d(inp["gamma"]) * dge + d(inp["beta"]) * dbe, "dmt": dbe}


def gn_run(c, dt, inp, *, strides=None, grads=(1, 1, 1), dmod=True, accumulate=False, init=None):
    """forward then backward through the entry points; returns the outputs (None where a null pointer was passed)"""
    from cyhip import _lib
    N, HW, Cc, G = c.N, c.HW, c.C, c.G
    st = {k: Cc + v for k, v in (strides or {k: 0 for k in uc.GN_STRIDES}).items()}
    mod = inp["ms"] is not None
    f = {k: inp[k].to(DEV).contiguous() for k in ("bias", "gamma", "beta")}
    ms, mt = (inp["ms"].to(DEV).contiguous(), inp["mt"].to(DEV).contiguous()) if mod else (None, None)
    y = padded(inp["y"], st["ldy"], NAN)
    dz = padded(inp["dz"], st["ldd"], NAN)
    out, du = out_buf(N * HW, Cc, st["ldo"], TD[dt]), out_buf(N * HW, Cc, st["ldu"], TD[dt])
    mr = nan_buf(N * G * 2)
    nbytes = _lib.load().cy_gn_ws_bytes(N, Cc)
    ws = ws_buf(nbytes)
    tail = (N, HW, Cc, G, EPS, CODE[dt], ws.data_ptr(), nbytes, stream())
    if mod:
        call("cy_gn_silu_mod_fwd", y.data_ptr(), st["ldy"], f["bias"].data_ptr(), f["gamma"].data_ptr(), f["beta"].data_ptr(),
             ms.data_ptr(), mt.data_ptr(), out.data_ptr(), st["ldo"], mr.data_ptr(), *tail)
    else:
        call("cy_gn_silu_fwd", y.data_ptr(), st["ldy"], f["bias"].data_ptr(), f["gamma"].data_ptr(), f["beta"].data_ptr(),
             out.data_ptr(), st["ldo"], mr.data_ptr(), *tail)
    res = {"out": payload(out, Cc, "out"), "mean_rstd": mr}
    init = init or {}
    pg = {}
    for k, on in zip(("dgamma", "dbeta", "dbias"), grads):
        pg[k] = (init[k].to(DEV).clone() if accumulate else nan_buf(Cc)) if on else None
    dms, dmt = (nan_buf(N, Cc), nan_buf(N, Cc)) if (mod and dmod) else (None, None)
    ws2 = ws_buf(nbytes)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    tail = (int(accumulate), N, HW, Cc, G, CODE[dt], ws2.data_ptr(), nbytes, stream())
    if mod:
        call("cy_gn_silu_mod_bwd", y.data_ptr(), st["ldy"], dz.data_ptr(), st["ldd"], f["bias"].data_ptr(),
             f["gamma"].data_ptr(), f["beta"].data_ptr(), ms.data_ptr(), mt.data_ptr(), mr.data_ptr(), du.data_ptr(), st["ldu"],
             ptr(pg["dgamma"]), ptr(pg["dbeta"]), ptr(pg["dbias"]), ptr(dms), ptr(dmt), *tail)
    else:
        call("cy_gn_silu_bwd", y.data_ptr(), st["ldy"], dz.data_ptr(), st["ldd"], f["bias"].data_ptr(), f["gamma"].data_ptr(),
             f["beta"].data_ptr(), mr.data_ptr(), du.data_ptr(), st["ldu"], ptr(pg["dgamma"]), ptr(pg["dbeta"]),
             ptr(pg["dbias"]), *tail)
    torch.cuda.synchronize()
    res.update(pg, du=payload(du, Cc, "du"), dms=dms, dmt=dmt)
    return res


def gn_check(c, dt, res, ref, what, *, init=None, bound=None):
    big = uc.ROUND[dt] + uc.TOL_GN  # out and du are stored in `dt`
    bound = bound or {}
    close(res["out"], ref["out"], bound.get("out", big), f"{what} out")
    close(res["mean_rstd"], ref["mean_rstd"], uc.TOL_GN, f"{what} mean/rstd")
    close(res["du"], ref["du"], bound.get("du", big), f"{what} du")
    for k in ("dgamma", "dbeta", "dbias"):  # f32 outputs
        if res[k] is None:
            continue
        want = ref[k] + (init[k].double() if init else 0.0)
        if k == "dbias" and c.C == c.G and not init:
            # one channel per group: du sums to zero over the group, so dbias is 0 by algebra and max|ref| is no scale.
            # The scale of a sum that cancels is the sum of the magnitudes it adds: sum over (n, pixel) of |du|
            scale = ref["du"].abs().sum(0).max().item()
            err = rel_err(res[k], want)[0]
            print(f"{what} dbias (cancels to zero): err {err:.3e}  sum|du| {scale:.3e}  bound {uc.TOL_GN:.2e}")
            assert err <= uc.TOL_GN * scale, f"{what} dbias: {err:.3e} vs sum|du| {scale:.3e}"
            continue
        close(res[k], want, uc.TOL_GN, f"{what} {k}")
    for k, r in (("dms", "dms"), ("dmt", "dmt")):
        if res[k] is not None:
            close(res[k], ref[r], uc.TOL_GN, f"{what} {k}")


@pytest.mark.parametrize("dt", uc.TYPES)
@pytest.mark.parametrize("c", uc.GN_SHAPES, ids=uc.ident)
def test_groupnorm_shapes(c, dt):
    for mod in (False, True):
        inp = gn_inputs(c, dt, mod, seed=10 + mod)
        gn_check(c, dt, gn_run(c, dt, inp), gn_reference(c, inp), f"{c.name} {dt} mod={int(mod)}")


@pytest.mark.parametrize("dt", uc.TYPES)
def test_groupnorm_strided_rows_nan_padding_and_sentinels(dt):
    c = uc.GN_STRIDED
    for mod in (False, True):
        inp = gn_inputs(c, dt, mod, seed=20 + mod)
        res = gn_run(c, dt, inp, strides=uc.GN_STRIDES)  # payload() asserts the sentinels
        gn_check(c, dt, res, gn_reference(c, inp), f"strided {dt} mod={int(mod)}")


@pytest.mark.parametrize("grads", uc.GN_NULL_SETS, ids=lambda s: "".join(map(str, s)))
def test_groupnorm_gradient_outputs_accumulate_and_null(grads):
    c = uc.GN_GRADS
    g = torch.Generator().manual_seed(30)
    init = {k: torch.randn(c.C, generator=g) * 3 for k in ("dgamma", "dbeta", "dbias")}
    for mod, dmod in ((False, False), (True, True), (True, False)):
        inp = gn_inputs(c, "f32", mod, seed=31 + mod)
        ref = gn_reference(c, inp)
        for acc in (False, True):
            res = gn_run(c, "f32", inp, grads=grads, dmod=dmod, accumulate=acc, init=init)
            assert all((res[k] is None) == (not on) for k, on in zip(("dgamma", "dbeta", "dbias"), grads))
            assert (res["dms"] is None) == (not dmod)
            gn_check(c, "f32", res, ref, f"grads {grads} mod={int(mod)} dmod={int(dmod)} acc={int(acc)}",
                     init=init if acc else None)


def test_groupnorm_past_the_apply_grid_cap_bf16():
    c = uc.GN_CAP
    inp = gn_inputs(c, "bf16", False, seed=40)
    gn_check(c, "bf16", gn_run(c, "bf16", inp), gn_reference(c, inp), "past the apply cap bf16")


def gn_offset_case():
    c = uc.GN_OFFSET
    return c, gn_inputs(c, "f32", False, seed=50, offset=True)


def yardstick_gn_offset():
    """torch's own f32 CPU GroupNorm + SiLU (forward, and autograd for du) against the float64 reference"""
    c, inp = gn_offset_case()
    ref = gn_reference(c, inp)
    y = inp["y"].view(c.N, c.HW, c.C).permute(0, 2, 1).contiguous().requires_grad_(True)
    out = F.silu(F.group_norm(y + inp["bias"].view(1, -1, 1), c.G, inp["gamma"], inp["beta"], EPS))
    out.backward(inp["dz"].view(c.N, c.HW, c.C).permute(0, 2, 1))
    back = lambda t: t.detach().permute(0, 2, 1).reshape(c.N * c.HW, c.C)  # noqa: E731
    return {"out": rel_only(back(out), ref["out"]), "du": rel_only(back(y.grad), ref["du"])}


def test_groupnorm_mean_thirty_sigma_from_zero():
    c, inp = gn_offset_case()
    gn_check(c, "f32", gn_run(c, "f32", inp), gn_reference(c, inp), "offset 30 sigma", bound=uc.GN_OFFSET_BOUND)


# ================================================================ strided GEMM
def layout(t):
    from cyhip._lib import MatLayout
    return MatLayout(*t)


def gemm_logical(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)


def gemm_operands(variant, M, N, K, seed):
    A, B = gemm_logical(M, N, K, seed)
    la, lb, sa, sb = uc.gemm_layouts(variant, M, N, K)
    As = torch.full(sa, NAN)
    if uc.GEMM_VARIANTS[variant][0]:
        As[:, :M] = A.t()
    else:
        As = A.clone()
    Bs = B.clone() if uc.GEMM_VARIANTS[variant][1] else B.t().contiguous()
    return A, B, As.to(DEV), Bs.to(DEV), la, lb


def gemm_once(variant, M, N, K, seed, ksplit):
    from cyhip.glue import gemm
    A, B, As, Bs, la, lb = gemm_operands(variant, M, N, K, seed)
    Cd = nan_buf(M, N)
    gemm((As, 0), layout(la), (Bs, 0), layout(lb), (Cd, 0), layout((N, 1, 0, 0)), M, N, K, ksplit=ksplit)
    return Cd, A.double() @ B.double()


@pytest.mark.parametrize("variant", sorted(uc.GEMM_VARIANTS))
def test_gemm_every_loader_variant_at_ragged_exact_and_tiny_sizes(variant):
    for M, N, K in uc.GEMM_SIZES:
        Cd, ref = gemm_once(variant, M, N, K, seed=60, ksplit=1)
        close(Cd, ref, uc.TOL_GEMM_FWD, f"gemm {variant} {M}x{N}x{K}")
    M, N, K = uc.GEMM_LONG  # automatic split-K
    outs = [gemm_once(variant, M, N, K, seed=61, ksplit=None) for _ in range(2)]
    close(outs[0][0], outs[0][1], uc.GEMM_LONG_BOUND, f"gemm {variant} {M}x{N}x{K} auto split")
    assert torch.equal(outs[0][0], outs[1][0]), "split-K is not bit-identical between two runs"


def yardstick_gemm_long():
    M, N, K = uc.GEMM_LONG
    A, B = gemm_logical(M, N, K, 61)
    return rel_only(A @ B, A.double() @ B.double())


@pytest.mark.parametrize("c", uc.GEMM_SPLITS, ids=uc.ident)
def test_gemm_split_k_partial_and_empty_last_split(c):
    outs = [gemm_once(c.variant, c.M, c.N, c.K, seed=62, ksplit=c.ksplit) for _ in range(2)]
    close(outs[0][0], outs[0][1], uc.TOL_GEMM_FWD, f"gemm {c.name}")
    assert torch.equal(outs[0][0], outs[1][0]), "split-K is not bit-identical between two runs"


def test_gemm_split_k_with_bias_alpha_accumulate_batches_into_a_column_slice():
    from cyhip.glue import gemm
    p = uc.GEMM_COMBINED
    nb1, nb2, M, N, K = p["nb1"], p["nb2"], p["M"], p["N"], p["K"]
    ldx, ldc = p["a_off"] + nb2 * K + p["a_pad"], p["ldc"]
    g = torch.Generator().manual_seed(63)
    X = torch.randn(nb1 * M, ldx, generator=g)
    Wm = torch.randn(nb1, nb2, K, N, generator=g)
    bias = torch.randn(N, generator=g)
    C0 = torch.randn(nb1 * M, ldc, generator=g)
    ref = C0.double().view(nb1, M, ldc).clone()
    for b in range(nb1):
        for h in range(nb2):
            a = X.view(nb1, M, ldx)[b, :, p["a_off"] + h * K: p["a_off"] + (h + 1) * K].double()
            ref[b, :, p["c_off"] + h * N: p["c_off"] + (h + 1) * N] += p["alpha"] * (a @ Wm[b, h].double()) + bias.double()
    outs = []
    for _ in range(2):
        Cd = C0.to(DEV)
        gemm((X.to(DEV), p["a_off"]), layout((ldx, 1, M * ldx, K)), (Wm.to(DEV), 0), layout((N, 1, nb2 * K * N, K * N)),
             (Cd, p["c_off"]), layout((ldc, 1, M * ldc, N)), M, N, K, bias=bias.to(DEV), nb1=nb1, nb2=nb2,
             alpha=p["alpha"], accumulate=True, ksplit=p["ksplit"])
        outs.append(Cd)
    close(outs[0], ref.view(-1, ldc), uc.TOL_GEMM_FWD, "gemm split-K + bias + alpha + accumulate + batches")
    assert torch.equal(outs[0], outs[1])
    untouched = [j for j in range(ldc) if not p["c_off"] <= j < p["c_off"] + nb2 * N]
    assert torch.equal(outs[0].cpu()[:, untouched], C0[:, untouched]), "columns outside the slice were written"


# ================================================================ im2col / col2im
def unfold_rows(x_nhwc, g):
    """F.unfold of the same map, reordered to rows (n, ho, wo) x columns (kh, kw, c)"""
    N, H, W, Cc = x_nhwc.shape
    Ho, Wo = uc.conv_out(g)
    u = F.unfold(x_nhwc.permute(0, 3, 1, 2), g.K, padding=g.pad, stride=g.stride)
    return u.view(N, Cc, g.K, g.K, Ho, Wo).permute(0, 4, 5, 2, 3, 1).reshape(N * Ho * Wo, g.K * g.K * Cc)


@pytest.mark.parametrize("g", (uc.IM2COL_CAP,) + uc.CONV_RAGGED, ids=uc.ident)
def test_im2col_equals_unfold_bit_for_bit(g):
    gen = torch.Generator().manual_seed(70)
    x = torch.randn(g.N, g.H, g.W, g.C, generator=gen)
    Ho, Wo = uc.conv_out(g)
    cols = nan_buf(g.N * Ho * Wo, g.K * g.K * g.C)
    xd = x.to(DEV)
    call("cy_im2col", xd.data_ptr(), cols.data_ptr(), g.N, g.H, g.W, g.C, g.K, g.K, g.stride, g.pad, stream())
    assert torch.equal(cols.cpu(), unfold_rows(x, g)), f"im2col {g.name} differs from F.unfold"


@pytest.mark.parametrize("g", (uc.COL2IM_CAP,) + uc.CONV_RAGGED, ids=uc.ident)
def test_col2im_is_the_adjoint_fold(g):
    gen = torch.Generator().manual_seed(71)
    Ho, Wo = uc.conv_out(g)
    cols = torch.randn(g.N * Ho * Wo, g.K * g.K * g.C, generator=gen)
    bias = torch.randn(g.C, generator=gen)
    out, cd, bd = nan_buf(g.N, g.H, g.W, g.C), cols.to(DEV), bias.to(DEV)
    call("cy_col2im", cd.data_ptr(), bd.data_ptr(), out.data_ptr(), g.N, g.H, g.W, g.C, g.K, g.K,
         g.stride, g.pad, stream())
    patches = cols.double().view(g.N, Ho, Wo, g.K, g.K, g.C).permute(0, 5, 3, 4, 1, 2)  # F.fold wants (c, kh, kw) x positions
    folded = F.fold(patches.reshape(g.N, g.C * g.K * g.K, Ho * Wo),
                    (g.H, g.W), g.K, padding=g.pad, stride=g.stride)
    close(out, folded.permute(0, 2, 3, 1) + bias.double(), uc.TOL_GEMM_FWD, f"col2im {g.name}")


def test_conv2d_past_the_im2col_cap_then_ragged_geometries():
    from cyhip.glue import Conv2dFn
    gen = torch.Generator().manual_seed(72)
    g = uc.IM2COL_CAP  # the cap-sized case first: forward (im2col + GEMM)
    x = torch.randn(g.N, g.C, g.H, g.W, generator=gen)
    w = torch.randn(g.Cout, g.C, g.K, g.K, generator=gen) * 0.2
    b = torch.randn(g.Cout, generator=gen)
    with torch.no_grad():
        y = Conv2dFn.apply(x.to(DEV), w.to(DEV), b.to(DEV), g.stride, g.pad)
    close(y, F.conv2d(x.double(), w.double(), b.double(), g.stride, g.pad), uc.TOL_GEMM_FWD, "conv past the im2col cap")
    for g in uc.CONV_RAGGED:
        x = torch.randn(g.N, g.C, g.H, g.W, generator=gen).double().requires_grad_(True)
        w = (torch.randn(g.Cout, g.C, g.K, g.K, generator=gen) * 0.2).double().requires_grad_(True)
        b = torch.randn(g.Cout, generator=gen).double().requires_grad_(True)
        y_ref = F.conv2d(x, w, b, g.stride, g.pad)
        dy = torch.randn(y_ref.shape, generator=gen)
        (y_ref * dy.double()).sum().backward()
        xd, wd, bd = (t.detach().float().to(DEV).requires_grad_(True) for t in (x, w, b))
        y = Conv2dFn.apply(xd, wd, bd, g.stride, g.pad)
        assert tuple(y.shape) == tuple(y_ref.shape)
        close(y, y_ref, uc.TOL_GEMM_FWD, f"conv {g.name} fwd")
        (y * dy.to(DEV)).sum().backward()
        close(xd.grad, x.grad, uc.TOL_GEMM_GRAD, f"conv {g.name} dx")
        close(wd.grad, w.grad, uc.TOL_GEMM_GRAD, f"conv {g.name} dw")
        close(bd.grad, b.grad, uc.TOL_GEMM_GRAD, f"conv {g.name} db")
        Ho, Wo = uc.conv_out(g)
        # the first row / column that no window reaches
        last_h, last_w = (Ho - 1) * g.stride - g.pad + g.K, (Wo - 1) * g.stride - g.pad + g.K
        if last_h < g.H:
            assert bool((xd.grad[:, :, last_h:, :] == 0).all()), f"{g.name}: dx of the unused rows"
        if last_w < g.W:
            assert bool((xd.grad[:, :, :, last_w:] == 0).all()), f"{g.name}: dx of the unused columns"


@pytest.mark.parametrize("g", uc.CONVT_CASES, ids=uc.ident)
def test_conv_transpose2d_against_float64(g):
    from cyhip.glue import ConvTranspose2dFn
    gen = torch.Generator().manual_seed(73)
    x = torch.randn(g.N, g.C, g.H, g.W, generator=gen).double().requires_grad_(True)
    w = (torch.randn(g.C, g.Cout, g.K, g.K, generator=gen) * 0.2).double().requires_grad_(True)
    b = torch.randn(g.Cout, generator=gen).double().requires_grad_(True)
    y_ref = F.conv_transpose2d(x, w, b, g.stride, g.pad)
    dy = torch.randn(y_ref.shape, generator=gen)
    (y_ref * dy.double()).sum().backward()
    xd, wd, bd = (t.detach().float().to(DEV).requires_grad_(True) for t in (x, w, b))
    y = ConvTranspose2dFn.apply(xd, wd, bd, g.stride, g.pad)
    close(y, y_ref, uc.TOL_GEMM_FWD, "convT fwd")
    (y * dy.to(DEV)).sum().backward()
    close(xd.grad, x.grad, uc.TOL_GEMM_GRAD, "convT dx")
    close(wd.grad, w.grad, uc.TOL_GEMM_GRAD, "convT dw")
    close(bd.grad, b.grad, uc.TOL_GEMM_GRAD, "convT db")


# ================================================================ column sums, channel LayerNorm
def rows_input(c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(c.M, c.N, generator=g) * 2 + 0.5, g


@pytest.mark.parametrize("c", uc.ROWS_CASES, ids=uc.ident)
def test_colsum_slices_and_accumulate(c):
    from cyhip import _lib
    x, g = rows_input(c, 80)
    c0 = torch.randn(c.N, generator=g) * 5
    nbytes = _lib.load().cy_colsum_ws_bytes(c.M, c.N)
    tol = uc.COLSUM_LONG_BOUND if c.M >= uc.LONG_M else uc.TOL_GEMM_GRAD
    xd = x.to(DEV)
    for acc in (0, 1):
        out = c0.to(DEV) if acc else nan_buf(c.N)
        ws = ws_buf(nbytes)
        call("cy_colsum", xd.data_ptr(), out.data_ptr(), c.M, c.N, acc, ws.data_ptr(), nbytes, stream())
        close(out, x.double().sum(0) + (c0.double() if acc else 0.0), tol, f"colsum {c.M}x{c.N} accumulate={acc}")


def yardstick_colsum_long():
    x, _ = rows_input(uc.RowsCase(uc.LONG_M, 8), 80)
    return rel_only(x.sum(0), x.double().sum(0))


def ln_reference(x, gam, bet, dy):
    x, gam, bet, dy = (t.double() for t in (x, gam, bet, dy))
    mu = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + EPS)
    xh = (x - mu) * rstd
    t = dy * gam
    dx = rstd * (t - t.mean(1, keepdim=True) - xh * (t * xh).mean(1, keepdim=True))
    return xh * gam + bet, dx, (dy * xh).sum(0), dy.sum(0)


def ln_inputs(c):
    x, g = rows_input(c, 81)
    return x, torch.randn(c.N, generator=g) + 1, torch.randn(c.N, generator=g), torch.randn(c.M, c.N, generator=g)


@pytest.mark.parametrize("c", uc.ROWS_CASES, ids=uc.ident)
def test_chan_layernorm_slices_one_channel_and_null_parameter_gradients(c):
    from cyhip import _lib
    M, Cc = c
    x, gam, bet, dy = ln_inputs(c)
    y_ref, dx_ref, dg_ref, db_ref = ln_reference(x, gam, bet, dy)
    xd, gd, bd, dyd = (t.to(DEV) for t in (x, gam, bet, dy))
    y = nan_buf(M, Cc)
    call("cy_chan_layernorm_fwd", xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), M, Cc, EPS, stream())
    close(y, y_ref, uc.TOL_GEMM_FWD, f"LN {M}x{Cc} y")
    tol = uc.LN_LONG_BOUND if M >= uc.LONG_M else uc.TOL_LN
    nbytes = _lib.load().cy_chan_layernorm_bwd_ws_bytes(M, Cc)
    for with_params in (True, False):
        dx, dg, db, ws = nan_buf(M, Cc), nan_buf(Cc), nan_buf(Cc), ws_buf(nbytes)
        call("cy_chan_layernorm_bwd", xd.data_ptr(), gd.data_ptr(), dyd.data_ptr(), dx.data_ptr(),
             dg.data_ptr() if with_params else None, db.data_ptr() if with_params else None, M, Cc, EPS, ws.data_ptr(),
             nbytes, stream())
        close(dx, dx_ref, tol, f"LN {M}x{Cc} dx params={int(with_params)}")
        if with_params:
            close(dg, dg_ref, tol, f"LN {M}x{Cc} dg")
            close(db, db_ref, tol, f"LN {M}x{Cc} db")


def yardstick_ln_long():
    x, gam, bet, dy = ln_inputs(uc.RowsCase(uc.LONG_M, 8))
    y_ref, dx_ref, dg_ref, db_ref = ln_reference(x, gam, bet, dy)
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gam, bet))
    y = F.layer_norm(xr, (8,), gr, br, EPS)
    y.backward(dy)
    return {"y": rel_only(y, y_ref), "dx": rel_only(xr.grad, dx_ref), "dg": rel_only(gr.grad, dg_ref),
            "db": rel_only(br.grad, db_ref)}


# ================================================================ softmaxes
@pytest.mark.parametrize("c", uc.HEAD_CASES, ids=uc.ident)
def test_head_softmax_offset_padding_wide_logits(c):
    g = torch.Generator().manual_seed(90)
    hid, scale = c.heads * c.dh, c.dh ** -0.5
    logits = (torch.rand(c.M, hid, generator=g) * 2 - 1) * 80
    x = torch.full((c.M, c.ld), NAN)
    x[:, c.off: c.off + hid] = logits
    y, xd = nan_buf(c.M, hid), x.to(DEV)
    call("cy_head_softmax_fwd", xd.data_ptr(), c.ld, c.off, y.data_ptr(), c.M, c.heads, c.dh, scale, stream())
    P = logits.double().view(c.M, c.heads, c.dh).softmax(-1)
    close(y, (P * scale).view(c.M, hid), uc.TOL_SOFTMAX, f"head softmax {c.name} fwd")
    # backward on the f32 output of the forward formula: dx = y (dy - sum_d P dy), into rows of ld at column off
    yf = (P * scale).view(c.M, hid).float()
    dy = torch.randn(c.M, hid, generator=g)
    dx = nan_buf(c.M, c.ld)
    dx[:, : c.off] = SENTINEL
    dx[:, c.off + hid:] = SENTINEL
    yd, dyd = yf.to(DEV), dy.to(DEV)
    call("cy_head_softmax_bwd", yd.data_ptr(), dyd.data_ptr(), dx.data_ptr(), c.ld, c.off, c.M, c.heads,
         c.dh, scale, stream())
    y3, d3 = yf.double().view(c.M, c.heads, c.dh), dy.double().view(c.M, c.heads, c.dh)
    ref = y3 * (d3 - (y3 / scale * d3).sum(-1, keepdim=True))
    dxc = dx.cpu()
    assert bool((dxc[:, : c.off] == SENTINEL).all() and (dxc[:, c.off + hid:] == SENTINEL).all()), "padding written"
    close(dxc[:, c.off: c.off + hid], ref.view(c.M, hid), uc.TOL_SOFTMAX, f"head softmax {c.name} bwd")


def col_inputs(c, seed=91):
    """logits in (-1, 1); channel c has its maximum (+3) at the first position when c is even, at the last when odd"""
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(c.B, c.n, c.Ch, generator=g) * 2 - 1
    v[:, 0, 0::2] += 3.0
    v[:, c.n - 1, 1::2] += 3.0
    return v, g


@pytest.mark.parametrize("c", uc.COL_CASES, ids=uc.ident)
def test_col_softmax_slices_caps_and_maximum_in_first_or_last_slice(c):
    from cyhip import _lib
    v, g = col_inputs(c)
    x = torch.full((c.B * c.n, c.ld), NAN)
    x[:, c.off: c.off + c.Ch] = v.view(-1, c.Ch)
    nbytes = _lib.load().cy_col_softmax_ws_bytes(c.B, c.n, c.Ch)
    y, ws, xd = nan_buf(c.B * c.n, c.Ch), ws_buf(nbytes), x.to(DEV)
    call("cy_col_softmax_fwd", xd.data_ptr(), c.ld, c.off, y.data_ptr(), c.B, c.n, c.Ch, ws.data_ptr(), nbytes,
         stream())
    ref = v.double().softmax(1)
    tol = uc.COL_LONG_BOUND if c.n > 32768 else uc.TOL_SOFTMAX
    close(y, ref.view(-1, c.Ch), tol, f"col softmax {c.name} fwd")
    yf = ref.float()
    dy, t = torch.randn(c.B, c.n, c.Ch, generator=g), torch.randn(c.B, c.Ch, generator=g)
    dx = nan_buf(c.B * c.n, c.ld)
    dx[:, : c.off] = SENTINEL
    dx[:, c.off + c.Ch:] = SENTINEL
    yd, dyd, td = yf.to(DEV), dy.to(DEV), t.to(DEV)
    call("cy_col_softmax_bwd", yd.data_ptr(), dyd.data_ptr(), td.data_ptr(), dx.data_ptr(), c.ld,
         c.off, c.B, c.n, c.Ch, stream())
    dxc = dx.cpu()
    assert bool((dxc[:, : c.off] == SENTINEL).all() and (dxc[:, c.off + c.Ch:] == SENTINEL).all()), "padding written"
    want = yf.double() * (dy.double() - t.double().view(c.B, 1, c.Ch))
    close(dxc[:, c.off: c.off + c.Ch], want.view(-1, c.Ch), uc.TOL_SOFTMAX, f"col softmax {c.name} bwd")


def yardstick_col_long():
    v, _ = col_inputs(uc.COL_CASES[0])
    return rel_only(v.softmax(1), v.double().softmax(1))


@pytest.mark.parametrize("n", uc.ROW_N)
def test_row_softmax_strided_loop(n):
    g = torch.Generator().manual_seed(92)
    rows = uc.ROW_ROWS
    x = torch.randn(rows, n, generator=g) * 3
    xd = x.to(DEV)
    call("cy_row_softmax_fwd", xd.data_ptr(), rows, n, stream())
    P = x.double().softmax(-1)
    close(xd, P, uc.TOL_SOFTMAX, f"row softmax n={n} fwd")
    pf, dp = P.float(), torch.randn(rows, n, generator=g)
    dd, pd = dp.to(DEV), pf.to(DEV)
    call("cy_row_softmax_bwd", pd.data_ptr(), dd.data_ptr(), rows, n, stream())
    want = pf.double() * (dp.double() - (pf.double() * dp.double()).sum(-1, keepdim=True))
    close(dd, want, uc.TOL_SOFTMAX, f"row softmax n={n} bwd")


def _heads(t, heads):
    b, ch, h, w = t.shape
    return t.reshape(b, heads, ch // heads, h * w)


def linattn_expr(qkv, heads, dh):
    b, _, H, W = qkv.shape
    q, k, v = (_heads(t, heads) for t in qkv.chunk(3, dim=1))
    q = q.softmax(dim=-2) * dh ** -0.5
    k = k.softmax(dim=-1)
    context = torch.einsum("bhdn,bhen->bhde", k, v)
    return torch.einsum("bhde,bhdn->bhen", context, q).reshape(b, heads * dh, H, W)


def linattn_inputs():
    p = uc.LINATTN_LONG
    g = torch.Generator().manual_seed(93)
    qkv = torch.randn(p["N"], 3 * p["heads"] * p["dh"], p["H"], p["W"], generator=g)
    return p, qkv, torch.randn(p["N"], p["heads"] * p["dh"], p["H"], p["W"], generator=g)


def linattn_cpu(qkv, dy, p):
    q = qkv.clone().requires_grad_(True)
    out = linattn_expr(q, p["heads"], p["dh"])
    (out * dy.to(out.dtype)).sum().backward()
    return out.detach(), q.grad


def test_linear_attention_past_32768_positions():
    from cyhip.glue import LinearAttentionFn
    p, qkv, dy = linattn_inputs()
    out_ref, dq_ref = linattn_cpu(qkv.double(), dy, p)
    qd = qkv.to(DEV).requires_grad_(True)
    out = LinearAttentionFn.apply(qd, p["heads"], p["dh"], p["dh"] ** -0.5)
    close(out, out_ref, uc.LINATTN_LONG_BOUND["out"], "linear attention 182x181 fwd")
    (out * dy.to(DEV)).sum().backward()
    close(qd.grad, dq_ref, uc.LINATTN_LONG_BOUND["dqkv"], "linear attention 182x181 dqkv")


def yardstick_linattn_long():
    p, qkv, dy = linattn_inputs()
    out_ref, dq_ref = linattn_cpu(qkv.double(), dy, p)
    out, dq = linattn_cpu(qkv, dy, p)
    return {"out": rel_only(out, out_ref), "dqkv": rel_only(dq, dq_ref)}


def test_softmax_attention_at_784_positions():
    from cyhip.glue import AttentionFn
    p = uc.ATTN_784
    heads, dh = p["heads"], p["dh"]
    g = torch.Generator().manual_seed(94)
    qkv = torch.randn(p["N"], 3 * heads * dh, p["H"], p["W"], generator=g)
    dy = torch.randn(p["N"], heads * dh, p["H"], p["W"], generator=g)
    qr = qkv.double().requires_grad_(True)
    q, k, v = (_heads(t, heads) for t in qr.chunk(3, dim=1))
    attn = torch.einsum("bhdi,bhdj->bhij", q * dh ** -0.5, k).softmax(dim=-1)
    out_ref = torch.einsum("bhij,bhdj->bhid", attn, v).transpose(-1, -2).reshape(p["N"], heads * dh, p["H"], p["W"])
    (out_ref * dy.double()).sum().backward()
    qd = qkv.to(DEV).requires_grad_(True)
    out = AttentionFn.apply(qd, heads, dh, dh ** -0.5)
    close(out, out_ref, uc.TOL_SOFTMAX, "attention 28x28 fwd")
    (out * dy.to(DEV)).sum().backward()
    close(qd.grad, qr.grad, uc.TOL_ATTN_GRAD, "attention 28x28 dqkv")


# ================================================================ activations, embedding, bilinear
@pytest.mark.parametrize("kind", uc.ACT_KINDS)
def test_activation_past_the_grid_cap_over_plus_minus_20(kind):
    g = torch.Generator().manual_seed(100)
    n = uc.ACT_N
    x = (torch.rand(n, generator=g) * 2 - 1) * 20
    x[0], x[1], x[2] = -20.0, 20.0, 0.0
    dy = torch.randn(n, generator=g)
    xd, dyd, y, dx = x.to(DEV), dy.to(DEV), nan_buf(n), nan_buf(n)
    call("cy_act_fwd", xd.data_ptr(), y.data_ptr(), n, kind, stream())
    call("cy_act_bwd", xd.data_ptr(), dyd.data_ptr(), dx.data_ptr(), n, kind, stream())
    xx = x.double()
    if kind == 0:
        s = torch.sigmoid(xx)
        f, df = xx * s, s * (1 + xx * (1 - s))
    else:
        phi = 0.5 * (1 + torch.erf(xx / math.sqrt(2.0)))
        f, df = xx * phi, phi + xx * torch.exp(-0.5 * xx * xx) / math.sqrt(2.0 * math.pi)
    close(y, f, uc.TOL_ACT, f"act kind {kind} fwd")
    close(dx, dy.double() * df, uc.TOL_ACT, f"act kind {kind} bwd")


@pytest.mark.parametrize("c", uc.EMB_CASES, ids=uc.ident)
def test_sinusoidal_embedding_within_argument_rounding(c):
    """|out - ref| <= 2 * 2^-24 * |t e_i| + 4e-7: the two f32 roundings of the argument (e_i, then t e_i) plus a few ulp of
    sin / cos.  With e_i computed in f32 (three roundings of an exponent of up to 9.2) the kernel was at 2.14 x this bound
    at dim = 128 (4.96e-5 absolute); with e_i rounded once from double it is at 0.62 x (dim 4: 0.08, dim 6: 0.47)."""
    g = torch.Generator().manual_seed(101)
    t = torch.rand(c.B, generator=g) * uc.EMB_T_MAX
    t[0], t[1] = uc.EMB_T_MAX, 0.0
    out, td = nan_buf(c.B, c.dim), t.to(DEV)
    call("cy_sinusoidal_emb", td.data_ptr(), out.data_ptr(), c.B, c.dim, stream())
    half = c.dim // 2
    e = torch.exp(torch.arange(half, dtype=torch.float64) * -(math.log(10000.0) / (half - 1)))
    arg = t.double()[:, None] * e[None]
    ref = torch.cat((arg.sin(), arg.cos()), dim=-1)
    bound = torch.cat((arg.abs(), arg.abs()), dim=-1) * 2.0 * 2.0 ** -24 + 4e-7
    excess = ((out.double().cpu() - ref).abs() / bound).max().item()
    print(f"sinusoidal B={c.B} dim={c.dim}: largest |err| / bound = {excess:.3f}, "
          f"largest |err| = {(out.double().cpu() - ref).abs().max().item():.3e}")
    assert excess <= 1.0, f"sinusoidal dim={c.dim}: error is {excess:.2f} x the bound"


def bilinear_bound(c, dt):
    """one rounding of the output to the storage type (its unit roundoff); the source coordinate (o + 0.5) * (H / h) - 0.5
    carries two f32 roundings (2 * 2^-24 relative, of a coordinate up to max(H, W)) and moves an interpolation weight by
    as much, a weight that multiplies a difference of two neighbours (at most 2 max|x|); plus the project's 1e-6"""
    return uc.ROUND[dt] + 2 * 2.0 ** -24 * max(c.H, c.W) * 2 + 1e-6


@pytest.mark.parametrize("dt", uc.TYPES)
def test_bilinear_non_integer_ratios_and_past_the_cap(dt):
    g = torch.Generator().manual_seed(102)
    for c in uc.BILINEAR_CASES:
        if c.name == "past-cap" and dt not in uc.BILINEAR_BIG_TYPES:
            continue
        x = torch.randn(c.N, c.H, c.W, c.C, generator=g).to(TD[dt])
        out = nan_buf(c.N, c.h, c.w, c.C, dtype=TD[dt])
        xd = x.to(DEV)
        call("cy_bilinear_fwd", xd.data_ptr(), out.data_ptr(), c.N, c.H, c.W, c.C, c.h, c.w, CODE[dt], stream())
        ref = F.interpolate(x.double().permute(0, 3, 1, 2), size=(c.h, c.w), mode="bilinear", align_corners=False)
        close(out, ref.permute(0, 2, 3, 1), bilinear_bound(c, dt), f"bilinear {c.name} {dt}")
