"""Parity of csrc/cy_contrast.hip and csrc/cy_proj_head.hip on every branch and past every cap: cy_sgemm, the InfoNCE /
SupCon loss on its three paths (materialised similarity matrix, fused, exclude_other_pos) with labels and with the
reference's general mask -- 1 positive, 0 negative, anything else neither, never transposed -- (cy_contrast.hip); the
projector pieces (average pool, linear, L2 normalise) and the one-launch projection head (cy_proj_head.hip).  The cases
are those of tests/contrast_cases.py;
tests/test_contrast_plan_coverage.py checks on the CPU that they reach every branch and cap, and the rejections.

Reference: the same operation in float64, torch on the CPU or the oracle, with autograd, on inputs already rounded to
the storage type; for the mask cases of tests/golden/supcon_masks.npz the reference's own vectors.  The entry points are
called through the binding with buffers of this file: every output, scratch matrix and workspace is filled with NaN
before the call, so an element a kernel leaves unwritten fails its comparison.  Tolerances (contrast_cases.py) are on
max|got - ref| <= tol * max|ref| over the whole tensor."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import contrast_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
NAN = float("nan")


def _ops():
    from cyhip import ops
    return ops


def lib_call(name, *args):
    from cyhip import _lib
    return _lib.call(name, *args)


def stream():
    return _ops()._stream()


def ptr(t):
    return None if t is None else t.data_ptr()


def nanf(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def gpu(t, dtype=torch.float32):
    return t.to(dtype).to(DEV).contiguous()


def rnd(*shape, gen):
    return torch.rand(*shape, generator=gen, dtype=torch.float64) * 2 - 1


def check(got, ref, tol, what, rows=None, floor=0.0):
    """max|got - ref| <= tol * max|ref| over the whole tensor (+ floor: only where contrast_cases.py derives one);
    rows=[scale per row]: row by row, each against the larger of its own maximum and that scale"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} elements not finite (unwritten?)"
    if rows is not None:
        err, scale = (got - ref).abs().amax(dim=1), torch.maximum(ref.abs().amax(dim=1), rows)
        print(f"{what}: worst row err/scale {(err / scale.clamp_min(1e-300)).max().item():.3e}, tol {tol:.1e}")
        assert bool((err <= tol * scale).all()), f"{what}: row-wise err {err.tolist()} vs {tol:.1e} * {scale.tolist()}"
        return
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    print(f"{what}: err {err:.3e}, tol {tol:.1e} * {scale:.3e}")
    assert err <= tol * scale + floor, f"{what}: max err {err:.3e} > {tol:.1e} * {scale:.3e} + {floor:.1e}"


def check_loss(got, ref, what):
    got, ref = float(got), float(ref)
    print(f"{what}: {got!r} vs {ref!r}, rel {abs(got - ref) / abs(ref):.3e}")
    assert abs(got - ref) <= cc.TOL_LOSS * abs(ref), f"{what}: {got!r} vs {ref!r}"


# ================================================================ SupCon
def run_supcon(path, P, labels, codes, matrices=False):
    """forward and backward of one path on NaN-filled buffers -> dict(loss, dP, stats, [sim_logits, sim_exp, pos, neg])"""
    lib = _load()
    R, D = P.shape
    n = R // 2
    gs = torch.full((1,), cc.GSCALE, device=DEV)
    out = {"loss": nanf(1), "stats": nanf(R, 4), "dP": nanf(R, D)}
    lp, mp, st = ptr(labels), ptr(codes), stream()
    if path == "fused":
        nbytes = lib.cy_supcon_fused_ws_bytes(n, D)
        ws, out["diag"] = nanf((nbytes + 3) // 4), nanf(R)
        lib_call("cy_supcon_fused_fwd", P.data_ptr(), lp, mp, out["loss"].data_ptr(), out["stats"].data_ptr(),
                 out["diag"].data_ptr(), ws.data_ptr(), nbytes, n, D, cc.T, st)
        ws.fill_(NAN)
        lib_call("cy_supcon_fused_bwd", P.data_ptr(), lp, mp, out["stats"].data_ptr(), gs.data_ptr(), out["dP"].data_ptr(),
                 ws.data_ptr(), nbytes, n, D, cc.T, st)
        return out
    S, G = nanf(R, R), nanf(R, R)
    if path == "materialised":
        lib_call("cy_supcon_fwd", P.data_ptr(), lp, mp, S.data_ptr(), out["loss"].data_ptr(), out["stats"].data_ptr(), n, D,
                 cc.T, st)
        lib_call("cy_supcon_bwd", P.data_ptr(), lp, mp, S.data_ptr(), out["stats"].data_ptr(), gs.data_ptr(), G.data_ptr(),
                 out["dP"].data_ptr(), n, D, cc.T, st)
    else:
        assert path == "exclude_other_pos"
        tmp = nanf(4 * R + 1)
        lib_call("cy_supcon_excl_fwd", P.data_ptr(), lp, mp, S.data_ptr(), out["loss"].data_ptr(), out["stats"].data_ptr(),
                 tmp.data_ptr(), n, D, cc.T, st)
        lib_call("cy_supcon_excl_bwd", P.data_ptr(), lp, mp, S.data_ptr(), out["stats"].data_ptr(), tmp.data_ptr(),
                 gs.data_ptr(), G.data_ptr(), out["dP"].data_ptr(), n, D, cc.T, st)
    out["G"] = G
    if matrices:
        m = [nanf(R, R) for _ in range(4)]
        lib_call("cy_supcon_matrices", S.data_ptr(), out["stats"].data_ptr(), lp, mp, *[x.data_ptr() for x in m], n, st)
        out["sim_logits"], out["sim_exp"], out["pos"], out["neg"] = m
    return out


def _load():
    from cyhip import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def golden(golden_dir):
    g = np.load(golden_dir / cc.GOLDEN_FILE)
    return {k: torch.from_numpy(np.asarray(g[k])) for k in g.files}


def codes_of(mask):
    """the kernels' uint8 codes straight from a mask's values: -1 becomes 255, 2 stays 2 -- both 'any other value'"""
    return mask.to(torch.int8).to(torch.uint8).to(DEV).contiguous()


def unit_rows(n, D, seed):
    """two views of n unit-norm rows; seed None: cc.twin_rows, the exact inputs of the one-pair case"""
    if seed is None:
        z1 = torch.tensor(cc.twin_rows(n, D), dtype=torch.float32)
        return z1, z1.clone()
    g = torch.Generator().manual_seed(seed)
    z1 = F.normalize(torch.randn(n, D, generator=g), dim=1)
    z2 = F.normalize(z1 + 0.4 * torch.randn(n, D, generator=g), dim=1)
    return z1, z2


def targets(kind, n):
    return list(range(n)) if kind == "simclr" else [i % 3 for i in range(n)]


@functools.lru_cache(maxsize=None)
def oracle_ref(n, D, seed, positives, excl, mask_seed=None):
    """(loss, dP) of the oracle in float64 for labels (`positives`) or a mask of kind (d) (`mask_seed`)"""
    from oracle import losses as ol
    z1, z2 = unit_rows(n, D, seed)
    a, b = z1.double().requires_grad_(True), z2.double().requires_grad_(True)
    kw = {"mask": cc.kind_d_mask(n, mask_seed)} if mask_seed is not None else {"target": targets(positives, n)}
    loss = (ol.supcon_loss_exclude_pos if excl else ol.supcon_loss)(a, b, t=cc.T, **kw)
    loss.backward()
    return loss.item(), torch.cat([a.grad, b.grad])


@functools.lru_cache(maxsize=None)
def chunked_ref(n, D, seed, positives):
    """SupConLoss1 with labels in float64 without the R x R matrix: rows in chunks of cc.CHUNK_ROWS, autograd
    accumulating into P.grad.  The global shift max S is detached in the reference and lies on the diagonal
    (S_ij <= max(S_ii, S_jj)), so it is known before the first chunk and chunking does not change the function."""
    z1, z2 = unit_rows(n, D, seed)
    P = torch.cat([z1, z2]).double().requires_grad_(True)
    R = 2 * n
    lab = torch.tensor(targets(positives, n) * 2)
    same = torch.nn.functional.one_hot(lab).double()   # [R][classes]: S @ same = per row the sums of S over each class
    with torch.no_grad():
        M = ((P * P).sum(1) / cc.T).max()
    total = 0.0
    for r0 in range(0, R, cc.CHUNK_ROWS):
        r1 = min(R, r0 + cc.CHUNK_ROWS)
        rows = torch.arange(r1 - r0)
        S = P[r0:r1] @ P.t() / cc.T - M
        E = torch.exp(S)
        den = E.sum(1) - E[rows, rows + r0] + 1e-16   # (the diagonal term is 1 of a sum of tens: nothing cancels)
        # the positives of row i: its own class without itself
        ps = (S @ same)[rows, lab[r0:r1]] - S[rows, rows + r0]
        cnt = same.sum(0)[lab[r0:r1]] - 1
        part = -((ps / cnt) - torch.log(den)).sum() / R
        part.backward()
        total += part.item()
    return total, P.grad.clone()


@pytest.mark.parametrize("name", list(cc.GOLDEN_MASKS))
def test_golden_masks_on_every_path(name, golden_dir):
    """the reference's own loss and gradient for each mask of supcon_masks.npz on the three paths; fused against
    materialised; the fused path twice, bit for bit; the four matrices of the materialised and exclude_other_pos paths"""
    g = golden(golden_dir)
    n = cc.GOLDEN_N
    P = gpu(torch.cat([g["z1"], g["z2"]]))
    codes = codes_of(g[f"{name}_mask"])
    res = {}
    for path in cc.PATHS:
        excl = int(path == "exclude_other_pos")
        r = res[path] = run_supcon(path, P, None, codes, matrices=path != "fused")
        check_loss(r["loss"].item(), g[f"{name}_e{excl}_loss"].item(), f"{name} {path} loss")
        ref = cc.GSCALE * torch.cat([g[f"{name}_e{excl}_dz1"], g[f"{name}_e{excl}_dz2"]])
        check(r["dP"], ref, cc.TOL_GRAD, f"{name} {path} dP")
        if path != "fused":
            assert torch.equal(r["pos"].cpu(), g[f"{name}_pos"].float()), f"{name} {path} pos_mask"
            assert torch.equal(r["neg"].cpu(), g[f"{name}_neg"].float()), f"{name} {path} neg_mask"
            if name == "d":
                check(r["sim_logits"], g["d_sim_logits"], cc.TOL_SIM, f"{path} sim_logits")
                check(r["sim_exp"], g["d_sim_exp"], cc.TOL_SIM, f"{path} sim_exp")
            assert float(r["G"].diagonal().abs().max()) == 0.0, "the gradient matrix has a zero diagonal"
    f, m = res["fused"], res["materialised"]
    check_loss(f["loss"].item(), m["loss"].item(), f"{name} fused vs materialised loss")
    check(f["dP"], m["dP"], cc.TOL_PATHS, f"{name} fused vs materialised dP")
    check(f["stats"][:, :3], m["stats"][:, :3], cc.TOL_PATHS, f"{name} fused vs materialised row statistics")
    assert torch.equal(f["stats"][:, 1].cpu(), g[f"{name}_pos"].float().sum(1)), "positives per row, exact"
    check(f["diag"], (P * P).sum(1).double() / cc.T, 1e-6, "diag")
    again = run_supcon("fused", P, None, codes)
    assert torch.equal(again["loss"], f["loss"]) and torch.equal(again["dP"], f["dP"]) and torch.equal(again["stats"], f["stats"])


@pytest.mark.parametrize("path", cc.PATHS)
def test_criterion_with_the_general_mask(path, monkeypatch, golden_dir):
    """SupConLoss1(mask=) with the four-valued asymmetric mask (d), .backward() with an upstream gradient, and the four
    inspection properties, against the reference's vectors -- once per path the criterion can take"""
    ops = _ops()
    from contrastyou.losses.contrastive import SupConLoss1
    g = golden(golden_dir)
    if path == "materialised":
        monkeypatch.setattr(ops, "SUPCON_FUSED", False)
    excl = int(path == "exclude_other_pos")
    z1, z2 = gpu(g["z1"]).requires_grad_(True), gpu(g["z2"]).requires_grad_(True)
    assert ops.supcon_fused_ok(torch.cat([z1, z2])) == (path != "materialised")
    crit = SupConLoss1(temperature=cc.T, exclude_other_pos=bool(excl))
    loss = crit(z1, z2, mask=g["d_mask"].float())
    (loss * cc.GSCALE).backward()
    check_loss(loss.item(), g[f"d_e{excl}_loss"].item(), f"criterion {path} loss")
    check(z1.grad, cc.GSCALE * g[f"d_e{excl}_dz1"], cc.TOL_GRAD, f"criterion {path} dz1")
    check(z2.grad, cc.GSCALE * g[f"d_e{excl}_dz2"], cc.TOL_GRAD, f"criterion {path} dz2")
    check(crit.sim_logits, g["d_sim_logits"], cc.TOL_SIM, "sim_logits")
    check(crit.sim_exp, g["d_sim_exp"], cc.TOL_SIM, "sim_exp")
    assert torch.equal(crit.pos_mask.cpu(), g["d_pos"].float()) and torch.equal(crit.neg_mask.cpu(), g["d_neg"].float())
    # the same mask on the device, and as integers
    for m in (g["d_mask"].to(DEV), g["d_mask"].long()):
        assert torch.equal(crit(z1.detach(), z2.detach(), mask=m), loss.detach())


@pytest.mark.parametrize("case", cc.SPLIT_CASES, ids=lambda c: c.name)
def test_column_split_geometry(case):
    """row-block and column-split counts of the fused kernels from one block to past the split budget, labels mode"""
    n, D = case.n, case.D
    seed = None if case.twins else 500 + n
    z1, z2 = unit_rows(n, D, seed)
    P = gpu(torch.cat([z1, z2]))
    lab = torch.tensor(targets(case.positives, n), dtype=torch.int32, device=DEV)
    res = {}
    for path in case.paths:
        excl = path == "exclude_other_pos"
        if 2 * n >= cc.CHUNKED_FROM:
            assert path == "fused"
            rloss, rdP = chunked_ref(n, D, seed, case.positives)
        else:
            rloss, rdP = oracle_ref(n, D, seed, case.positives, excl)
        r = res[path] = run_supcon(path, P, lab, None)
        if case.twins:  # loss and gradient are 0 up to the reference's own rounding of 1 + 1e-16 (contrast_cases.py)
            assert rloss == 0.0 and float(rdP.abs().max()) == 0.0
            err_l, err_g = abs(r["loss"].item()), r["dP"].abs().max().item()
            print(f"{case.name} {path}: |loss| {err_l:.3e}, max|dP| {err_g:.3e}, bound {cc.ONE_PAIR_ABS:.0e}")
            assert err_l <= cc.ONE_PAIR_ABS and err_g <= cc.ONE_PAIR_ABS, (path, err_l, err_g)
            assert torch.equal(r["stats"][:, 1].cpu(), torch.ones(2)), "one positive per row"
            continue
        check_loss(r["loss"].item(), rloss, f"{case.name} {path} loss")
        check(r["dP"], cc.GSCALE * rdP, cc.TOL_GRAD, f"{case.name} {path} dP")
    if "materialised" in res:
        check(res["fused"]["dP"], res["materialised"]["dP"], cc.TOL_PATHS, "fused vs materialised dP")
    again = run_supcon("fused", P, lab, None)
    assert torch.equal(again["loss"], res["fused"]["loss"]) and torch.equal(again["dP"], res["fused"]["dP"])


@pytest.mark.parametrize("positives", ["labels", "mask"])
@pytest.mark.parametrize("D", cc.FUSED_WIDTHS)
def test_fused_widths(D, positives):
    """1, 2, 3, 5 and 8 (ragged, full) column tiles of the fused backward's second product"""
    n = cc.WIDTH_N
    P = gpu(torch.cat(unit_rows(n, D, 600 + D)))
    assert _ops().supcon_fused_ok(P)
    if positives == "labels":
        lab, codes = torch.tensor(targets("mod3", n), dtype=torch.int32, device=DEV), None
        rloss, rdP = oracle_ref(n, D, 600 + D, "mod3", False)
    else:
        lab, codes = None, codes_of(cc.kind_d_mask(n, 61))
        rloss, rdP = oracle_ref(n, D, 600 + D, None, False, 61)
    f = run_supcon("fused", P, lab, codes)
    check_loss(f["loss"].item(), rloss, f"D={D} fused loss")
    check(f["dP"], cc.GSCALE * rdP, cc.TOL_GRAD, f"D={D} fused dP")
    m = run_supcon("materialised", P, lab, codes)
    check(f["dP"], m["dP"], cc.TOL_PATHS, f"D={D} fused vs materialised dP")


@pytest.mark.parametrize("positives", ["labels", "mask"])
@pytest.mark.parametrize("D", cc.MATERIALISED_WIDTHS)
def test_materialised_widths(D, positives):
    """K below, across and past the 16-wide stage of the GEMM, and the widths the fused path refuses"""
    n = cc.WIDTH_N
    P = gpu(torch.cat(unit_rows(n, D, 700 + D)))
    assert not _ops().supcon_fused_ok(P)
    for path in ("materialised", "exclude_other_pos"):
        excl = path == "exclude_other_pos"
        if positives == "labels":
            lab, codes = torch.tensor(targets("mod3", n), dtype=torch.int32, device=DEV), None
            rloss, rdP = oracle_ref(n, D, 700 + D, "mod3", excl)
        else:
            lab, codes = None, codes_of(cc.kind_d_mask(n, 61))
            rloss, rdP = oracle_ref(n, D, 700 + D, None, excl, 61)
        r = run_supcon(path, P, lab, codes)
        check_loss(r["loss"].item(), rloss, f"D={D} {path} loss")
        check(r["dP"], cc.GSCALE * rdP, cc.TOL_GRAD, f"D={D} {path} dP")


def test_elementwise_kernels_past_the_block_cap():
    """R = 1450: R * R elements are more than 8192 blocks of 256 -- the grid-stride loops of the gradient matrices and
    of cy_supcon_matrices go round again -- with a mask of kind (d)"""
    from oracle import losses as ol
    n, D = cc.CAP_N, cc.CAP_D
    mask = cc.kind_d_mask(n, 62)
    P = gpu(torch.cat(unit_rows(n, D, 800)))
    codes = codes_of(mask)
    pos, neg = ol.supcon_masks(n, mask=mask)
    for path in ("materialised", "exclude_other_pos"):
        rloss, rdP = oracle_ref(n, D, 800, None, path == "exclude_other_pos", 62)
        r = run_supcon(path, P, None, codes, matrices=True)
        check_loss(r["loss"].item(), rloss, f"cap {path} loss")
        check(r["dP"], cc.GSCALE * rdP, cc.TOL_GRAD, f"cap {path} dP")
        assert torch.equal(r["pos"].cpu(), pos) and torch.equal(r["neg"].cpu(), neg), f"cap {path} masks"
        Pd = P.cpu().double()
        S = Pd @ Pd.t() / cc.T
        S = S - S.max()
        check(r["sim_logits"], S, cc.TOL_SIM, f"cap {path} sim_logits")
        check(r["sim_exp"], S.exp(), cc.TOL_SIM, f"cap {path} sim_exp")
        # the gradient matrix itself, last element included: dP = (G + G^T) P / t has been formed from all of it
        assert torch.isfinite(r["G"]).all() and float(r["G"].diagonal().abs().max()) == 0.0


# ================================================================ cy_sgemm
@pytest.mark.parametrize("b_trans", [0, 1])
@pytest.mark.parametrize("size", cc.SGEMM_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_sgemm(size, b_trans):
    M, N, K = size
    g = torch.Generator().manual_seed(M * 1000 + N)
    A, B = rnd(M, K, gen=g).float(), rnd(*((N, K) if b_trans else (K, N)), gen=g).float()
    Cm, Ag, Bg = nanf(M, N), gpu(A), gpu(B)
    lib_call("cy_sgemm", Ag.data_ptr(), Bg.data_ptr(), Cm.data_ptr(), M, N, K, cc.SGEMM_ALPHA, b_trans, stream())
    ref = cc.SGEMM_ALPHA * A.double() @ (B.double().t() if b_trans else B.double())
    check(Cm, ref, cc.TOL_SGEMM, f"sgemm {size} b_trans={b_trans}")


# ================================================================ projector pieces
def dcode(dt):
    return _ops().dtype_code(DT[dt])


@pytest.mark.parametrize("dt", cc.TYPES)
def test_avgpool(dt):
    """every HW x C of the table, forward and backward; feature maps are [N][HW][C]"""
    g = torch.Generator().manual_seed(31)
    N = cc.POOL_N
    for HW in cc.POOL_HW:
        for C in cc.POOL_C:
            x = rnd(N, HW, C, gen=g).to(DT[dt])
            pooled, xg = nanf(N, C), gpu(x, DT[dt])
            lib_call("cy_avgpool_fwd", xg.data_ptr(), pooled.data_ptr(), N, HW, C, dcode(dt), stream())
            check(pooled, x.double().mean(1), cc.TOL_POOL, f"avgpool fwd HW={HW} C={C} {dt}")
            dp = rnd(N, C, gen=g).float()
            dx, dpg = nanf(N, HW, C, dtype=DT[dt]), gpu(dp)
            lib_call("cy_avgpool_bwd", dpg.data_ptr(), dx.data_ptr(), N, HW, C, dcode(dt), stream())
            check(dx, (dp.double() / HW)[:, None, :].expand(N, HW, C), cc.TOL_16[dt], f"avgpool bwd HW={HW} C={C} {dt}")


@pytest.mark.parametrize("dt", cc.TYPES)
def test_avgpool_bwd_past_the_block_cap(dt):
    N, HW, C = cc.POOL_CAP
    g = torch.Generator().manual_seed(32)
    dp = rnd(N, C, gen=g).float()
    dx, dpg = nanf(N, HW, C, dtype=DT[dt]), gpu(dp)
    lib_call("cy_avgpool_bwd", dpg.data_ptr(), dx.data_ptr(), N, HW, C, dcode(dt), stream())
    check(dx, (dp.double() / HW)[:, None, :].expand(N, HW, C), cc.TOL_16[dt], f"avgpool bwd past the cap {dt}")


def linear_ref(x, w, b, dy, act):
    x, w = x.double().requires_grad_(True), w.double().requires_grad_(True)
    b = None if b is None else b.double().requires_grad_(True)
    y = F.linear(x, w, b)
    if act:
        y = F.leaky_relu(y, cc.LINEAR_SLOPE)
    y.backward(dy.double())
    return y.detach(), x.grad, w.grad, None if b is None else b.grad


def run_linear_bwd(entry, x, w, y, dy, act, want, fill):
    M, I = x.shape
    O = w.shape[0]
    bufs = [torch.full(s, fill, device=DEV) if k else None for k, s in zip(want, ((M, I), (O, I), (O,)))]
    lib_call(entry, x.data_ptr(), w.data_ptr(), y.data_ptr(), dy.data_ptr(), *[ptr(t) for t in bufs], M, I, O, act,
             cc.LINEAR_SLOPE, stream())
    return bufs


@pytest.mark.parametrize("act", cc.LINEAR_ACTS)
@pytest.mark.parametrize("bias", [True, False])
def test_linear(act, bias):
    """every I x O of the table: forward, backward, and the accumulating backward into buffers that hold 1.5"""
    g = torch.Generator().manual_seed(33 + act)
    M = cc.LINEAR_M
    for I in cc.LINEAR_I:
        for O in cc.LINEAR_O:
            x, w, dy = rnd(M, I, gen=g).float(), rnd(O, I, gen=g).float(), rnd(M, O, gen=g).float()
            b = rnd(O, gen=g).float() if bias else None
            ry, rdx, rdw, rdb = linear_ref(x, w, b, dy, act)
            xg, wg, dyg, bg = gpu(x), gpu(w), gpu(dy), None if b is None else gpu(b)
            y = nanf(M, O)
            lib_call("cy_linear_fwd", xg.data_ptr(), wg.data_ptr(), ptr(bg), y.data_ptr(), M, I, O, act, cc.LINEAR_SLOPE,
                     stream())
            what = f"linear I={I} O={O} act={act} bias={bias}"
            check(y, ry, cc.TOL_Z, what + " y")
            if rdb is None:  # (db does not depend on the bias being there)
                rdb = linear_ref(x, w, torch.zeros(O), dy, act)[3]
            dx, dw, db = run_linear_bwd("cy_linear_bwd", xg, wg, y, dyg, act, (1, 1, 1), NAN)
            check(dx, rdx, cc.TOL_GRAD, what + " dx"), check(dw, rdw, cc.TOL_GRAD, what + " dw")
            check(db, rdb, cc.TOL_GRAD, what + " db")
            dx, dw, db = run_linear_bwd("cy_linear_bwd_into", xg, wg, y, dyg, act, (1, 1, 1), 1.5)
            check(dx, rdx, cc.TOL_GRAD, what + " dx (into: written, not added)")
            check(dw - 1.5, rdw, cc.TOL_GRAD, what + " dw added"), check(db - 1.5, rdb, cc.TOL_GRAD, what + " db added")


@pytest.mark.parametrize("want", cc.LINEAR_WANTS, ids=lambda w: "dx%d-dw%d-db%d" % w)
def test_linear_bwd_null_outputs(want):
    """each combination of null dx / dw / db, both activations, both entries: what is asked for is right, and the call
    with nothing asked for is accepted"""
    I, O = cc.LINEAR_WANTS_AT
    M = cc.LINEAR_M
    g = torch.Generator().manual_seed(35)
    for act in cc.LINEAR_ACTS:
        x, w, b, dy = rnd(M, I, gen=g).float(), rnd(O, I, gen=g).float(), rnd(O, gen=g).float(), rnd(M, O, gen=g).float()
        ry, *refs = linear_ref(x, w, b, dy, act)
        for entry, fill in (("cy_linear_bwd", NAN), ("cy_linear_bwd_into", 1.5)):
            dev = [gpu(t) for t in (x, w, ry, dy)]
            bufs = run_linear_bwd(entry, *dev, act, want, fill)
            for k, (got, ref) in enumerate(zip(bufs, refs)):
                if got is not None:
                    added = 1.5 if (entry.endswith("into") and k > 0) else 0.0
                    check(got - added, ref, cc.TOL_GRAD, f"{entry} act={act} want={want} output {k}")


@pytest.mark.parametrize("M", cc.L2_M)
def test_l2norm(M):
    """every D of the table; row L2_ZERO_ROW of the cases with more than one row (and, for M = 1, a case of its own) is
    exactly zero: z = 0 and dx = dz / eps, what F.normalize gives in float64.  Compared row by row: the zero row's
    gradient is 1e12 times the others'."""
    g = torch.Generator().manual_seed(36 + M)
    for D in cc.L2_D:
        for zero in ((True,) if M > 1 else (False, True)):
            x, dz = rnd(M, D, gen=g).float(), rnd(M, D, gen=g).float()
            if zero:
                x[cc.L2_ZERO_ROW] = 0
            xr = x.double().requires_grad_(True)
            zr = F.normalize(xr, p=2, dim=1, eps=cc.L2_EPS)
            zr.backward(dz.double())
            if zero:
                assert torch.equal(xr.grad[cc.L2_ZERO_ROW], dz[cc.L2_ZERO_ROW].double() / cc.L2_EPS)
            xg, dzg = gpu(x), gpu(dz)
            z, norms, dx = nanf(M, D), nanf(M), nanf(M, D)
            lib_call("cy_l2norm_fwd", xg.data_ptr(), z.data_ptr(), norms.data_ptr(), M, D, cc.L2_EPS, stream())
            lib_call("cy_l2norm_bwd", xg.data_ptr(), norms.data_ptr(), dzg.data_ptr(), dx.data_ptr(), M, D, cc.L2_EPS,
                     stream())
            what = f"l2norm M={M} D={D} zero={zero}"
            check(z, zr, cc.TOL_Z, what + " z")
            check(norms, x.double().norm(dim=1), cc.TOL_Z, what + " norms")
            check(dx, xr.grad, cc.TOL_GRAD, what + " dx")  # (the issue's rule: the zero row sets the scale)
            # and row by row, each row against the size of its own two terms dz / nrm and x (x . dz) / nrm^3 -- for
            # D = 1 they cancel to zero
            term = dz.double().abs().amax(1) / x.double().norm(dim=1).clamp_min(cc.L2_EPS)
            check(dx, xr.grad, cc.TOL_GRAD, what + " dx", rows=term)
            if zero:
                assert float(z[cc.L2_ZERO_ROW].abs().max()) == 0.0 and float(norms[cc.L2_ZERO_ROW]) == 0.0


# ================================================================ the one-launch projection head
def head_ref(feat, w1, b1, w2, b2, dz):
    """float64, end to end: mean over positions -> Linear -> LeakyReLU -> Linear -> F.normalize, with autograd"""
    leaves = [t.double().requires_grad_(True) for t in (feat, w1, b1, w2, b2)]
    f, W1, B1, W2, B2 = leaves
    pooled = f.mean(1)
    y1 = F.leaky_relu(F.linear(pooled, W1, B1), cc.HEAD_SLOPE)
    y2 = F.linear(y1, W2, B2)
    z = F.normalize(y2, p=2, dim=1, eps=cc.HEAD_EPS)
    z.backward(dz.double())
    fwd = dict(pooled=pooled.detach(), y1=y1.detach(), y2=y2.detach(), z=z.detach(), norms=y2.detach().norm(dim=1))
    return fwd, [t.grad for t in leaves]


def run_head(feat, w1, b1, w2, b2, dz, dt, want_dfeat=True, sinks=None):
    B, HW, C = feat.shape
    hid, out = w1.shape[0], w2.shape[0]
    lib = _load()
    fwd = dict(pooled=nanf(B, C), y1=nanf(B, hid), y2=nanf(B, out), z=nanf(B, out), norms=nanf(B))
    lib_call("cy_proj_head_fwd", feat.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
             fwd["pooled"].data_ptr(), fwd["y1"].data_ptr(), fwd["y2"].data_ptr(), fwd["z"].data_ptr(),
             fwd["norms"].data_ptr(), B, HW, C, hid, out, cc.HEAD_SLOPE, cc.HEAD_EPS, dcode(dt), stream())
    dfeat = nanf(B, HW, C, dtype=DT[dt]) if want_dfeat else None
    grads = sinks if sinks is not None else [nanf(hid, C), nanf(hid), nanf(out, hid), nanf(out)]
    nbytes = lib.cy_proj_head_bwd_ws_bytes(B, hid, out)
    ws = nanf((nbytes + 3) // 4)
    lib_call("cy_proj_head_bwd", dz.data_ptr(), fwd["pooled"].data_ptr(), fwd["y1"].data_ptr(), fwd["y2"].data_ptr(),
             fwd["norms"].data_ptr(), w1.data_ptr(), w2.data_ptr(), ptr(dfeat), *[t.data_ptr() for t in grads],
             int(sinks is not None), ws.data_ptr(), nbytes, B, HW, C, hid, out, cc.HEAD_SLOPE, cc.HEAD_EPS, dcode(dt),
             stream())
    return fwd, dfeat, grads


def head_inputs(shape, HW, B, dt, seed, zero_sample=None):
    C, hid, out = shape
    g = torch.Generator().manual_seed(seed)
    feat = rnd(B, HW, C, gen=g).to(DT[dt])
    w1, b1 = (rnd(hid, C, gen=g) / C ** 0.5).float(), (rnd(hid, gen=g) / C ** 0.5).float()
    w2, b2 = (rnd(out, hid, gen=g) / hid ** 0.5).float(), (rnd(out, gen=g) / hid ** 0.5).float()
    dz = rnd(B, out, gen=g).float()
    if zero_sample is not None:
        feat[zero_sample] = 0
        b1.zero_(), b2.zero_()
        dz[zero_sample] *= 1e-12  # dy2 = dz / eps for that sample: of the size of the others' (and inside f16's range)
    return feat, w1, b1, w2, b2, dz


def check_head(got, ref, dt, what):
    fwd, dfeat, grads = got
    rfwd, rgrads = ref
    # one output: the normalised vector is +-1 and every gradient cancels to zero (contrast_cases.HEAD_OUT1_BOUND)
    floor = cc.HEAD_OUT1_BOUND if rfwd["z"].shape[1] == 1 else dict.fromkeys(cc.HEAD_OUT1_BOUND, 0.0)
    for k in ("pooled", "y1", "y2", "norms", "z"):
        check(fwd[k], rfwd[k], cc.TOL_Z, f"{what} {k}")
    if dfeat is not None:
        check(dfeat, rgrads[0], cc.TOL_16[dt], f"{what} dfeat", floor=floor["dfeat"])
    for k, got_g, ref_g in zip(("dw1", "db1", "dw2", "db2"), grads, rgrads[1:]):
        check(got_g, ref_g, cc.TOL_GRAD, f"{what} {k}", floor=floor[k])


def head_f32_mirror(feat, w1, b1, w2, b2, dz):
    """the kernels' own operations (proj_head_fwd_kernel / _bwd_kernel / _dw_kernel) in float32 on the CPU: gradients
    (dfeat, dw1, db1, dw2, db2).  Summation orders are torch's."""
    feat, w1, b1, w2, b2, dz = [t.float() for t in (feat, w1, b1, w2, b2, dz)]
    HW = feat.shape[1]
    pooled = feat.mean(1)
    y1 = F.leaky_relu(pooled @ w1.t() + b1, cc.HEAD_SLOPE)
    y2 = y1 @ w2.t() + b2
    iv = 1 / (y2 * y2).sum(1, keepdim=True).sqrt()
    dot = (y2 * dz).sum(1, keepdim=True)
    dy2 = dz * iv - y2 * (dot * iv * iv * iv)
    dh = (dy2 @ w2) * torch.where(y1 > 0, 1.0, cc.HEAD_SLOPE)
    dfeat = ((dh @ w1) * (1.0 / HW))[:, None, :].expand_as(feat)
    return [dfeat, dh.t() @ pooled, dh.sum(0), dy2.t() @ y1, dy2.sum(0)]


def yardstick_head_out1():
    """contrast_cases.HEAD_OUT1_YARDSTICK: the (C, hid, 1) case in float32 on the CPU, the kernels' operations, against
    the float64 reference -- the largest error of each gradient over the case's HW x B x storage types.  Run by hand."""
    worst = dict.fromkeys(cc.HEAD_OUT1_BOUND, 0.0)
    shape = next(s for s in cc.HEAD_SHAPES if s[2] == 1)
    for dt in cc.TYPES:
        for HW in cc.HEAD_HW:
            for B in cc.HEAD_B:
                ins = head_inputs(shape, HW, B, dt, 40 + HW + B)
                for k, a, b in zip(worst, head_f32_mirror(*ins), head_ref(*ins)[1]):
                    worst[k] = max(worst[k], (a.double() - b).abs().max().item())
    return worst


@pytest.mark.parametrize("dt", cc.TYPES)
@pytest.mark.parametrize("shape", cc.HEAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_proj_head_one_launch(shape, dt):
    """every HW x B of the table against float64 end to end; at the hook's size also: dfeat null, parameter gradients
    added into buffers that hold 1.5, and a second run bit for bit"""
    for HW in cc.HEAD_HW:
        for B in cc.HEAD_B:
            ins = head_inputs(shape, HW, B, dt, 40 + HW + B)
            ref = head_ref(*ins)
            dev = [gpu(ins[0], DT[dt])] + [gpu(t) for t in ins[1:]]
            got = run_head(*dev, dt)
            what = f"head {shape} HW={HW} B={B} {dt}"
            check_head(got, ref, dt, what)
            if HW == cc.HEAD_HW[-1]:
                again = run_head(*dev, dt)
                assert all(torch.equal(again[0][k], got[0][k]) for k in got[0]) and torch.equal(again[1], got[1])
                assert all(torch.equal(a, b) for a, b in zip(again[2], got[2])), what + ": second run differs"
                sinks = [torch.full_like(t, 1.5) for t in got[2]]
                _, none, added = run_head(*dev, dt, want_dfeat=False, sinks=sinks)
                assert none is None
                for k, a, r in zip(("dw1", "db1", "dw2", "db2"), added, ref[1][1:]):
                    # (1.5 + g - 1.5 rounds g to the spacing of f32 at 1.5, 1.2e-7: half of it as a floor)
                    out1 = cc.HEAD_OUT1_BOUND[k] if shape[2] == 1 else 0.0
                    check(a - 1.5, r, cc.TOL_GRAD, f"{what} {k} added into", floor=2.0 ** -24 + out1)


@pytest.mark.parametrize("dt", cc.TYPES)
def test_proj_head_zero_sample(dt):
    """one sample of all-zero features with zero biases: LeakyReLU at 0 (slope side) and a zero norm, where
    z = 0 and dy2 = dz / eps"""
    zc = cc.HEAD_ZERO
    ins = head_inputs(zc["shape"], zc["HW"], zc["B"], dt, 44, zero_sample=zc["sample"])
    ref = head_ref(*ins)
    assert float(ref[0]["norms"][zc["sample"]]) == 0.0 and float(ref[1][0][zc["sample"]].abs().max()) > 0
    got = run_head(gpu(ins[0], DT[dt]), *[gpu(t) for t in ins[1:]], dt)
    check_head(got, ref, dt, f"head zero sample {dt}")
    s = zc["sample"]
    assert float(got[0]["z"][s].abs().max()) == 0.0 and float(got[0]["norms"][s]) == 0.0
    check(got[1][s], ref[1][0][s], cc.TOL_16[dt], f"head zero sample {dt}: dfeat of that sample")


@pytest.mark.parametrize("case", cc.MODULE_CASES, ids=lambda c: c[0])
def test_projection_head_module(case):
    """ProjectionHead.forward + backward through the one-launch path and through the pieces proj_head_ok sends the
    other shapes to, against float64"""
    from contrastyou.projectors.heads import ProjectionHead
    name, C, hid, out, one_launch = case
    B, H, W = 3, 3, 2
    feat, w1, b1, w2, b2, dz = head_inputs((C, hid, out), H * W, B, "f32", 45)
    head = ProjectionHead(input_dim=C, hidden_dim=hid, output_dim=out, head_type="mlp", normalize=True).to(DEV)
    sd = {"_header.2.weight": w1, "_header.2.bias": b1, "_header.4.weight": w2, "_header.4.bias": b2}
    head.load_state_dict(sd, strict=True)
    x = feat.float().view(B, H, W, C).permute(0, 3, 1, 2).to(DEV).requires_grad_(True)  # NCHW view of NHWC memory
    assert _ops().proj_head_ok(x, head._header[2].weight, head._header[4].weight) == one_launch
    z = head(x)
    z.backward(gpu(dz))
    rfwd, rg = head_ref(feat, w1, b1, w2, b2, dz)
    check(z, rfwd["z"], cc.TOL_Z, f"{name} z")
    check(x.grad.permute(0, 2, 3, 1).reshape(B, H * W, C), rg[0], cc.TOL_GRAD, f"{name} dfeat")
    for k, ref in zip(sd, rg[1:]):
        check(head.state_dict(keep_vars=True)[k].grad, ref, cc.TOL_GRAD, f"{name} grad of {k}")
