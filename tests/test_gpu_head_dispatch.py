"""Parity of the kernels behind the decoder on every dispatch branch and past every launch cap: the 1x1 head
(cy_head1x1_fwd / _bwd / _bwd_into), softmax-KL, softmax-MSE, dice counts (csrc/cy_head_loss.hip), the cluster head in
its softmax mode (csrc/cy_cluster_head.hip) and the projection head with the separate kernels it fuses
(csrc/cy_proj_head.hip).  The cases are those of tests/head_cases.py; tests/test_head_plan_coverage.py checks on the CPU
that they reach every branch and cap.

Reference: torch on the CPU in float64, with autograd, on inputs already rounded to the storage type.  Tolerances, on
max|got - ref| <= tol * max|ref|: logits and probabilities 1e-5; dw, db 1e-4; dx 1e-4 (f32) or ATOL of
test_gpu_kernels.py (16-bit); the gradients of the losses 1e-4; loss scalars 1e-5 * max(1, |ref|); dice counts exact.

Cases that go round a loop a second time carry sentinel pixels -- pixel 0, the last pixel of the first trip, the first
of the second (from the plan's grid) and the last pixel -- with a marker of magnitude 64 in one channel of x and one
class of dlogits.  Before the GPU is looked at, the reference is recomputed with each sentinel dropped in turn and must
move by at least 10 x the tolerance; for outputs with one row per pixel that means the sentinel's own row.  Row-wise
outputs are also compared without the sentinel rows, whose size would otherwise set the scale for every other pixel."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import head_cases as hc
from tests.test_gpu_kernels import ATOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MARK = 64.0


def _ops():
    from cyhip import ops
    return ops


def rnd(*shape, gen):
    return torch.rand(*shape, generator=gen, dtype=torch.float64) * 2 - 1


def to_map(rows, shape, dt):
    """[npix, C] rows on the CPU -> GPU tensor [N, C, H, W] with NHWC memory"""
    N, H, W = shape
    return rows.to(dt).to(DEV).view(N, H, W, rows.shape[1]).permute(0, 3, 1, 2)


def to_rows(t):
    """GPU tensor [N, C, H, W] with NHWC memory -> f64 rows [npix, C] on the CPU"""
    return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).cpu().double()


def check(got, ref, tol, what, skip_rows=None, floor=0.0):
    """max|got - ref| <= tol * max|ref| (+ floor: only where the reference is exactly zero by construction)"""
    got = got.detach().cpu().double().reshape(ref.shape)
    scale, err = ref.abs().max().item(), (got - ref).abs().max().item()
    print(f"{what}: err {err:.3e}, tol {tol:.0e} * {scale:.3e}")
    assert err <= tol * scale + floor, f"{what}: max err {err:.3e} > {tol:.0e} * {scale:.3e} + {floor:.1e}"
    if skip_rows:  # the same without the sentinel rows (their markers set the scale above)
        keep = torch.ones(ref.shape[0], dtype=torch.bool)
        keep[list(skip_rows)] = False
        scale, err = ref[keep].abs().max().item(), (got[keep] - ref[keep]).abs().max().item()
        print(f"{what}, other pixels: err {err:.3e}, tol {tol:.0e} * {scale:.3e}")
        assert err <= tol * scale, f"{what}, other pixels: max err {err:.3e} > {tol:.0e} * {scale:.3e}"
    return err


def rows_are_visible(ref, rows, tol, what):
    """losing one of `rows` (its output row left unwritten: zero, or whatever was there) moves a row-wise output by
    the row's own size: at least 10 x the tolerance"""
    scale = ref.abs().max().item()
    for p in rows:
        assert ref[p].abs().max().item() >= 10 * tol * scale, (what, p, ref[p].abs().max().item(), scale)


def dxtol(dt):
    return 1e-4 if dt == torch.float32 else ATOL[dt]


def sentinels(case, plan):
    """pixel 0, the last pixel of the first trip and the first of the second of every loop the case's parts run, and the
    last pixel"""
    n = hc.npix(case)
    s = {0, n - 1}
    if case.parts == "fwd":
        s |= {plan["fwd_grid"] * 256 - 1, plan["fwd_grid"] * 256}
    elif case.parts == "dx":
        per_pixel = case.C // (32 if plan["dx_kernel"] == 1 else 8)
        s |= {(plan["dx_grid"] * 256 - 1) // per_pixel, plan["dx_grid"] * 256 // per_pixel}
    elif case.parts == "dw":
        s |= {plan["dw_rows"] - 1, plan["dw_rows"]}  # block 0: row r of its pixels goes to thread row r % dw_rows
    elif case.parts == "mc":
        s |= {plan["fwd_grid"] * plan["fwd_waves"] * 32 - 1, plan["fwd_grid"] * plan["fwd_waves"] * 32}
        if plan["dx_trips"] >= 2:
            s |= {plan["dx_grid"] * 128 - 1, plan["dx_grid"] * 128}
    else:
        return []
    assert all(0 <= p < n for p in s) and len(s) >= 4, (s, n)
    return sorted(s)


@functools.lru_cache(maxsize=1)
def head_problem(case):
    """inputs (f64, rounded to the storage type) and the f64 autograd reference of a head case, built once"""
    n, dt = hc.npix(case), DT[case.dtype]
    gen = torch.Generator().manual_seed(1000 * case.C + case.K + n)
    plan = hc.plan(case)
    sent = sentinels(case, plan)
    w = rnd(case.K, case.C, gen=gen).float().double() / 4
    b = rnd(case.K, gen=gen).float().double() / 4 if case.bias else None
    dl = rnd(n, case.K, gen=gen).float().double()
    c0, k0 = case.C - 3, case.K - 1
    for i, p in enumerate(sent):
        dl[p, k0] = MARK if i % 2 else -MARK
    P = dict(case=case, plan=plan, sent=sent, w=w, b=b, dl=dl, n=n, dt=dt, c0=c0, k0=k0)
    if case.parts == "dx":  # the data gradient reads no x: none is built, and the reference goes chunk by chunk
        return P
    x = rnd(n, case.C, gen=gen).to(dt).double()
    for p in sent:
        x[p, c0] = MARK
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = (b if case.bias else torch.zeros(case.K, dtype=torch.float64)).clone().requires_grad_(True)
    logits = F.linear(xr, wr, br)
    logits.backward(dl)
    P.update(x=x, logits=logits.detach(), dx=xr.grad, dw=wr.grad, db=br.grad)
    if sent:
        # each sentinel dropped in turn: the parameter gradients (sums over the pixels) move by its product, the
        # row-wise outputs by its row
        for p in sent:
            ddw, ddb = torch.outer(dl[p], x[p]).abs().max().item(), dl[p].abs().max().item()
            assert ddw >= 10 * 1e-4 * P["dw"].abs().max().item(), (p, ddw, P["dw"].abs().max().item())
            assert ddb >= 10 * 1e-4 * P["db"].abs().max().item(), (p, ddb, P["db"].abs().max().item())
        rows_are_visible(P["logits"], sent, 1e-5, "logits")
        rows_are_visible(P["dx"], sent, dxtol(dt), "dx")
    return P


def gpu_inputs(P):
    case = P["case"]
    xd = to_map(P["x"], case.shape, P["dt"])
    wd = P["w"].float().to(DEV).view(case.K, case.C, 1, 1)
    bd = P["b"].float().to(DEV) if case.bias else None
    gd = to_map(P["dl"], case.shape, torch.float32)
    return xd, wd, bd, gd


@pytest.fixture
def ws_sizes(monkeypatch):
    """the workspace sizes the binding asks torch for, in call order"""
    ops = _ops()
    seen, real = [], ops._ws
    monkeypatch.setattr(ops, "_ws", lambda nbytes, device: (seen.append(int(nbytes)), real(nbytes, device))[1])
    return seen


SMALL_CASES = [c for c in hc.HEAD_CASES if c.parts == "all"]
TRIP_CASES = [c for c in hc.HEAD_CASES if c.parts != "all"]


@pytest.mark.parametrize("case", SMALL_CASES, ids=hc.case_id)
def test_head_every_branch(case, ws_sizes):
    """forward; backward with (dx, dw), dx alone, dw alone -- bit-equal where they overlap; the accumulating form"""
    ops = _ops()
    P = head_problem(case)
    K, C, dt, plan = case.K, case.C, P["dt"], P["plan"]
    xd, wd, bd, gd = gpu_inputs(P)
    out = ops.head_fwd(xd, wd, bd)
    assert tuple(out.shape) == (case.shape[0], K, case.shape[1], case.shape[2]) and out.dtype == torch.float32
    check(to_rows(out), P["logits"], 1e-5, "logits")
    dx, dw, db = ops.head_bwd(xd, wd, gd, True, True)
    assert ws_sizes == [plan["ws_bytes"]], (ws_sizes, plan)
    assert dx.shape == xd.shape and dx.dtype == dt and tuple(dw.shape) == (K, C, 1, 1) and tuple(db.shape) == (K,)
    check(dw, P["dw"], 1e-4, "dw")
    check(db, P["db"], 1e-4, "db")
    check(to_rows(dx), P["dx"], dxtol(dt), "dx")
    dx1, none_w, none_b = ops.head_bwd(xd, wd, gd, True, False)
    assert none_w is None and none_b is None and torch.equal(dx1, dx)
    none_x, dw1, db1 = ops.head_bwd(xd, wd, gd, False, True)
    assert none_x is None and torch.equal(dw1, dw) and torch.equal(db1, db)
    sink_w, sink_b = torch.ones(K, C, device=DEV), torch.full((K,), 2.0, device=DEV)
    dx2, _, _ = ops.head_bwd(xd, wd, gd, True, True, dw_into=sink_w.view(-1), db_into=sink_b)
    torch.cuda.synchronize()
    assert torch.equal(dx2, dx)
    check(sink_w - 1, P["dw"], 1e-4, "dw into")
    check(sink_b - 2, P["db"], 1e-4, "db into")
    assert ws_sizes == [plan["ws_bytes"]] * 3 and plan["fwd_trips"] == plan["dx_trips"] == 1


def _losses_on(logits_rows, case, gen):
    """softmax-KL and softmax-MSE, forward and backward, on 4 x the head's logits of a second-trip case.  The forward
    kernels (1024 blocks) make three trips at this size and the backward kernels (2048 blocks) two, so the sentinels
    sit on both boundaries."""
    ops = _ops()
    n, K = logits_rows.shape
    sent = sorted({0, 1024 * 256 - 1, 1024 * 256, 2048 * 256 - 1, 2048 * 256, n - 1})
    gs = torch.ones(1, device=DEV)
    z = (logits_rows * 4).float()
    z[sent] = (rnd(len(sent), K, gen=gen) * 2).float()  # (the head's own sentinel rows are saturated: ordinary rows instead)
    tgt = z.argmax(1)
    # KL.  A pixel can add at most -log(eps) / npix to the mean: 7.0e-5 with the training loop's eps = 1e-16, below
    # 10 x the tolerance whatever its logits are.  So the sentinels are judged at eps = 0, where logits that put
    # e^-74 / (K - 1) on the target add 1.4e-4 each (and their gradient rows are the largest there are); eps = 1e-16
    # runs as well, for parity alone.
    zk = z.clone()
    for i, p in enumerate(sent):
        tgt[p] = i % K
        zk[p] = 0.0
        zk[p, i % K] = -74.0
    for eps in (0.0, 1e-16):
        zr = zk.double().requires_grad_(True)
        pt = torch.softmax(zr, 1).gather(1, tgt[:, None])[:, 0]
        per_pixel = -torch.log((pt + eps) / (1 + eps))
        ref = per_pixel.mean()
        ref.backward()
        tol = 1e-5 * max(1.0, abs(ref.item()))
        if eps == 0.0:
            for p in sent:  # dropped in turn
                assert per_pixel[p].item() / n >= 10 * tol, (p, per_pixel[p].item() / n, tol)
            rows_are_visible(zr.grad, sent, 1e-4, "KL dlogits")
        zd, td = to_map(zk, case.shape, torch.float32), tgt.to(DEV).view(case.shape)
        loss = ops.softmax_kl_fwd(zd, td, eps).item()
        print(f"KL eps {eps:g}: {loss:.8f} vs {ref.item():.8f}, tol {tol:.1e}")
        assert abs(loss - ref.item()) <= tol, (eps, loss, ref.item())
        check(to_rows(ops.softmax_kl_bwd(zd, td, gs, eps)), zr.grad, 1e-4, f"KL dlogits eps {eps:g}", sent)
    # MSE of two softmaxes: a pixel adds at most 2 / (npix K) to the mean, a tenth of the tolerance, so no marker can
    # make one lost pixel visible in the scalar.  Instead each sentinel (one-hot rows on two different classes: the
    # largest a pixel can add) is taken out in turn ON THE GPU, and the difference of the two results -- the kernel
    # sums per-block f64 partials in a fixed order, so everything else cancels up to the rounding of two f32 results
    # -- must be the sentinel's term of the reference to within a tenth.
    a, b = z.clone(), (rnd(n, K, gen=gen) * 2).float()
    ar, br = a.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = ((torch.softmax(ar, 1) - torch.softmax(br, 1)) ** 2).mean()
    ref.backward()
    ad, bd = to_map(a, case.shape, torch.float32), to_map(b, case.shape, torch.float32)
    rows_are_visible(ar.grad, sent, 1e-4, "MSE da"), rows_are_visible(br.grad, sent, 1e-4, "MSE db")
    da, db = ops.softmax_mse_bwd(ad, bd, gs, True, True)
    check(to_rows(da), ar.grad, 1e-4, "MSE da", sent), check(to_rows(db), br.grad, 1e-4, "MSE db", sent)
    da1, none = ops.softmax_mse_bwd(ad, bd, gs, True, False)
    assert none is None and torch.equal(da1, da)
    for i, p in enumerate(sent):
        a[p], b[p] = 0.0, 0.0
        a[p, i % K], b[p, (i + 1) % K] = 40.0, 40.0
    terms = ((torch.softmax(a.double(), 1) - torch.softmax(b.double(), 1)) ** 2).sum(1)
    ref = terms.sum().item() / (n * K)
    tol = 1e-5 * max(1.0, abs(ref))
    ad, bd = to_map(a, case.shape, torch.float32), to_map(b, case.shape, torch.float32)
    full = ops.softmax_mse_fwd(ad, bd).item()
    print(f"MSE: {full:.9f} vs {ref:.9f}, tol {tol:.1e}")
    assert abs(full - ref) <= tol
    arows = ad.permute(0, 2, 3, 1).reshape(n, K)  # (a view of the GPU tensor)
    for p in sent:
        keep = arows[p].clone()
        arows[p] = bd.permute(0, 2, 3, 1).reshape(n, K)[p]  # equal rows: the pixel adds nothing
        without = ops.softmax_mse_fwd(ad, bd).item()
        arows[p] = keep
        term = terms[p].item() / (n * K)
        assert 0.1 * term >= 2 * 2.0 ** -23 * ref  # (the allowance is at least two ulp of an f32 result)
        assert abs((full - without) - term) <= 0.1 * term, (p, full, without, term)


@pytest.mark.parametrize("case", TRIP_CASES, ids=hc.case_id)
def test_head_past_the_launch_caps(case, ws_sizes):
    """the part of the head a second-trip case is there for, with sentinel pixels on the loop boundaries"""
    ops = _ops()
    P = head_problem(case)
    K, C, dt, plan, sent, n = case.K, case.C, P["dt"], P["plan"], P["sent"], P["n"]
    wd = P["w"].float().to(DEV).view(K, C, 1, 1)
    bd = P["b"].float().to(DEV)
    gd = to_map(P["dl"], case.shape, torch.float32)
    print(f"{hc.case_id(case)}: sentinels {sent}, plan {plan}")
    if case.parts == "dx":
        assert plan["dx_trips"] >= 2
        xd = torch.zeros((case.shape[0], case.shape[1], case.shape[2], C), dtype=dt, device=DEV).permute(0, 3, 1, 2)
        dx, _, _ = ops.head_bwd(xd, wd, gd, True, False)
        assert ws_sizes == [] and dx.shape == xd.shape and dx.dtype == dt
        got = dx.permute(0, 2, 3, 1).reshape(n, C)
        tol, stats = dxtol(dt), []
        for lo in range(0, n, 1 << 16):  # the f64 reference, 65 536 pixels at a time
            hi = min(n, lo + (1 << 16))
            xr = torch.zeros(hi - lo, C, dtype=torch.float64, requires_grad=True)
            F.linear(xr, P["w"]).backward(P["dl"][lo:hi])
            g = got[lo:hi].cpu().double()
            marked = [p - lo for p in sent if lo <= p < hi]
            keep = torch.ones(hi - lo, dtype=torch.bool)
            keep[marked] = False
            stats.append(((g - xr.grad).abs().max().item(), xr.grad.abs().max().item(),
                          (g - xr.grad)[keep].abs().max().item(), xr.grad[keep].abs().max().item(),
                          min([xr.grad[p].abs().max().item() for p in marked], default=float("inf"))))
        err, scale, err_o, scale_o, smallest = (f(s[i] for s in stats) for i, f in enumerate((max, max, max, max, min)))
        print(f"dx: err {err:.3e}, tol {tol:.0e} * {scale:.3e}; other pixels: err {err_o:.3e}, tol {tol:.0e} * {scale_o:.3e}")
        assert smallest >= 10 * tol * scale  # a lost sentinel row moves dx by its own size
        assert err <= tol * scale and err_o <= tol * scale_o
        return
    xd = to_map(P["x"], case.shape, dt)
    if case.parts == "dw":
        assert plan["dw_per"] > 256 and plan["dw_blocks"] > 1
        _, dw, db = ops.head_bwd(xd, wd, gd, False, True)
        assert ws_sizes == [plan["ws_bytes"]]
        check(dw, P["dw"], 1e-4, "dw"), check(db, P["db"], 1e-4, "db")
        sink_w, sink_b = torch.ones(K, C, device=DEV), torch.full((K,), 2.0, device=DEV)
        ops.head_bwd(xd, wd, gd, False, True, dw_into=sink_w.view(-1), db_into=sink_b)
        check(sink_w - 1, P["dw"], 1e-4, "dw into"), check(sink_b - 2, P["db"], 1e-4, "db into")
        return
    assert plan["fwd_trips"] >= 2
    out = ops.head_fwd(xd, wd, bd)
    rows = to_rows(out)
    check(rows, P["logits"], 1e-5, "logits", sent)
    if case.parts == "fwd":
        _losses_on(rows, case, torch.Generator().manual_seed(K))
        return
    dx, dw, db = ops.head_bwd(xd, wd, gd, True, True)  # "mc"
    assert ws_sizes == [plan["ws_bytes"]]
    check(dw, P["dw"], 1e-4, "dw"), check(db, P["db"], 1e-4, "db")
    check(to_rows(dx), P["dx"], dxtol(dt), "dx", sent)
    dx1, _, _ = ops.head_bwd(xd, wd, gd, True, False)
    _, dw1, db1 = ops.head_bwd(xd, wd, gd, False, True)
    assert torch.equal(dx1, dx) and torch.equal(dw1, dw) and torch.equal(db1, db)


@pytest.mark.parametrize("case", hc.CLUSTER_CASES, ids=hc.case_id)
def test_cluster_head_softmax_mode(case):
    """cy_cluster_head_fwd / _bwd past both forward caps and the backward's, and around one 32-pixel tile.  Sentinels of
    the second-trip cases: x = 8 in one channel (64 would saturate every softmax of the pixel and leave no gradient),
    dprobs = 64^2 in one cluster."""
    ops = _ops()
    M, C, S, k, dt, Tt = case.M, case.C, case.S, case.k, DT[case.dtype], case.T
    K = S * k
    plan = ops.cluster_head_plan(M, C, S, k)
    gen = torch.Generator().manual_seed(M + K)
    x = rnd(M, C, gen=gen).to(dt).double()
    w, b = (rnd(K, C, gen=gen) * 0.3).float().double(), (rnd(K, gen=gen) * 0.1).float().double()
    g = rnd(S, M, k, gen=gen).float().double()
    sent = []
    if plan["fwd_trips"] >= 2:
        edge = plan["fwd_grid"] * plan["fwd_waves"] * 32
        sent = sorted({0, edge - 1, edge, M - 1} | ({plan["bwd_grid"] * 128 - 1, plan["bwd_grid"] * 128}
                                                    if plan["bwd_trips"] >= 2 else set()))
        for i, p in enumerate(sent):
            x[p, C - 3] = 8.0
            g[S - 1, p, i % k] = MARK * MARK
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = torch.softmax((xr @ wr.t() + br).view(M, S, k) / Tt, dim=2).permute(1, 0, 2)
    (ref * g).sum().backward()
    ref = ref.detach()
    if sent:
        z = (x @ w.t() + b).view(M, S, k).requires_grad_(True)
        (torch.softmax(z / Tt, dim=2).permute(1, 0, 2) * g).sum().backward()
        dl = z.grad.view(M, K)
        for p in sent:  # dropped in turn
            assert torch.outer(dl[p], x[p]).abs().max().item() >= 10 * 1e-4 * wr.grad.abs().max().item(), p
            assert dl[p].abs().max().item() >= 10 * 1e-4 * br.grad.abs().max().item(), p
        rows_are_visible(xr.grad, sent, dxtol(dt), "dx")
        rows_are_visible(ref.permute(1, 0, 2).reshape(M, K), sent, 1e-5, "probs")
    xd, wd, bd, gd = x.to(dt).to(DEV), w.float().to(DEV), b.float().to(DEV), g.float().to(DEV)
    probs = ops.cluster_head_fwd(xd, wd, bd, S, k, Tt)
    assert tuple(probs.shape) == (S, M, k)
    check(probs, ref, 1e-5, "probs")
    dx, dw, db = ops.cluster_head_bwd(xd, wd, probs, gd, Tt, True, True)
    print(f"{hc.case_id(case)}: sentinels {sent}, plan {plan}")
    check(dw, wr.grad, 1e-4, "dw"), check(db, br.grad, 1e-4, "db")
    check(dx, xr.grad, dxtol(dt), "dx", sent)
    dx2, dw2, db2 = ops.cluster_head_bwd(xd, wd, probs, gd, Tt, True, True)
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and torch.equal(dx, dx2)
    assert torch.equal(ops.cluster_head_fwd(xd, wd, bd, S, k, Tt), probs)
    dx3, _, _ = ops.cluster_head_bwd(xd, wd, probs, gd, Tt, True, False)
    assert torch.equal(dx3, dx)


@pytest.mark.parametrize("N,H,W,K", hc.DICE_CASES)
def test_dice_counts_past_the_cap(N, H, W, K):
    """64 blocks per sample: HW > 16 384 sends threads round again.  Sentinels (per sample: pixel 0, 16 383, 16 384, the
    last) predict a class no other pixel predicts, so the counts of that class are the sentinels alone; a few pixels
    have exactly tied top logits, which go to the lowest class index as argmax does."""
    ops = _ops()
    HW = H * W
    gen = torch.Generator().manual_seed(K)
    z = rnd(N, HW, K, gen=gen).float()
    z[:, :, K - 1] = -5.0
    tgt = torch.randint(0, K, (N, HW), generator=gen)
    sent = [0, 64 * 256 - 1, 64 * 256, HW - 1]
    for n in range(N):
        for i, p in enumerate(sent):
            z[n, p, K - 1] = 5.0
            tgt[n, p] = K - 1 if i % 2 else 0
        z[n, 100] = 0.0                    # all tied: class 0
        z[n, 16500, :] = -1.0
        z[n, 16500, 1:3] = 2.0             # classes 1 and 2 tied on top: class 1
    pred = z.double().argmax(2)
    assert (pred[:, 100] == 0).all() and (pred[:, 16500] == 1).all()
    ref = torch.zeros(N, K, 2, dtype=torch.int64)
    for k in range(K):
        ref[:, k, 0] = ((pred == k) & (tgt == k)).sum(1)
        ref[:, k, 1] = (pred == k).sum(1) + (tgt == k).sum(1)
    assert (ref[:, K - 1, 0] == 2).all() and ((pred == K - 1).sum(1) == 4).all()  # each sentinel counts once
    zd = z.to(DEV).view(N, H, W, K).permute(0, 3, 1, 2)
    got = ops.dice_counts(zd, tgt.to(DEV).view(N, H, W)).cpu()
    assert torch.equal(got, ref), (got, ref)


# ---------------------------------------------------------------- projection head
PROJ_CASES = [  # B, HW (H, W), C, hid, out, dtype
    (1, (1, 1), 8, 4, 1, "f32"),        # minimal
    (3, (7, 7), 40, 36, 10, "bf16"),    # ragged: nothing a multiple of 64, out < 16 (waves without rows in the backward)
    (2, (7, 1), 24, 260, 65, "f32"),    # hid > 256: second pass of the lane loop; HW < the 16 pooling slices
    (4, (20, 15), 128, 256, 256, "bf16"),
    (5, (14, 14), 512, 512, 512, "f16"),  # the maxima
    (2, (5, 1), 16, 8, 3, "f16"),
]


def _proj_reference(x, w1, b1, w2, b2, gz):
    leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    xr, w1r, b1r, w2r, b2r = leaves
    z = F.normalize(F.linear(F.leaky_relu(F.linear(xr.mean((2, 3)), w1r, b1r), .01), w2r, b2r), dim=1)
    (z * gz).sum().backward()
    return z.detach(), [t.grad for t in leaves]


def _proj_check(B, hw, C, hid, out, dtname, zero_w2=False):
    ops = _ops()
    dt = DT[dtname]
    H, W = hw
    gen = torch.Generator().manual_seed(B * 1000 + hid + out)
    x = rnd(B, C, H, W, gen=gen).to(dt).double()
    w1, b1 = (rnd(hid, C, gen=gen) / C ** 0.5).float().double(), (rnd(hid, gen=gen) / 4).float().double()
    w2, b2 = (rnd(out, hid, gen=gen) / hid ** 0.5).float().double(), (rnd(out, gen=gen) / 4).float().double()
    if zero_w2:
        w2, b2 = torch.zeros_like(w2), torch.zeros_like(b2)
    gz = rnd(B, out, gen=gen).float().double()
    z_ref, (dx_ref, dw1_ref, db1_ref, dw2_ref, db2_ref) = _proj_reference(x, w1, b1, w2, b2, gz)
    if zero_w2:  # every norm is 0: z = 0 and dy2 = dz / eps, as F.normalize's clamp gives
        assert z_ref.abs().max().item() == 0.0 and torch.allclose(db2_ref, gz.sum(0) / 1e-12, rtol=1e-12, atol=0)
    xd = x.to(dt).to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    w1d, b1d, w2d, b2d, gzd = (t.float().to(DEV) for t in (w1, b1, w2, b2, gz))
    ftol = 1e-4 if dt == torch.float32 else 1e-2
    refs = (dw1_ref, db1_ref, dw2_ref, db2_ref)
    floor = [0.0] * 5
    if out == 1:
        # z = y2 / |y2| = +-1 whatever y2 is: every gradient is exactly 0, the f64 reference holds rounding noise
        # (1e-16) and tol * max|ref| means nothing.  What f32 leaves of dy2 = dz / n - y2 (y2 dz) / n^3 is a few ulp of
        # its two equal terms, |dz| / n; the gradients are linear in dy2, so they may hold that times the gradients
        # of y2 itself (unit upstream), and no more.
        leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
        y2 = F.linear(F.leaky_relu(F.linear(leaves[0].mean((2, 3)), leaves[1], leaves[2]), .01), leaves[3], leaves[4])
        y2.sum().backward()
        resid = 4 * 2.0 ** -24 * (gz.abs() / y2.detach().abs()).max().item()
        floor = [resid * t.grad.abs().max().item() for t in leaves]
        assert all(r.abs().max().item() <= f for r, f in zip((dx_ref,) + refs, floor))
    # one launch per direction
    assert ops.proj_head_ok(xd, w1d, w2d)
    z, pooled, y1, y2, norms = ops.proj_head_fwd(xd, w1d, b1d, w2d, b2d)
    check(z, z_ref, 2e-5, "z")
    check(pooled, x.mean((2, 3)), 1e-5, "pooled")
    dx, grads = ops.proj_head_bwd(gzd, pooled, y1, y2, norms, w1d, w2d, tuple(xd.shape), dt, True)
    assert dx.dtype == dt and ops.is_nhwc(dx)
    for got, ref, name, fl in zip(grads, refs, ("dw1", "db1", "dw2", "db2"), floor[1:]):
        check(got, ref, 1e-4, name, floor=fl)
    check(dx, dx_ref, ftol, "dfeat", floor=floor[0])
    sinks = tuple(torch.ones_like(t) for t in grads)
    dx2, nones = ops.proj_head_bwd(gzd, pooled, y1, y2, norms, w1d, w2d, tuple(xd.shape), dt, False, sinks)
    assert dx2 is None and nones == (None, None, None, None)
    for got, ref, name, fl in zip(sinks, refs, ("dw1", "db1", "dw2", "db2"), floor[1:]):
        # (the sink holds 1 + gradient in f32: half an ulp of that sum is allowed on top)
        g = got.detach().cpu().double() - 1
        bound = 1e-4 * ref.abs().max().item() + 2.0 ** -24 * (1 + ref.abs().max().item()) + fl
        assert (g - ref).abs().max().item() <= bound, (name, (g - ref).abs().max().item(), bound)
    # the separate kernels
    p0 = ops.avgpool_fwd(xd)
    h0 = ops.linear_fwd(p0, w1d, b1d, 1, 0.01)
    o0 = ops.linear_fwd(h0, w2d, b2d, 0, 0.0)
    z0, n0 = ops.l2norm_fwd(o0)
    check(z0, z_ref, 2e-5, "z (separate kernels)")
    do = ops.l2norm_bwd(o0, n0, gzd)
    dh, rw2, rb2 = ops.linear_bwd(h0, w2d, o0, do, 0, 0.0, True, True)
    dp, rw1, rb1 = ops.linear_bwd(p0, w1d, h0, dh, 1, 0.01, True, True)
    rx = ops.avgpool_bwd(dp, tuple(xd.shape), dt)
    for got, ref, name, fl in zip((rw1, rb1, rw2, rb2), refs, ("dw1", "db1", "dw2", "db2"), floor[1:]):
        check(got, ref, 1e-4, name + " (separate kernels)", floor=fl)
    check(rx, dx_ref, ftol, "dfeat (separate kernels)", floor=floor[0])


@pytest.mark.parametrize("B,hw,C,hid,out,dtname", PROJ_CASES)
def test_projection_head_against_float64(B, hw, C, hid, out, dtname):
    _proj_check(B, hw, C, hid, out, dtname)


def test_projection_head_zero_norm_branch():
    """w2 = 0, b2 = 0: every norm is 0 <= eps, the output is 0 and the backward is dz / eps"""
    _proj_check(3, (3, 2), 24, 36, 10, "f32", zero_w2=True)


def test_linear_kernels_at_sizes_that_are_no_multiple_of_four():
    """cy_linear_fwd / _bwd with I = 7 and M * O = 15, both activations"""
    ops = _ops()
    gen = torch.Generator().manual_seed(7)
    M, I, O = 3, 7, 5
    x, w, b, gy = (rnd(*s, gen=gen).float().double() for s in ((M, I), (O, I), (O,), (M, O)))
    for act in (0, 1):
        xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
        y = F.linear(xr, wr, br)
        y = F.leaky_relu(y, 0.01) if act else y
        y.backward(gy)
        xd, wd, bd, gd = (t.float().to(DEV) for t in (x, w, b, gy))
        yd = ops.linear_fwd(xd, wd, bd, act, 0.01)
        check(yd, y.detach(), 1e-5, f"linear act {act}")
        dx, dw, db = ops.linear_bwd(xd, wd, yd, gd, act, 0.01, True, True)
        check(dx, xr.grad, 1e-4, "dx"), check(dw, wr.grad, 1e-4, "dw"), check(db, br.grad, 1e-4, "db")
        sw, sb = torch.ones(O, I, device=DEV), torch.full((O,), 2.0, device=DEV)
        ops.linear_bwd(xd, wd, yd, gd, act, 0.01, False, True, dw_into=sw, db_into=sb)
        check(sw - 1, wr.grad, 1e-4, "dw into"), check(sb - 2, br.grad, 1e-4, "db into")
