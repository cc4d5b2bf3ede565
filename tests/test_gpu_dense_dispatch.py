"""Parity of the dense projector at entry-point level -- cy_dense_proj_fwd / _bwd in their three forms (VALU,
register-resident and streamed matrix-core kernels), the adaptive pools and the row gather -- over the case table of
tests/dense_proj_cases.py: non-square maps, one job and one-pixel bins, bins of 400 pixels, past every launch cap, a
long bin list, null outputs, `accumulate`, a pixel stride above C.  tests/test_dense_proj_coverage.py checks on the CPU
that the table reaches those branches and that the bounds used here see the faults the cases exist for.

The reference is float64 torch on the CPU (dense_proj_cases.reference).  Bounds, relative to the reference tensor's
largest magnitude (dense_proj_cases.bounds): 16-bit forms hpool 1e-4, dW1 / db1 3e-3, dx 1e-2; f32 1e-4 and 2e-4.  dx
is also compared per pixel class -- pixels of one, two, (three,) four of the case's bins -- each against its own
maximum, and is exactly zero at pixels of no listed bin.  Every output and the workspace are NaN-filled before each call
(dx: zeroed, as the header asks, except where the all-bins matrix-core form writes every pixel exactly once), and a
guard band on both sides of every output must come back bit-unchanged.  Every figure is printed before it is asserted."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import dense_proj_cases as dc

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 256       # elements on each side of an output
PAD_MARK = 3.0    # what the padding columns of dx hold before the call


class Guarded:
    """`n` elements of `dtype` holding `fill`, with GUARD elements of a pattern on both sides"""

    def __init__(self, n, dtype, fill):
        self.all = torch.full((n + 2 * GUARD,), -5.0 if dtype != torch.uint8 else 0x5A, dtype=dtype, device=DEV)
        self.t = self.all[GUARD:GUARD + n]
        self.t.fill_(fill)
        self.before = (self.all[:GUARD].clone(), self.all[GUARD + n:].clone())

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        n = self.t.numel()
        raw = lambda v: v.view(torch.uint8) if v.dtype != torch.uint8 else v  # noqa: E731
        return all(torch.equal(raw(a), raw(b)) for a, b in zip(self.before, (self.all[:GUARD], self.all[GUARD + n:])))


def writes_every_pixel_once(c):
    """the all-bins matrix-core backward: one job per cell of the bin partition, dx stored and not accumulated"""
    return c.inst.form in ("reg", "stream") and not dc.GEOMS[c.geom].listed


def run(c, ldx_pad=0, want_dx=True, want_dw=True, want_db=True, accumulate=0, forward=True):
    """cy_dense_proj_fwd and cy_dense_proj_bwd through _lib.call -> CPU tensors and `guards` (all intact)"""
    from cyhip import _lib, ops
    g, i = dc.GEOMS[c.geom], c.inst
    t = dc.inputs(c, ldx_pad)
    T = dc.DTYPES[i.dtype]
    ldx, nb = i.C + ldx_pad, dc.num_bins(c.geom)
    x, w1, b1, dh = (t[k].to(DEV).contiguous() for k in ("x", "w1", "b1", "dh"))
    bins = dc.bin_list(c.geom)
    bins = None if bins is None else bins.to(DEV)
    bp = None if bins is None else bins.data_ptr()
    args = (g.N, g.H, g.W, i.C, ldx, i.hid, g.sh, g.sw, i.slope, ops.dtype_code(T))
    nan = float("nan")
    out, held = {}, []
    if forward:
        hpool = Guarded(nb * i.hid, torch.float32, nan)
        _lib.call("cy_dense_proj_fwd", x.data_ptr(), w1.data_ptr(), b1.data_ptr(), bp, nb, hpool.ptr(), *args, ops._stream())
        out["hpool"] = hpool.t.view(nb, i.hid).cpu()
        held.append(hpool)
    dx = dw = db = None
    if want_dx:
        dx = Guarded(g.N * g.H * g.W * ldx, T, PAD_MARK)
        dx.t.view(g.N, g.H, g.W, ldx)[..., :i.C] = nan if writes_every_pixel_once(c) else 0.0
        held.append(dx)
    if want_dw:
        dw = Guarded(i.hid * i.C, torch.float32, nan)
        if accumulate:
            dw.t.copy_(t["pre_dw"].reshape(-1))
        held.append(dw)
    if want_db:
        db = Guarded(i.hid, torch.float32, nan)
        if accumulate:
            db.t.copy_(t["pre_db"])
        held.append(db)
    nbytes = _lib.load().cy_dense_proj_bwd_ws_bytes(nb, i.C, i.hid)
    ws = Guarded(nbytes, torch.uint8, 0xFF)  # (all ones: a NaN as f32, -1 as a job record's integers)
    held.append(ws)
    p = lambda v: None if v is None else v.ptr()  # noqa: E731
    _lib.call("cy_dense_proj_bwd", x.data_ptr(), w1.data_ptr(), b1.data_ptr(), bp, nb, dh.data_ptr(), p(dx), p(dw), p(db),
              accumulate, *args, ws.ptr(), nbytes, ops._stream())
    torch.cuda.synchronize()
    if dx is not None:
        full = dx.t.view(g.N, g.H, g.W, ldx).cpu()
        out["dx"], out["dx_pad"] = full[..., :i.C].contiguous(), full[..., i.C:].contiguous()
    if dw is not None:
        out["dw1"] = dw.t.view(i.hid, i.C).cpu()
    if db is not None:
        out["db1"] = db.t.cpu()
    out["guards"] = all(h.intact() for h in held)
    return out


def check(c, out, ref, keys):
    """print every figure, then assert all of them"""
    bar = dc.bounds(c.inst.dtype)
    fig, ok = [], True
    for k in keys:
        finite = bool(out[k].isfinite().all())
        err = dc.rel_err(out[k], ref[k]) if finite else float("inf")
        fig.append(f"{k} {err:.2e} (bound {bar[k]:.0e})")
        ok &= finite and err <= bar[k]
    if "dx" in keys and out["dx"].isfinite().all():
        for n, err in dc.class_errors(c.geom, out["dx"], ref["dx"]).items():
            fig.append(f"dx at pixels of {n} bin(s) {err:.2e} (bound {bar['dx']:.0e})")
            ok &= err <= bar["dx"]
        outside = dc.cover(c.geom) == 0
        if outside.any():
            worst = float(out["dx"][outside].float().abs().max())
            fig.append(f"dx at pixels of no listed bin: largest magnitude {worst:.1e} (must be 0)")
            ok &= worst == 0.0
    print(f"{dc.case_id(c)}: " + "; ".join(fig) + f"; guards intact: {out['guards']}")
    assert ok and out["guards"], (dc.case_id(c), fig)


ALL = ("hpool", "dx", "dw1", "db1")


@pytest.mark.parametrize("c", dc.CASES, ids=dc.case_id)
def test_dense_projector_parity(c):
    """one_bin on the register-resident bf16 form is the case that found the coherent rounding of the pooled gradient
    in the dW1 kernel (3.12e-3 against 3e-3 before the gradient went into the product as two 16-bit terms): with one bin
    every pixel of a hidden unit carries the same gradient, so its rounding error does not average out over the sum."""
    assert dc.form_of(c.inst) == c.inst.form  # a silent change of form fails here instead of passing
    out = run(c)
    check(c, out, dc.reference(c), ALL)
    if c.geom in dc.TWICE:  # several jobs per wave: the job -> wave assignment and the reduction order are fixed
        again = run(c)
        same = {k: torch.equal(out[k].view(torch.uint8), again[k].view(torch.uint8)) for k in ALL}
        print("second run bit-equal:", same)
        assert all(same.values()), same
    if c.geom == "nonsquare_a":  # cyhip.ops reaches the same entry points with the same arguments
        from cyhip import ops
        t = dc.inputs(c)
        x = t["x"].to(DEV).permute(0, 3, 1, 2)
        w1, b1, dh = t["w1"].to(DEV), t["b1"].to(DEV), t["dh"].to(DEV)
        g = dc.GEOMS[c.geom]
        hp = ops.dense_proj_fwd(x, w1, b1, (g.sh, g.sw), None, c.inst.slope)
        dx, dw, db = ops.dense_proj_bwd(x, w1, b1, (g.sh, g.sw), None, dh, True, True, c.inst.slope)
        same = dict(hpool=torch.equal(hp.cpu(), out["hpool"]), dx=torch.equal(dx.permute(0, 2, 3, 1).cpu(), out["dx"]),
                    dw1=torch.equal(dw.cpu(), out["dw1"]), db1=torch.equal(db.cpu(), out["db1"]))
        print("cyhip.ops bit-equal:", same)
        assert all(same.values()), same


@pytest.mark.parametrize("c", dc.OPTION_CASES, ids=dc.case_id)
def test_dense_projector_options(c):
    ref = dc.reference(c)
    plain = run(c)
    check(c, plain, ref, ALL)
    # dx alone, the parameter gradients alone (the other pointers null), dW1 alone and db1 alone
    only_dx = run(c, want_dw=False, want_db=False, forward=False)
    check(c, only_dx, ref, ("dx",))
    only_par = run(c, want_dx=False, forward=False)
    check(c, only_par, ref, ("dw1", "db1"))
    only_dw = run(c, want_dx=False, want_db=False, forward=False)
    check(c, only_dw, ref, ("dw1",))
    only_db = run(c, want_dx=False, want_dw=False, forward=False)
    check(c, only_db, ref, ("db1",))
    same = dict(dx=torch.equal(only_dx["dx"], plain["dx"]), dw1=torch.equal(only_par["dw1"], plain["dw1"]),
                db1=torch.equal(only_par["db1"], plain["db1"]), dw1_alone=torch.equal(only_dw["dw1"], plain["dw1"]),
                db1_alone=torch.equal(only_db["db1"], plain["db1"]))
    print("outputs asked for alone, bit-equal to the full call:", same)
    assert all(same.values()), same
    # accumulate: one f32 addition onto the pre-fill
    t = dc.inputs(c)
    acc = run(c, accumulate=1, forward=False)
    same = dict(dw1=torch.equal(acc["dw1"], t["pre_dw"] + plain["dw1"]), db1=torch.equal(acc["db1"], t["pre_db"] + plain["db1"]),
                dx=torch.equal(acc["dx"], plain["dx"]))
    print("accumulate = pre-fill + gradient, bit-equal:", same, "guards intact:", acc["guards"])
    assert all(same.values()) and acc["guards"], same
    # a pixel stride above C: NaN in the padding columns of x, the padding of dx untouched
    wide = run(c, ldx_pad=dc.LDX_PAD)
    check(c, wide, dc.reference(c, dc.LDX_PAD), ALL)
    untouched = bool((wide["dx_pad"].float() == PAD_MARK).all())
    print("padding columns of dx untouched:", untouched)
    assert untouched and wide["dx_pad"].shape[-1] == dc.LDX_PAD


# ------------------------------------------------------------------------------------------------ pools and gather
def nchw_view(x):
    return x.to(DEV).permute(0, 3, 1, 2)  # NHWC memory


@pytest.mark.parametrize("p", dc.AVG_FWD, ids=dc.pool_id)
def test_adaptive_avgpool_forward(p):
    from cyhip import ops
    x, _ = dc.avg_inputs(p)
    want, bound = dc.avg_fwd_reference(p)
    bins = dc.pool_bins(p).to(DEV) if p.listed else None
    got = ops.adaptive_avgpool_fwd(nchw_view(x), (p.sh, p.sw), bins).cpu().double()
    assert got.shape == want.shape
    excess = ((got - want).abs() - bound).max().item()
    print(f"{dc.pool_id(p)}: largest error {(got - want).abs().max():.3e}, largest error minus bound {excess:.3e}")
    assert got.isfinite().all() and excess <= 0


@pytest.mark.parametrize("p", dc.AVG_BWD, ids=dc.pool_id)
def test_adaptive_avgpool_backward(p):
    from cyhip import ops
    _, dpool = dc.avg_inputs(p)
    want, bound = dc.avg_bwd_reference(p)
    dx = ops.adaptive_avgpool_bwd(dpool.to(DEV), (p.N, p.C, p.H, p.W), dc.DTYPES[p.dtype], (p.sh, p.sw))
    got = dx.permute(0, 2, 3, 1).cpu().double()
    excess = ((got - want).abs() - bound).max().item()
    print(f"{dc.pool_id(p)}: largest error {(got - want).abs().max():.3e}, largest error minus bound {excess:.3e}")
    assert got.isfinite().all() and excess <= 0


@pytest.mark.parametrize("p", dc.MAX_CASES, ids=dc.pool_id)
def test_adaptive_maxpool_is_bit_equal(p):
    from cyhip import ops
    x, dpool = dc.max_inputs(p)
    rows, arg, dx = dc.max_reference(p)
    got, garg = ops.adaptive_maxpool_fwd(nchw_view(x), (p.sh, p.sw))
    gdx = ops.adaptive_maxpool_bwd(dpool.to(DEV), garg, (p.N, p.C, p.H, p.W), dc.DTYPES[p.dtype], (p.sh, p.sw))
    gdx = gdx.permute(0, 2, 3, 1).cpu()
    same = dict(values=torch.equal(got.cpu(), rows), arg=torch.equal(garg.cpu(), arg),
                dx=gdx.dtype == dc.DTYPES[p.dtype] and torch.equal(gdx.float(), dx))
    print(f"{dc.pool_id(p)}: bit-equal {same}; arg mismatches {(garg.cpu() != arg).sum().item()}")
    assert all(same.values()), same


@pytest.mark.parametrize("M,D", dc.GATHER)
def test_gather_and_scatter_rows_are_bit_equal(M, D):
    from cyhip import ops
    src, idx, dout = dc.gather_inputs(M, D)
    got = ops.gather_rows_fwd(src.to(DEV), idx.to(DEV)).cpu()
    assert torch.equal(got, src.index_select(0, idx.long()))
    R = src.shape[0]
    back = ops.gather_rows_bwd(dout.to(DEV), idx.to(DEV), R).cpu()
    want = torch.zeros(R, D).index_copy_(0, idx.long(), dout)
    assert torch.equal(back, want)
    rest = torch.ones(R, dtype=torch.bool)
    rest[idx.long()] = False
    assert rest.sum() == dc.GATHER_SPARE and (back[rest] == 0).all(), "rows not listed are exactly zero"


# ------------------------------------------------------------------------------------------------ head level
def _reference_head(head, cin, pool_name, head_type, size):
    """the same nn modules composed in float64 on the CPU"""
    hid, out = dc.HEAD_HIDDEN, dc.HEAD_OUT
    hid = head._projector[0].weight.shape[0] if head_type == "mlp" else hid
    if head_type == "mlp":
        proj = nn.Sequential(nn.Conv2d(cin, hid, 1), nn.LeakyReLU(0.01), nn.Conv2d(hid, out, 1))
    else:
        proj = nn.Sequential(nn.Conv2d(cin, out, 1))
    proj.load_state_dict({k: v.detach().cpu() for k, v in head._projector.state_dict().items()})
    pool = {"adaptive_avg": nn.AdaptiveAvgPool2d(size), "adaptive_max": nn.AdaptiveMaxPool2d(size)}.get(pool_name, nn.Identity())
    return proj.double(), pool


def _head_inputs(cin, dtype, g, seed, hid=dc.HEAD_HIDDEN, head_type="mlp", pool_name="adaptive_avg", out=dc.HEAD_OUT):
    from contrastyou.projectors.heads import DenseProjectionHead
    T = dc.DTYPES[dtype]
    torch.manual_seed(seed)
    head = DenseProjectionHead(input_dim=cin, hidden_dim=hid, output_dim=out, head_type=head_type, normalize=True,
                               pool_name=pool_name, spatial_size=(g.sh, g.sw))
    with torch.no_grad():
        for prm in head.parameters():
            if prm.dim() > 1:
                prm.copy_(prm.to(T).float())  # weights representable in the storage type
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(g.N, g.H, g.W, cin, generator=gen).to(T)
    if head_type == "mlp":  # the margin rule of dense_proj_cases.inputs
        w1, b1 = head._projector[0].weight.detach().reshape(hid, cin), head._projector[0].bias.detach()
        for _ in range(40):
            bad = (dc.pre_activation(x, w1, b1).abs() < dc.MARGIN).any(dim=-1)
            if not bad.any():
                break
            x[bad] = torch.randn(int(bad.sum()), cin, generator=gen).to(T)
        assert not bad.any()
    return head, x, gen


def _head_parity(head, x, gen, cin, pool_name, head_type, g, bars, what):
    """forward and project_points, values and every gradient, against the float64 composition"""
    unpooled = pool_name in ("identical", "none", None)
    gh, gw = (g.H, g.W) if unpooled else (g.sh, g.sw)
    proj, pool = _reference_head(head, cin, pool_name, head_type, (g.sh, g.sw))
    points = [[(0, 0), (gh - 1, gw - 1), (1, 2), (2, 1), (gh // 2, gw // 2)], [(gh - 1, 0), (0, gw - 1), (1, 1)]]
    flat = [(n, a, b) for n, pts in enumerate(points) for a, b in pts]
    coef = torch.randn(g.N, dc.HEAD_OUT, gh, gw, generator=gen)
    coef_pts = torch.randn(len(flat), dc.HEAD_OUT, generator=gen)
    head = head.to(DEV)
    ok, fig = True, []
    for mode in ("forward", "project_points"):
        head.zero_grad()
        proj.zero_grad()
        xa = x.to(DEV).permute(0, 3, 1, 2).requires_grad_(True)
        xr = x.double().permute(0, 3, 1, 2).requires_grad_(True)
        zr = F.normalize(pool(proj(xr)), p=2, dim=1)
        if mode == "forward":
            z = head(xa)
            (z * coef.to(DEV)).sum().backward()
            (zr * coef.double()).sum().backward()
        else:
            z = head.project_points(xa, points)
            zr = torch.stack([zr[n, :, a, b] for n, a, b in flat])
            (z * coef_pts.to(DEV)).sum().backward()
            (zr * coef_pts.double()).sum().backward()
        pairs = [("z", z, zr.detach(), bars["z"]), ("dx", xa.grad, xr.grad, bars["dx"])]
        pairs += [(k, p.grad.reshape(q.grad.shape), q.grad, bars["par"])
                  for (k, p), q in zip(head._projector.named_parameters(), proj.parameters())]
        for k, got, want, bar in pairs:
            assert got.shape == want.shape, (what, mode, k, got.shape, want.shape)
            err = dc.rel_err(got.detach().cpu().float(), want)
            fig.append(f"{mode} {k} {err:.2e} ({bar:.1e})")
            ok &= err <= bar
    print(f"{what}: " + "; ".join(fig))
    return ok, fig


# 16-bit heads without pooling run the per-row projector, which rounds the hidden tile, dY and dH to the storage type
# (include/contrastyou_hip.h): up to three roundings of half a unit in the last place (bf16: 2^-9) in a chain, against
# sums whose terms add up to about twice the largest result -- 8 * 2^-9.  Every other 16-bit path computes in f32 on
# exact products and rounds dx once on its store: the bounds of the fused form (dense_proj_cases.bounds).
F32_HEAD = dict(z=1e-4, dx=2e-4, par=2e-4)
BF16_HEAD = dict(z=1e-4, dx=1e-2, par=3e-3)
BF16_UNPOOLED = dict(z=8 * 2.0 ** -9, dx=8 * 2.0 ** -9, par=8 * 2.0 ** -9)


def test_dense_projection_head_every_pool_and_head_type():
    g = dc.GEOMS["nonsquare_a"]
    failures = []
    for cin, dtype in dc.HEAD_MAPS:
        for pool_name in dc.HEAD_POOLS:
            for head_type in dc.HEAD_TYPES:
                unpooled = pool_name in ("identical", "none", None)
                bars = F32_HEAD if dtype == "f32" else BF16_UNPOOLED if unpooled else BF16_HEAD
                head, x, gen = _head_inputs(cin, dtype, g, seed=cin + len(str(pool_name)), head_type=head_type, pool_name=pool_name)
                what = f"C{cin}-{dtype}-{pool_name}-{head_type}"
                ok, fig = _head_parity(head, x, gen, cin, pool_name, head_type, g, bars, what)
                if not ok:
                    failures.append((what, fig))
    assert not failures, failures


@pytest.mark.parametrize("cin,hid", [(32, 512), (20, 128), (20, 512)])
def test_heads_outside_the_fused_range_train(cin, hid):
    """more than 256 hidden units (cy_dense_proj_bwd refuses them after cy_dense_proj_fwd has run), or channels that are
    no multiple of 8: the head composes the Linear and the pooling kernels instead, forward AND backward"""
    g = dc.GEOMS["nonsquare_a"]
    head, x, gen = _head_inputs(cin, "f32", g, seed=hid + cin, hid=hid)
    assert not head._fused_hidden()
    ok, fig = _head_parity(head, x, gen, cin, "adaptive_avg", "mlp", g, F32_HEAD, f"C{cin}-h{hid}-f32")
    assert ok, fig
    opt = torch.optim.SGD(head.parameters(), lr=0.1)
    before = [p.detach().clone() for p in head.parameters()]
    opt.step()
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, head.parameters())), "a step moves every parameter"


@pytest.mark.parametrize("pool_name", ["adaptive_avg", "adaptive_max"])
@pytest.mark.parametrize("size,named", [((24, 9), "(24, 9)"), ((5, 39), "(5, 39)")])
def test_a_pooling_grid_larger_than_the_map_is_refused_by_name(pool_name, size, named):
    from contrastyou.projectors.heads import DenseProjectionHead
    head = DenseProjectionHead(input_dim=16, hidden_dim=32, output_dim=8, head_type="mlp", normalize=True,
                               pool_name=pool_name, spatial_size=size).to(DEV)
    x = torch.randn(2, 16, 23, 38, device=DEV)
    with pytest.raises(ValueError) as e:
        head(x)
    assert named in str(e.value) and "(23, 38)" in str(e.value)
    with pytest.raises(ValueError):
        head.project_points(x, [[(0, 0)], [(1, 1)]])
