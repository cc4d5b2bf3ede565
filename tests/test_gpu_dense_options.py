"""The per-row projector kernels (csrc/cy_pixel_mlp.hip) and the DenseProjectionHead options built on them: no pooling
("identical" / "none" / None), point evaluation under adaptive_max pooling and for the linear head.

Bounds.  f32 rows: 1e-4 of each tensor's largest magnitude forward, 2e-4 for gradients (the project's bars), against
float64 torch on the CPU.  bf16 / f16 rows: the bound of a tensor is TWICE the error of a CPU emulation with the
kernels' rounding points (tests/dense_option_cases.emulate) against the same float64 reference on the same inputs; the
measured emulation errors are recorded in EMU_ERR below (tests/test_dense_options_host.py re-measures them).  Over the
cases of a dtype the largest are
    bf16: forward 6.95e-3, gradients 2.31e-1        f16: forward 1.78e-3, gradients 1.88e-3
(the bf16 gradient figure is LeakyReLU's: W1 rounded to bf16 moves ~0.2 % of the pre-activations across 0, and each
such element changes its dH by a factor 100; the tensors without that -- y, dW2, db2, the linear head -- sit at
2-7e-3).  Because that bound is wide, the 16-bit results are ALSO held against the emulation itself at two units in
the last place of the storage type (2^-6 bf16, 2^-9 f16, of the tensor's largest magnitude): kernel and emulation
multiply the same rounded operands and differ by f32 against f64 summation only, which can move a rounding of an
intermediate or of a stored dx element by one unit.  The inputs keep every pre-activation 1e-4 away from 0, so both
take the same side of LeakyReLU."""
import numpy as np
import pytest
import torch

from tests import dense_option_cases as dc

pytestmark = pytest.mark.gpu

# measured: rel_err(emulate(case), reference(case)) per tensor; the kernel's bound is twice the entry
EMU_ERR = {
    "M1-C32-h0-o5-bf16-idx": {"y": 0.00258, "dx": 0.0024, "dw1": 0.00242, "db1": 0.00242},
    "M63-C8-h64-o32-bf16-norm": {"y": 0.00277, "dx": 0.0625, "dw1": 0.148, "db1": 0.0511, "dw2": 0.00346, "db2": 0.00186},
    "M126-C256-h256-o256-bf16-norm-idx": {"y": 0.00237, "dx": 0.121, "dw1": 0.137, "db1": 0.0637, "dw2": 0.00255, "db2": 0.00168},
    "M65537-C8-h64-o5-bf16-norm": {"y": 0.00695, "dx": 0.231, "dw1": 0.0277, "db1": 0.0271, "dw2": 0.00373, "db2": 0.0044},
    "M126-C32ld48-h64-o32-f16-norm": {"y": 0.000385, "dx": 0.000537, "dw1": 0.000422, "db1": 0.000511, "dw2": 0.00021, "db2": 0.000249},
    "M63-C256-h0-o256-f16-idx": {"y": 0.000164, "dx": 0.000452, "dw1": 0.000223, "db1": 0.000225},
    "M65537-C32-h0-o5-f16-norm": {"y": 0.00178, "dx": 0.00188, "dw1": 0.000519, "db1": 0.00026},
}
F32_BAR = {"y": 1e-4, "dx": 2e-4, "dw1": 2e-4, "db1": 2e-4, "dw2": 2e-4, "db2": 2e-4}
TWO_ULP = {"bf16": 2.0 ** -6, "f16": 2.0 ** -9}
DEV = "cuda:0"


def _run(c, t=None):
    """forward and backward of PixelMLPFn on the case's inputs -> CPU tensors named as in dc.reference"""
    from cyhip.functions import PixelMLPFn
    t = t or dc.inputs(c)
    base = t["x"].to(DEV).requires_grad_(True)  # [R, ldx]; the kernel reads the first C columns of every row
    idx = None if t["idx"] is None else t["idx"].to(DEV)
    par = {k: (None if t[k] is None else t[k].to(DEV).requires_grad_(True)) for k in ("w1", "b1", "w2", "b2")}
    y = PixelMLPFn.apply(base[:, :c.C], idx, par["w1"], par["b1"], par["w2"], par["b2"], dc.SLOPE, c.normalize)
    y.backward(t["dy"].to(DEV))
    torch.cuda.synchronize()
    res = dict(y=y.detach().cpu(), dx=base.grad.cpu(), dw1=par["w1"].grad.cpu(), db1=par["b1"].grad.cpu())
    if c.hid:
        res.update(dw2=par["w2"].grad.cpu(), db2=par["b2"].grad.cpu())
    return res


@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_kernel_parity_with_float64(case):
    ref, got = dc.reference(case), _run(case)
    assert set(got) == set(ref)
    bars = F32_BAR if case.dtype == "f32" else {k: 2 * v for k, v in EMU_ERR[dc.case_id(case)].items()}
    errs = {k: dc.rel_err(got[k], ref[k]) for k in ref}
    print(dc.case_id(case), "vs float64:", {k: f"{e:.2e}" for k, e in errs.items()})
    assert got["y"].dtype == torch.float32 and got["dx"].dtype == dc.DTYPES[case.dtype]
    assert all(torch.isfinite(v).all() for v in got.values())
    if case.dtype != "f32":
        emu = dc.emulate(case)
        eerrs = {k: dc.rel_err(got[k], emu[k]) for k in ref}
        print(dc.case_id(case), "vs emulation:", {k: f"{e:.2e}" for k, e in eerrs.items()})
    for k in ref:
        assert errs[k] <= bars[k], (k, errs[k], bars[k])
    if case.dtype != "f32":
        for k in ref:
            assert eerrs[k] <= TWO_ULP[case.dtype], (k, eerrs[k])
    # exactly zero where nothing was computed: rows not listed, columns of the pixel stride's padding
    zero = ref["dx"] == 0
    zero[:, case.C:] = True
    if case.idx:
        rest = torch.ones(ref["dx"].shape[0], dtype=torch.bool)
        rest[dc.inputs(case)["idx"].long()] = False
        zero[rest] = True
        assert rest.sum() == 37
    assert (got["dx"][zero] == 0).all()


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_row_list_gives_the_rows_of_the_full_launch(dtype):
    from cyhip.functions import PixelMLPFn
    g = torch.Generator().manual_seed(11)
    R, Cc, hid, out = 2 * 7 * 9 + 3, 32, 64, 24
    x = torch.randn(R, Cc, generator=g).to(dc.DTYPES[dtype]).to(DEV)
    w1, b1 = (torch.randn(hid, Cc, generator=g) / 6).to(DEV), torch.randn(hid, generator=g).to(DEV)
    w2, b2 = (torch.randn(out, hid, generator=g) / 8).to(DEV), torch.randn(out, generator=g).to(DEV)
    idx = torch.randperm(R, generator=g)[:70].to(torch.int32).to(DEV)
    for lin in (False, True):
        args = (w1, b1, None, None) if lin else (w1, b1, w2, b2)
        for normalize in (True, False):
            full = PixelMLPFn.apply(x, None, *args, 0.01, normalize)
            xl = x.clone().requires_grad_(True)
            some = PixelMLPFn.apply(xl, idx, *args, 0.01, normalize)
            assert some.shape == (70, hid if lin else out)
            assert torch.equal(some, full[idx.long()])
            some.backward(torch.randn(some.shape, generator=g).to(DEV))
            rest = torch.ones(R, dtype=torch.bool, device=DEV)
            rest[idx.long()] = False
            assert (xl.grad[rest] == 0).all() and (xl.grad[idx.long()] != 0).any(dim=1).all()


@pytest.mark.parametrize("case", [c for c in dc.CASES if c.M == 126 and c.hid == 256], ids=dc.case_id)
def test_two_runs_give_the_same_bits(case):
    assert dc.plan(case)["slabs"] > 1
    a, b = _run(case), _run(case)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_two_runs_give_the_same_bits_past_the_cap():
    case = next(c for c in dc.CASES if c.dtype == "bf16" and c.M > 60000)
    p = dc.plan(case)
    assert p["slabs"] == 256 and p["bwd_trips"] > 1
    a, b = _run(case), _run(case)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ module level
def _golden(golden_dir):
    return np.load(golden_dir / "dense_options.npz")


@pytest.mark.parametrize("normalize", (True, False))
@pytest.mark.parametrize("head_type", ("mlp", "linear"))
@pytest.mark.parametrize("pool", ("identical", "none"))
def test_unpooled_head_matches_the_reference(golden_dir, pool, head_type, normalize):
    from contrastyou.projectors import DenseProjectionHead
    G = _golden(golden_dir)
    tag = f"{pool}_{head_type}_{int(normalize)}"
    head = DenseProjectionHead(input_dim=16, hidden_dim=32, output_dim=24, head_type=head_type, normalize=normalize,
                               pool_name=pool)
    names = [str(n) for n in G[f"{tag}_names"]]
    assert sorted(head.state_dict()) == names
    head.load_state_dict({n: torch.from_numpy(G[f"{tag}_w_{n}"]) for n in names}, strict=True)
    head = head.to(DEV)
    x = (torch.from_numpy(G["feat_i8d32"]).float() / 32).to(DEV).requires_grad_(True)
    y = head(x)
    assert tuple(y.shape) == (2, 24, 7, 9) and y.permute(0, 2, 3, 1).is_contiguous()
    (y * torch.from_numpy(G[f"{tag}_coef"]).to(DEV)).sum().backward()
    errs = {"y": dc.rel_err(y.detach().cpu(), torch.from_numpy(G[f"{tag}_y"]).double()),
            "dx": dc.rel_err(x.grad.cpu(), torch.from_numpy(G[f"{tag}_dx"]).double())}
    for n, p in head.named_parameters():
        errs[n] = dc.rel_err(p.grad.cpu(), torch.from_numpy(G[f"{tag}_g_{n}"]).double())
    print(tag, {k: f"{e:.2e}" for k, e in errs.items()})
    assert errs.pop("y") <= 1e-4
    assert all(e <= 2e-4 for e in errs.values()), errs


def test_sizes_outside_the_fused_range_compose_the_linear_kernels():
    import torch.nn.functional as F
    from contrastyou.projectors import DenseProjectionHead
    torch.manual_seed(5)
    head = DenseProjectionHead(input_dim=260, hidden_dim=32, output_dim=24, head_type="mlp", normalize=True,
                               pool_name="none").to(DEV)
    x = torch.randn(2, 260, 5, 6, device=DEV, requires_grad=True)
    pts = [[(0, 0), (4, 5)], [(2, 3)]]
    rows = head.project_points(x, pts)
    w1, b1, w2, b2 = (p.detach().double().cpu() for p in head._projector.parameters())
    xd = x.detach().double().cpu()
    want = F.conv2d(F.leaky_relu(F.conv2d(xd, w1, b1), 0.01), w2, b2)
    want = F.normalize(want, dim=1)
    want = torch.stack([want[0, :, 0, 0], want[0, :, 4, 5], want[1, :, 2, 3]])
    assert dc.rel_err(rows.detach().cpu(), want) <= 1e-4
    full = head(x)
    assert dc.rel_err(full.detach().cpu()[1, :, 2, 3], want[2]) <= 1e-4


# ------------------------------------------------------------------------------------------------ point evaluation
PTS = [[(0, 0), (3, 2), (1, 4)], [(2, 2), (4, 0)]]


def _point_case(pool, head_type, size, dtype=torch.float32):
    from contrastyou.projectors import DenseProjectionHead
    torch.manual_seed(21)
    head = DenseProjectionHead(input_dim=16, hidden_dim=32, output_dim=24, head_type=head_type, normalize=True,
                               pool_name=pool, spatial_size=size).to(DEV)
    x = torch.randn(2, 16, 11, 13, device=DEV).to(dtype)
    coef = torch.randn(5, 24, device=DEV)
    a = x.clone().requires_grad_(True)
    rows = head.project_points(a, PTS)
    (rows * coef).sum().backward()
    b = x.clone().requires_grad_(True)
    full = head(b)
    n = torch.tensor([i for i, im in enumerate(PTS) for _ in im], device=DEV)
    r = torch.tensor([p[0] for im in PTS for p in im], device=DEV)
    cc = torch.tensor([p[1] for im in PTS for p in im], device=DEV)
    picked = full[n, :, r, cc]
    (picked * coef).sum().backward()
    assert tuple(full.shape[2:]) == tuple(head.output_size(x)) and rows.shape == (5, 24)
    return rows.detach(), picked.detach(), a.grad, b.grad


def _close(u, v, rel):
    return float((u.double() - v.double()).abs().max()) <= rel * float(v.double().abs().max())


@pytest.mark.parametrize("head_type", ("mlp", "linear"))
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
def test_unpooled_points_are_the_map_at_the_points(head_type, dtype):
    rows, picked, ga, gb = _point_case("identical", head_type, (16, 16), dtype)
    assert _close(rows, picked, 1e-6) and _close(ga, gb, 1e-6)
    listed = torch.zeros(2, 11, 13, dtype=torch.bool, device=DEV)
    for i, im in enumerate(PTS):
        for r, c in im:
            listed[i, r, c] = True
    assert (ga.permute(0, 2, 3, 1)[~listed] == 0).all() and ga.dtype == dtype


@pytest.mark.parametrize("head_type", ("mlp", "linear"))
def test_adaptive_max_points_gather_the_pooled_rows(head_type):
    rows, picked, ga, gb = _point_case("adaptive_max", head_type, (5, 5))
    assert torch.equal(rows, picked) and torch.equal(ga, gb)


def test_linear_average_pool_points():
    rows, picked, ga, gb = _point_case("adaptive_avg", "linear", (5, 5))
    assert _close(rows, picked, 1e-6) and _close(ga, gb, 1e-6)


# ------------------------------------------------------------------------------------------------ memory
def test_no_hidden_intermediate_reaches_memory():
    """M = 2 * 256 * 256 rows, C = 32, hid = 256, out = 16, f32: a [M, hid] f32 tensor would be 128 MB; everything the
    launches may allocate -- y 8 MB, inv 0.5 MB, dx 16 MB, the 256 partial slabs 16.3 MB, + 1 MB for the parameter
    gradients and the allocator's rounding -- is 42 MB.  (At the 2 * 64 * 64 rows of the smaller problem the slabs alone
    exceed the 8 MB hidden tensor: the workspace does not shrink with M once there are 256 tiles.)"""
    from cyhip import _lib
    from cyhip.functions import PixelMLPFn
    M, Cc, hid, out = 2 * 256 * 256, 32, 256, 16
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, Cc, generator=g).to(DEV).requires_grad_(True)
    w1, b1 = (torch.randn(hid, Cc, generator=g) / 6).to(DEV).requires_grad_(True), torch.zeros(hid, device=DEV, requires_grad=True)
    w2, b2 = (torch.randn(out, hid, generator=g) / 16).to(DEV).requires_grad_(True), torch.zeros(out, device=DEV, requires_grad=True)
    dy = torch.randn(M, out, generator=g).to(DEV)
    ws_bytes = _lib.load().cy_pixel_mlp_bwd_ws_bytes(M, Cc, hid, out, 0)
    allowed = M * out * 4 + M * 4 + M * Cc * 4 + ws_bytes + (1 << 20)
    assert allowed < M * hid * 4 / 2
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    y = PixelMLPFn.apply(x, None, w1, b1, w2, b2, 0.01, True)
    y.backward(dy)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise / 2 ** 20:.1f} MB, allowed {allowed / 2 ** 20:.1f} MB, hidden tensor {M * hid * 4 / 2 ** 20:.0f} MB")
    assert rise < allowed
    assert x.grad is not None and w2.grad is not None and torch.isfinite(y).all()
