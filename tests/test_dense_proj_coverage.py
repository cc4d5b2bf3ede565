"""tests/test_gpu_dense_dispatch.py claims to run every form of the dense projector (VALU, register-resident and
streamed matrix-core kernels) on non-square maps, at the small and the large end of the job sizes and past every launch
cap, and the pools and the row gather past theirs.  The claims are conditions on the case table
(tests/dense_proj_cases.py), on constants read from the sources and on the host-side plan query (cy_dense_proj_plan),
so they are checked here without a GPU.  Each assertion names its condition: deleting a case fails here, by name.

Also here, because they need no GPU either: the sensitivity of the bounds (a float64 model with ONE fault of the kind
the cases exist for must miss the true reference by more than the bound the GPU test applies), and the argument checks
of the entry points, which all return before any launch."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import dense_proj_cases as dc

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "contrast-you_amd" / "csrc"

REG_BF16 = dc.Inst("reg", 64, 256, "bf16", dc.SLOPE)


def _const(text, name):
    return int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))


@pytest.fixture(scope="module")
def caps():
    dense, mfma = (CSRC / "cy_dense.hip").read_text(), (CSRC / "cy_dense_mfma.h").read_text()
    valu_cap = re.search(r"inline int dp_bwd_blocks\(int nb\) \{ return nb < (\d+) \? nb : (\d+); \}", dense)
    assert valu_cap and valu_cap.group(1) == valu_cap.group(2)
    part = re.search(r"constexpr int DPM_PART = (\d+) \* (\d+);", mfma)
    return dict(wgs=_const(mfma, "DPM_WGS"), grid_cap=_const(dense, "GRID_CAP"), valu=int(valu_cap.group(1)),
                part=int(part.group(1)) * int(part.group(2)))


def test_caps_match_the_sources(caps):
    assert caps == dict(wgs=512, grid_cap=8192, valu=256, part=68 * 64)
    mfma = (CSRC / "cy_dense_mfma.h").read_text()
    # the grids the job counts below are derived from
    assert "const int grid = nb < DPM_WGS * 4 ? cy_cdiv(nb, 4) : DPM_WGS;" in mfma
    assert "const int grid = njobs < DPM_WGS * 4 ? cy_cdiv(njobs, 4) : DPM_WGS;" in mfma
    assert "const int njobs = cells ? N * (2 * sh - 1) * (2 * sw - 1) : nb;" in mfma


def test_every_instantiation_and_geometry_is_present():
    assert list(dc.GEOMS) == ["nonsquare_a", "nonsquare_b", "one_bin", "pixel_bins", "big_bins", "past_cap", "long_list"]
    g = {k: tuple(v) for k, v in dc.GEOMS.items()}
    assert g["nonsquare_a"] == (2, 23, 38, 5, 9, False) and g["nonsquare_b"] == (2, 38, 23, 7, 4, False)
    assert g["one_bin"] == (1, 19, 21, 1, 1, False) and g["pixel_bins"] == (2, 9, 12, 9, 12, False)
    assert g["big_bins"] == (2, 40, 56, 2, 3, False)
    assert g["past_cap"] == (3, 33, 33, 32, 32, False) and g["long_list"] == (3, 33, 33, 32, 32, True)
    insts = {(i.form, i.C, i.hid, i.dtype, i.slope) for i in dc.INSTANCES}
    want = {("valu", c, h, d, dc.SLOPE) for c in (8, 40, 96) for h in (64, 256) for d in ("f32", "bf16", "f16")}
    want |= {("valu", 32, 128, d, 1.5) for d in ("bf16", "f16")}
    want |= {("reg", c, h, d, dc.SLOPE) for c in (32, 64, 128) for h in (128, 256) for d in ("bf16", "f16")}
    want |= {("stream", c, h, d, dc.SLOPE) for c in (256, 512) for h in (128, 256) for d in ("bf16", "f16")}
    assert insts == want and len(dc.INSTANCES) == len(want) == 40
    have = set(dc.CASES)
    for inst in dc.INSTANCES:
        for name in ("nonsquare_a", "past_cap"):
            assert dc.Case(name, inst) in have, (name, inst)
    for name in ("nonsquare_b", "one_bin", "pixel_bins", "big_bins", "long_list"):
        seen = {(c.inst.form, c.inst.dtype) for c in dc.CASES if c.geom == name}
        assert seen >= {(f, d) for f in ("valu", "reg", "stream") for d in ("bf16", "f16")} | {("valu", "f32")}, name
    assert {c.inst.form for c in dc.OPTION_CASES} == {"valu", "reg", "stream"}
    assert all(c.geom == "nonsquare_a" for c in dc.OPTION_CASES)
    assert len(set(map(dc.case_id, dc.CASES))) == len(dc.CASES)


def test_each_case_runs_the_form_it_names():
    from cyhip import ops
    for inst in dc.INSTANCES + dc.ROTATION + dc.OPTION_INSTANCES:
        assert dc.form_of(inst) == inst.form, inst
    # the slope case has a matrix-core shape and is on the VALU form because of its slope alone
    assert dc.form_of(dc.Inst("reg", 32, 128, "bf16", dc.SLOPE)) == "reg"
    # C = 512 with 256 hidden units: W1 of the dx kernel comes from the workspace
    assert ops.dense_proj_plan(512, 256, torch.bfloat16)["w1_image_in_ws"] == 1
    assert any(i.C == 512 and i.hid == 256 for i in dc.ROTATION) and any(i.C == 512 and i.hid == 256 for i in dc.OPTION_INSTANCES)


def test_the_geometries_reach_what_they_claim(caps):
    G = dc.GEOMS
    waves = 4 * caps["wgs"]
    # past_cap: the forward's second job per wave, many cells per wave, the VALU backward past its blocks
    assert dc.num_bins("past_cap") == 3072 > waves and dc.num_cells(G["past_cap"]) == 11907 > 5 * waves
    assert dc.num_bins("past_cap") > 2 * caps["valu"]
    # long_list: every colour launch of the CELLS = false kernels walks more records than there are waves, so a wave
    # takes a second record in each; the dW1 kernel at 256 hidden units has half the waves per pass: three records.
    # (A colour class alone -- a quarter of at most 3 072 bins -- cannot outnumber 2 048 waves at this map size.)
    nb = dc.num_bins("long_list")
    b = dc.bin_list("long_list")
    assert 2400 < nb < 2500 and nb > waves and -(-nb // (waves // 2)) == 3
    assert len({tuple(r) for r in b.tolist()}) == nb and not all((b[1:, 1] >= b[:-1, 1]).tolist()), "distinct, shuffled"
    colours = [dc.colour_of(i, j) for _, i, j in b.tolist()]
    per_colour = [colours.count(k) for k in range(4)]
    assert min(per_colour) > 500, per_colour
    # ... and in every colour launch some wave's FIRST record is of another colour while its second is of this one
    for k in range(4):
        assert any(colours[w] != k and colours[w + waves] == k for w in range(nb - waves)), k
    cnt = dc.cover("long_list")
    assert set(cnt.unique().tolist()) >= {0, 1, 2, 3, 4}, "pixels of no listed bin, and of one to four"
    # one_bin: one job, fewer than four jobs, 13 blocks with a partial last one
    g = G["one_bin"]
    assert dc.num_bins("one_bin") == 1 and g.N == 1 and g.H * g.W == 399 == 12 * 32 + 15 and dc.num_cells(g) == 1
    # pixel_bins: every bin one pixel, every odd cell segment empty
    g = G["pixel_bins"]
    assert all(dc.bin_rect(g, i, j) == (i, i + 1, j, j + 1) for i in range(g.sh) for j in range(g.sw))
    assert (dc.cover("pixel_bins") == 1).all() and dc.num_cells(g) > dc.num_bins("pixel_bins")
    # big_bins: bins of 20 x 19 pixels and more, many blocks per job
    g = G["big_bins"]
    sizes = [(r1 - r0) * (c1 - c0) for r0, r1, c0, c1 in (dc.bin_rect(g, i, j) for i in range(2) for j in range(3))]
    assert min(sizes) == 20 * 19 and max(sizes) == 20 * 20 and min(sizes) > 11 * 32
    # the non-square maps: ragged bins, shared rows and columns, and rectangles that change under a swap of the axes
    for name in ("nonsquare_a", "nonsquare_b"):
        g = G[name]
        assert g.H != g.W and g.sh != g.sw and g.H % g.sh and g.W % g.sw
        assert set(dc.cover(name).unique().tolist()) == {1, 2, 4}
        t = dc.Geom(g.N, g.W, g.H, g.sw, g.sh, False)
        rects = {dc.bin_rect(g, i, j) for i in range(g.sh) for j in range(g.sw)}
        swapped = {(c0, c1, r0, r1) for r0, r1, c0, c1 in (dc.bin_rect(t, j, i) for i in range(g.sh) for j in range(g.sw))}
        assert rects == swapped, "transposing map and grid together transposes the rectangles"
        wrong = dc.Geom(g.N, g.H, g.W, g.sw, g.sh, False)  # sh and sw exchanged alone
        assert all(dc.bin_rect(g, i, j) != dc.bin_rect(wrong, i, j) for i in range(1, min(g.sh, g.sw)) for j in range(1, min(g.sh, g.sw)))
        heights = {dc.bin_range(i, g.H, g.sh)[1] - dc.bin_range(i, g.H, g.sh)[0] for i in range(g.sh)}
        widths = {dc.bin_range(j, g.W, g.sw)[1] - dc.bin_range(j, g.W, g.sw)[0] for j in range(g.sw)}
        assert len(heights) > 1 and len(widths) > 1 and g.H * g.sw != g.W * g.sh, "ragged, another ratio per axis"
    a, b = G["nonsquare_a"], G["nonsquare_b"]
    assert a.H < a.W and a.sh < a.sw and b.H > b.W and b.sh > b.sw


def test_the_margin_holds_on_every_input_set():
    for c in dc.CASES + dc.OPTION_CASES:
        for pad in ((0, dc.LDX_PAD) if c in dc.OPTION_CASES else (0,)):
            t = dc.inputs(c, pad)
            T = dc.DTYPES[c.inst.dtype]
            assert t["x"].dtype == T and torch.equal(t["w1"], t["w1"].to(T).float()), dc.case_id(c)
            assert dc.pre_activation(t["x"], t["w1"], t["b1"]).abs().min() >= dc.MARGIN, dc.case_id(c)
            if pad:
                assert t["x"][..., c.inst.C:].isnan().all() and t["x"].shape[-1] == c.inst.C + 16


def test_the_workspace_query_covers_every_case(caps):
    from cyhip import _lib, ops
    lib = _lib.load()
    for c in dc.CASES + dc.OPTION_CASES:
        g, i = dc.GEOMS[c.geom], c.inst
        nb = dc.num_bins(c.geom)
        njobs = nb if g.listed else dc.num_cells(g)
        have = lib.cy_dense_proj_bwd_ws_bytes(nb, i.C, i.hid)
        valu = min(nb, caps["valu"]) * (i.hid * i.C + i.hid) * 4
        assert njobs <= 4 * nb
        need = valu
        if i.form == "reg":
            need = caps["wgs"] * caps["part"] * 4 + 64 * njobs
        elif i.form == "stream":
            image = i.hid * i.C * 2 * ops.dense_proj_plan(i.C, i.hid, dc.DTYPES[i.dtype])["w1_image_in_ws"]
            need = max(valu, caps["wgs"] * caps["part"] * 4 + 64 * 4 * nb + image)
        assert have >= need, (dc.case_id(c), have, need)


# ------------------------------------------------------------------------------------------------ sensitivity
def test_the_model_is_the_reference():
    for name in ("nonsquare_a", "nonsquare_b", "one_bin", "long_list"):
        c = dc.Case(name, REG_BF16)
        assert c in dc.CASES
        ref, mod = dc.reference(c), dc.model(c)
        assert dc.rel_err(mod["hpool"], ref["hpool"]) < 1e-12 and dc.rel_err(mod["dx"], ref["dx"]) < 1e-12, name


def test_the_bounds_see_the_faults_the_cases_exist_for():
    bar = dc.bounds("bf16")  # the widest bounds the GPU test applies
    for name in ("nonsquare_a", "nonsquare_b"):
        c = dc.Case(name, REG_BF16)
        ref, bad = dc.reference(c), dc.model(c, "swap")
        assert dc.rel_err(bad["hpool"], ref["hpool"]) > bar["hpool"], name
        assert dc.rel_err(bad["dx"], ref["dx"]) > bar["dx"], name
    c = dc.Case("nonsquare_a", REG_BF16)
    ref = dc.reference(c)
    dropped = dc.class_errors(c.geom, dc.model(c, "drop_bin")["dx"], ref["dx"])
    assert dropped[4] > bar["dx"] and max(dropped[1], dropped[2]) < 1e-12, dropped
    wrong = dc.class_errors(c.geom, dc.model(c, "wrong_inv")["dx"], ref["dx"])
    assert wrong[2] > bar["dx"] and wrong[4] > bar["dx"] and wrong[1] < 1e-12, wrong
    c = dc.Case("one_bin", REG_BF16)
    assert dc.rel_err(dc.model(c, "drop_tail")["hpool"], dc.reference(c)["hpool"]) > bar["hpool"]
    # the max pool is compared bit for bit: the last maximum instead of the first must change indices AND gradients
    for p in dc.MAX_CASES:
        rows, arg, dx = dc.max_reference(p)
        rows_l, arg_l, dx_l = dc.max_reference(p, last=True)
        assert torch.equal(rows, rows_l), "the same maxima"
        if p.sh < p.H:
            assert not torch.equal(arg, arg_l) and not torch.equal(dx, dx_l), dc.pool_id(p)


# ------------------------------------------------------------------------------------------------ pools and gather
def test_the_pool_and_gather_cases_reach_their_branches(caps):
    per_trip = caps["grid_cap"] * 256
    n, h, w, ch = dc.PAST_CAP_MAP
    assert per_trip < n * h * w * ch == 2129920 < 2 * per_trip
    assert any((p.N, p.H, p.W, p.C) == dc.PAST_CAP_MAP and p.dtype == "bf16" for p in dc.AVG_BWD)
    assert any((p.N, p.H, p.W, p.C) == dc.PAST_CAP_MAP for p in dc.MAX_CASES)
    assert {p.C for p in dc.AVG_FWD} == {8, 260} and {p.C for p in dc.MAX_CASES} >= {8, 260}, "the c += 256 loop"
    for cases in (dc.AVG_FWD, dc.MAX_CASES):
        assert {p.dtype for p in cases} == {"f32", "bf16", "f16"}
    assert {p.listed for p in dc.AVG_FWD} == {True, False}
    geoms = {(p.N, p.H, p.W, p.sh, p.sw) for p in dc.AVG_FWD}
    assert geoms == {tuple(dc.GEOMS[k])[:5] for k in ("nonsquare_a", "one_bin", "pixel_bins")}
    M, D = dc.GATHER[0]
    assert (M, D) == (8200, 257) and M * D == 2107400 > per_trip and (300, 1) in dc.GATHER and (1, 257) in dc.GATHER
    for p in dc.MAX_CASES:
        x, dpool = dc.max_inputs(p)
        assert set(x.float().unique().tolist()) == set(dc.MAX_LEVELS) and (dpool * 8 == (dpool * 8).round()).all()
        if p.sh == p.H:
            continue
        rows, arg, dx = dc.max_reference(p)
        # ties in nearly every bin, and a pixel that is the arg-max of several overlapping bins
        xr = x.float().permute(0, 3, 1, 2)
        ties = 0
        for i in range(p.sh):
            r0, r1 = dc.bin_range(i, p.H, p.sh)
            for j in range(p.sw):
                c0, c1 = dc.bin_range(j, p.W, p.sw)
                blk = xr[:, :, r0:r1, c0:c1].reshape(p.N, p.C, -1)
                ties += int(((blk == blk.amax(-1, keepdim=True)).sum(-1) > 1).sum())
        assert ties > 0.9 * rows.numel(), (dc.pool_id(p), ties, rows.numel())
        a = arg.reshape(p.N, p.sh * p.sw, p.C).long()
        hits = torch.zeros(p.N, p.H * p.W, p.C, dtype=torch.int64).scatter_add_(1, a, torch.ones_like(a))
        assert hits.max() >= 2, dc.pool_id(p)


def test_the_head_decides_its_route_before_any_launch():
    """the limits the head routes by are the entry points' own (the rejection test below holds them to the library)"""
    from contrastyou.projectors.heads import DenseProjectionHead as Head
    mk = lambda cin, hid: Head(input_dim=cin, hidden_dim=hid, output_dim=8, head_type="mlp", normalize=True)  # noqa: E731
    assert (Head.FUSED_MAX_HIDDEN, Head.FUSED_CHANNEL_STEP) == (256, 8)
    assert mk(32, 256)._fused_hidden() and mk(8, 1)._fused_hidden()
    assert not mk(32, 257)._fused_hidden() and not mk(32, 512)._fused_hidden() and not mk(20, 128)._fused_hidden()
    dense = (CSRC / "cy_dense.hip").read_text()
    assert dense.count("C % 8 || ldx < C || ldx % 8 || hid <= 0") == 2 and dense.count("hid > 256") == 1


def test_half_ulp_is_the_rounding_error_of_the_storage_type():
    gen = torch.Generator().manual_seed(3)
    v = torch.randn(200000, generator=gen).double() * 10.0 ** torch.randint(-9, 3, (200000,), generator=gen).double()
    v = v.float().double()  # f32 values, as the kernels round them: one rounding to the storage type, not two
    for name, T in dc.DTYPES.items():
        err, bound = (v.to(T).double() - v).abs(), dc.half_ulp(v, name)
        assert (err <= bound).all(), name
        assert name == "f32" or (err / bound).max() > 0.99, (name, "the bound is met, not merely kept")
        normal = v.abs() > 2.0 ** dc.STORAGE_FORMAT[name][1]
        assert (bound[normal] <= 2.0 ** -(dc.STORAGE_FORMAT[name][0] + 1) * v.abs()[normal]).all(), name
    assert dc.half_ulp(torch.tensor([1.0, 1.5, 1e-6], dtype=torch.float64), "bf16").tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -28]
    assert dc.half_ulp(torch.tensor([1.0, 1e-6], dtype=torch.float64), "f16").tolist() == [2.0 ** -11, 2.0 ** -25]


# ------------------------------------------------------------------------------------------------ rejections
ARG, SHAPE, DTYPE, WORKSPACE = -1, -2, -3, -5


class _Host:
    """host buffers standing in for device memory: every call below is refused before any launch, so nothing may read
    or write them; `untouched()` holds the outputs to that"""

    def __init__(self):
        self.bufs = {k: (C.c_uint8 * 4096)(*([0xA5] * 4096)) for k in ("x", "w1", "b1", "hpool", "dh", "dx", "dw1", "db1", "ws")}

    def __getitem__(self, k):
        return C.addressof(self.bufs[k])

    def untouched(self):
        return all(bytes(b) == b"\xa5" * 4096 for b in self.bufs.values())


def test_the_entry_points_refuse_before_any_launch():
    from cyhip import _lib
    lib = _lib.load()
    assert (_lib.CY_ERR_ARG, _lib.CY_ERR_SHAPE, _lib.CY_ERR_DTYPE, _lib.CY_ERR_WORKSPACE) == (ARG, SHAPE, DTYPE, WORKSPACE)
    m = _Host()
    N, H, W, Cc, hid, sh, sw = 2, 23, 38, 32, 128, 5, 9
    nb = N * sh * sw
    ws_bytes = lib.cy_dense_proj_bwd_ws_bytes(nb, Cc, hid)
    assert ws_bytes > 0

    def fwd(x="x", w1="w1", b1="b1", hpool="hpool", bins=None, nb=nb, N=N, H=H, W=W, C_=Cc, ldx=None, hid=hid, sh=sh,
            sw=sw, dtype=_lib.CY_BF16):
        p = lambda k: None if k is None else m[k]  # noqa: E731
        return lib.cy_dense_proj_fwd(p(x), p(w1), p(b1), p(bins), nb, p(hpool), N, H, W, C_, C_ if ldx is None else ldx,
                                     hid, sh, sw, 0.01, dtype, None)

    def bwd(x="x", w1="w1", b1="b1", dh="dh", bins=None, nb=nb, N=N, H=H, W=W, C_=Cc, ldx=None, hid=hid, sh=sh, sw=sw,
            dtype=_lib.CY_BF16, ws="ws", ws_bytes=ws_bytes):
        p = lambda k: None if k is None else m[k]  # noqa: E731
        return lib.cy_dense_proj_bwd(p(x), p(w1), p(b1), p(bins), nb, p(dh), m["dx"], m["dw1"], m["db1"], 0, N, H, W, C_,
                                     C_ if ldx is None else ldx, hid, sh, sw, 0.01, dtype, p(ws), ws_bytes, None)

    for f in (fwd, bwd):
        for k in ("x", "w1", "b1"):
            assert f(**{k: None}) == ARG, (f.__name__, k)
        assert f(N=0) == ARG and f(nb=0) == ARG
        assert f(C_=36) == SHAPE and f(ldx=Cc - 8) == SHAPE and f(ldx=Cc + 4) == SHAPE, f.__name__
        assert f(hid=0) == SHAPE and f(hid=-128) == SHAPE
        assert f(sh=H + 1) == SHAPE and f(sw=W + 1) == SHAPE and f(sh=0) == SHAPE and f(sw=0) == SHAPE
        assert f(nb=nb - 1) == SHAPE and f(nb=nb + 1) == SHAPE, "nb != N * sh * sw without a bin list"
        assert f(dtype=7) == DTYPE and f(dtype=-1) == DTYPE
        # the order of the checks: arguments, shapes, the bin count, the dtype (, the workspace)
        assert f(x=None, C_=36) == ARG and f(C_=36, dtype=7) == SHAPE and f(nb=nb - 1, dtype=7) == SHAPE
    assert fwd(hpool=None) == ARG and bwd(dh=None) == ARG
    assert bwd(hid=257) == SHAPE and bwd(hid=512) == SHAPE, "the backward takes at most 256 hidden units"
    assert bwd(ws=None) == WORKSPACE and bwd(ws_bytes=ws_bytes - 1) == WORKSPACE and bwd(ws_bytes=0) == WORKSPACE
    assert bwd(dtype=7, ws_bytes=ws_bytes - 1) == DTYPE and bwd(hid=257, ws_bytes=0) == SHAPE
    assert m.untouched()

    plan = _lib.DenseProjPlan(*([-77] * 8))
    assert lib.cy_dense_proj_plan(32, 128, _lib.CY_BF16, 0.01, None) == ARG
    for args, rc in (((0, 128, _lib.CY_BF16), SHAPE), ((36, 128, _lib.CY_BF16), SHAPE), ((32, 0, _lib.CY_BF16), SHAPE),
                     ((32, 128, 7), DTYPE)):
        assert lib.cy_dense_proj_plan(*args, 0.01, plan) == rc, args
        assert [getattr(plan, f) for f, _ in plan._fields_] == [-77] * 8, args

    # the pools and the gather
    def avg_f(x="x", out="hpool", N=N, nb=nb, ldx=Cc, sh=sh, sw=sw, dtype=_lib.CY_BF16):
        return lib.cy_adaptive_avgpool_fwd(None if x is None else m[x], None, nb, None if out is None else m[out], N, H, W,
                                           Cc, ldx, sh, sw, dtype, None)

    def avg_b(dp="dh", dx="dx", N=N, ldx=Cc, sh=sh, sw=sw, dtype=_lib.CY_BF16):
        return lib.cy_adaptive_avgpool_bwd(None if dp is None else m[dp], None if dx is None else m[dx], N, H, W, Cc, ldx,
                                           sh, sw, dtype, None)

    def max_f(x="x", out="hpool", arg="ws", N=N, ldx=Cc, sh=sh, sw=sw, dtype=_lib.CY_BF16):
        p = lambda k: None if k is None else m[k]  # noqa: E731
        return lib.cy_adaptive_maxpool_fwd(p(x), p(out), p(arg), N, H, W, Cc, ldx, sh, sw, dtype, None)

    def max_b(dp="dh", arg="ws", dx="dx", N=N, ldx=Cc, sh=sh, sw=sw, dtype=_lib.CY_BF16):
        p = lambda k: None if k is None else m[k]  # noqa: E731
        return lib.cy_adaptive_maxpool_bwd(p(dp), p(arg), p(dx), N, H, W, Cc, ldx, sh, sw, dtype, None)

    assert avg_f(x=None) == ARG and avg_f(out=None) == ARG and avg_f(nb=0) == ARG and avg_f(nb=nb - 1) == SHAPE
    assert avg_b(dp=None) == ARG and avg_b(dx=None) == ARG
    assert max_f(x=None) == ARG and max_f(out=None) == ARG and max_f(arg=None) == ARG
    assert max_b(dp=None) == ARG and max_b(arg=None) == ARG and max_b(dx=None) == ARG
    for f in (avg_f, avg_b, max_f, max_b):
        assert f(N=0) == ARG and f(ldx=Cc - 1) == SHAPE and f(sh=H + 1) == SHAPE and f(sw=W + 1) == SHAPE, f.__name__
        assert f(sh=0) == SHAPE and f(dtype=7) == DTYPE and f(N=0, sh=0) == ARG and f(sh=0, dtype=7) == SHAPE, f.__name__
    g = lambda fn, a="x", i="ws", o="dx", M=4, D=4: fn(None if a is None else m[a], None if i is None else m[i],  # noqa: E731
                                                       None if o is None else m[o], M, D, None)
    for fn in (lib.cy_gather_rows_fwd, lib.cy_gather_rows_bwd):
        assert g(fn, a=None) == ARG and g(fn, i=None) == ARG and g(fn, o=None) == ARG and g(fn, M=0) == ARG and g(fn, D=0) == ARG
    assert m.untouched()
