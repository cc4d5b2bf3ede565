"""tests/test_gpu_pica_stream.py claims to take every grid-stride loop of csrc/cy_pica.hip round a second time, the
displacement loop of puiseg_loss_kernel past 256, the maxima K = 64 and m = 8, a skipped map of jsd_bwd_kernel that is
not the last, the clamped column norm of pui_loss_kernel, and the balance term of PUISegLoss on input where it matters.
The claims are conditions on the case tables (tests/pica_stream_cases.py), on the constants parsed out of the source and
on the f64 formulas (tests/patch_losses_cases.py) alone, so they are checked here without a GPU.  Each assertion names
its condition: deleting a case fails here, by name."""
import math
import re
from pathlib import Path

import pytest
import torch

import patch_losses_cases as pc
import patch_losses_fixture as fx
import pica_stream_cases as ps

REPO = Path(__file__).resolve().parents[1]
SOURCE = REPO / "contrast-you_amd" / "csrc" / "cy_pica.hip"
STREAMING = ("rows_axpb_kernel", "pixmean_entropy_fwd_kernel", "pixmean_entropy_bwd_kernel", "jsd_fwd_kernel",
             "jsd_bwd_kernel", "prior_fwd_kernel", "prior_bwd_kernel")


def test_constants_and_launches_match_the_source():
    text = SOURCE.read_text()
    consts = dict(re.findall(r"constexpr int (STREAM_GRID_CAP|PK_KMAX|JSD_MMAX) = (\d+);", text))
    assert consts == {"STREAM_GRID_CAP": str(ps.STREAM_GRID_CAP), "PK_KMAX": str(ps.PK_KMAX),
                      "JSD_MMAX": str(ps.JSD_MMAX)}
    assert ps.ONE_TRIP == ps.STREAM_GRID_CAP * 256 == 262144
    # every grid (and every workspace size) of the file is cy_blocks(items, 256, STREAM_GRID_CAP)
    calls = re.findall(r"\bcy_blocks\(([^,]+), (\w+), (\w+)\)", text)
    assert len(calls) == 9 and {c[1:] for c in calls} == {("256", "STREAM_GRID_CAP")}, calls
    assert {c[0] for c in calls} == {"R", "M", "R * K", "R * C"}, "two backward grids count elements, not positions"
    # every streaming kernel walks `+= (long)gridDim.x * 256L` from `blockIdx.x * 256L + threadIdx.x`
    assert text.count("+= (long)gridDim.x * 256L") == len(STREAMING) == text.count("= blockIdx.x * 256L + threadIdx.x;")
    for k in STREAMING:
        assert len(re.findall(rf"\b{k}\(", text)) == 1 and len(re.findall(rf"hipLaunchKernelGGL\({k},", text)) == 1, k
    # the grids of the two element-counting backwards, by their launch lines
    assert re.search(r"rows_axpb_kernel, dim3\(cy_blocks\(R \* K, 256, STREAM_GRID_CAP\)\)", text)
    assert re.search(r"prior_bwd_kernel, dim3\(cy_blocks\(R \* C, 256, STREAM_GRID_CAP\)\)", text)
    assert "for (int d = tid; d < TT; d += 256)" in text, "the displacement loop of puiseg_loss_kernel"
    assert "if (!dx.p[i]) continue;" in text, "the skipped map of jsd_bwd_kernel"
    assert "atomicAdd" not in text and "__hip_atomic" not in text


def test_the_restated_launch_rule():
    # the static_asserts of csrc/cy_common.h
    assert [ps.cy_blocks(n, 256, 8192) for n in (0, 1, 256, 257, 8192 * 256 + 1)] == [1, 1, 1, 2, 8192]
    assert ps.cy_blocks(1025, 1024, 2048) == 2
    assert ps.trips(ps.ONE_TRIP) == 1 and ps.trips(ps.ONE_TRIP + 1) == 2
    # the library's own count, where a host function gives it away (8 bytes per block)
    from cyhip import _lib, ops
    lib = _lib.load()
    for n in (1, 256, 257, 4100, ps.ONE_TRIP, ps.PAST_CAP):
        assert lib.cy_stream_sum_ws_bytes(n) == 8 * ps.cy_blocks(n, 256, ps.STREAM_GRID_CAP), n
    assert ops.PICA_KMAX == ps.PK_KMAX and ops.JSD_MAPS == (2, ps.JSD_MMAX)


def test_the_past_cap_size():
    assert ps.PAST_CAP == 513 * 513 == ps.ONE_TRIP + 4 * 256 + 1
    assert ps.trips(ps.PAST_CAP) == 2
    assert ps.last_owner(ps.PAST_CAP) == (1, 4, 0), "the last item: thread 0 of block 4 in the second trip"
    assert ps.PAST_CAP < 1.01 * ps.ONE_TRIP, "past one trip by less than 1 %"


# ---------------------------------------------------------------------------------------------- JSD_div
def test_jsd_past_cap_cases():
    c = ps.by_name(ps.JSD_CASES, "cap_nchw_none")
    assert (c.m, c.shape, c.fmt, c.reduction, c.needs) == (3, (1, 4, 513, 513), "nchw", "none", None)
    assert ps.trips(ps.jsd_positions(c)) == 2, "out_map and the per-position upstream gradient in the second trip"
    c = ps.by_name(ps.JSD_CASES, "cap_nhwc_mean")
    assert (c.m, c.shape, c.fmt, c.reduction, c.needs) == (2, (1, 4, 513, 513), "nhwc", "mean", None)
    assert ps.trips(ps.jsd_positions(c)) == 2
    c = ps.by_name(ps.JSD_CASES, "cap_rows_sum")
    assert (c.m, c.shape, c.fmt, c.reduction, c.needs) == (2, (ps.PAST_CAP, 3), "rows", "sum", None)
    assert ps.trips(ps.jsd_positions(c)) == 2
    assert {c.reduction for c in ps.JSD_CASES if ps.trips(ps.jsd_positions(c)) == 2} == {"none", "mean", "sum"}
    assert {c.fmt for c in ps.JSD_CASES if ps.trips(ps.jsd_positions(c)) == 2} == {"nchw", "nhwc", "rows"}


def test_jsd_maxima_and_the_skipped_maps():
    for name, fmt, red in (("m8_none", "nchw", "none"), ("m8_sum", "nhwc", "sum")):
        c = ps.by_name(ps.JSD_CASES, name)
        assert (c.m, c.shape, c.fmt, c.reduction) == (ps.JSD_MMAX, (2, ps.PK_KMAX, 5, 7), fmt, red), name
        assert c.needs == (0, 5), "gradients on maps 0 and 5 only"
        skipped = [i for i in range(c.m) if i not in c.needs]
        assert len(skipped) == 6 and any(i < max(c.needs) for i in skipped), \
            "a skipped map in front of a wanted one: `break` for `continue` loses map 5"
        assert c.needs[-1] != c.m - 1 and c.m - 1 in skipped


def test_jsd_one_class_is_not_a_simplex():
    c = ps.by_name(ps.JSD_CASES, "c1")
    assert (c.m, c.shape) == (2, (2, 1, 9, 7))
    xs = ps.jsd_inputs(c)
    assert all(0.05 <= float(x.min()) and float(x.max()) <= 1.0 for x in xs)
    assert all(float((x - 1.0).abs().max()) > 0.5 for x in xs), "not the one-class simplex (all ones)"
    v, _ = pc.reference(ps.jsd_formula(c), xs)
    assert abs(float(v)) > 1e-3, "a value a relative check can speak about"


def test_jsd_row_counts_around_one_block():
    rows = {c.shape[0]: c for c in ps.JSD_CASES if c.fmt == "rows" and c.shape[1] == 5}
    assert set(rows) == {1, 255, 256, 257}
    assert {ps.cy_blocks(r, 256, ps.STREAM_GRID_CAP) for r in rows} == {1, 2}
    assert {c.reduction for c in rows.values()} == {"none", "mean", "sum"}


def test_jsd_exact_zeros():
    c = ps.by_name(ps.JSD_CASES, "cap_zeros")
    assert ps.trips(ps.jsd_positions(c)) == 2 and c.m == 2
    a, b = ps.jsd_inputs(c)
    k = ps.ZERO_CLASS
    both = (a[:, k] == 0) & (b[:, k] == 0)
    one = (a[:, k] == 0) & (b[:, k] > 0)
    assert int(both.sum()) == 100 * 513, "class 1 exactly 0 in both maps on 100 image rows: the mean is exactly 0"
    assert int(one.sum()) == 50 * 513, "class 1 exactly 0 in map 0 only on another 50 image rows"
    assert bool(both[:, ps.ZERO_BOTH].all()) and bool(one[:, ps.ZERO_ONE].all())
    assert bool(((a[:, k] + b[:, k])[both] == 0).all())
    v, grads = pc.reference(ps.jsd_formula(c), [a, b])
    assert math.isfinite(float(v)) and all(bool(torch.isfinite(g).all()) for g in grads)
    # where both are 0 the gradient is exactly 0; where one is, it is the largest of the map
    assert bool((grads[0][:, k][both] == 0).all()) and bool((grads[1][:, k][both] == 0).all())
    assert float(grads[0][:, k][one].abs().min()) > 10.0


# ---------------------------------------------------------------------------------------------- EntropyPrior
def test_prior_cases():
    c = ps.by_name(ps.PRIOR_CASES, "cap_given")
    R, C = c.shape
    assert (R, C, c.given) == (ps.PAST_CAP, 2, True)
    assert ps.trips(R) == 2 and ps.trips(R * C) == 3, "forward and backward both past the cap"
    c = ps.by_name(ps.PRIOR_CASES, "bwd_cap_k64")
    R, C = c.shape
    assert (R, C, c.given) == (4100, ps.PK_KMAX, False)
    assert ps.cy_blocks(R, 256, ps.STREAM_GRID_CAP) == 17 and ps.trips(R) == 1, "the forward is below the cap"
    assert R * C == ps.ONE_TRIP + 256 and ps.trips(R * C) == 2, "the backward is past it"
    c = ps.by_name(ps.PRIOR_CASES, "c1")
    assert c.shape == (300, 1) and not c.given
    x, _ = ps.prior_inputs(c)
    assert float(x.min()) > 0 and float((x - 1).abs().max()) > 0.5, "positive rows, not the one-class simplex"
    assert ps.by_name(ps.PRIOR_CASES, "r1").shape[0] == 1
    assert {c.given for c in ps.PRIOR_CASES} == {True, False}
    for c in ps.PRIOR_CASES:
        x, prior = ps.prior_inputs(c)
        assert (prior is not None) == c.given and (prior is None or prior.shape == (1, c.shape[1]))
        v, (g,) = pc.reference(ps.prior_formula(prior), [x])
        assert math.isfinite(float(v)) and abs(float(v)) > 1e-3 and bool(torch.isfinite(g).all()), c.name


# ---------------------------------------------------------------------------------------------- PUILoss
def test_pui_cases():
    c = ps.by_name(ps.PUI_CASES, "4100x64")
    assert (c.N, c.K) == (4100, ps.PK_KMAX)
    assert c.N * c.K == ps.ONE_TRIP + 256 and ps.trips(c.N * c.K) == 2, "rows_axpb_kernel past its cap"
    c = ps.by_name(ps.PUI_CASES, "5x33")
    assert (c.N, c.K) == (5, 33) and 256 // c.K == 7 and (256 // c.K) * c.K == 231, "nsl = 7, 231 live threads"
    c = ps.by_name(ps.PUI_CASES, "3x2")
    assert (c.N, c.K) == (3, 2) and c.N < 256 // c.K, "fewer rows than slices"
    assert all(c.K > 1 for c in ps.PUI_CASES), "K = 1 is left out: dy is exactly 0 there"
    for c in ps.PUI_CASES:
        x, y = ps.pui_inputs(c)
        assert float(x.min()) > 0, "no zero column of x: p log p"
        s = x.sum(1)
        assert float(s.max() / s.min()) > 1.2 or c.N < 10, f"{c.name}: rows are not simplex"


def test_pui_clamped_column():
    for name, value in (("clamped_300x6", 0.0), ("tiny_300x6", 1e-14)):
        c = ps.by_name(ps.PUI_CASES, name)
        assert (c.N, c.K, c.column) == (300, 6, value)
        x, y = ps.pui_inputs(c)
        k = ps.CLAMPED_COLUMN
        assert bool((y[:, k] == value).all()) and float(y.double()[:, k].norm()) < 1e-12, "the norm is below the clamp"
        others = [j for j in range(c.K) if j != k]
        assert float(y.double()[:, others].norm(dim=0).min()) > 1.0
        v, (dx, dy) = pc.reference(ps.pui_formula, [x, y])
        assert math.isfinite(float(v)) and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dy).all())
        big, small = float(dy[:, k].abs().max()), float(dy[:, others].abs().max())
        assert big > 1e9 and small < 1.0, "the clamped column is compared apart: it would hide the others"
    x, y = ps.pui_inputs(ps.by_name(ps.PUI_CASES, "tiny_300x6"))
    J = x.double().t() @ y.double()
    assert float(J[:, ps.CLAMPED_COLUMN].abs().min()) > 0, "a clamped column whose joint is not 0"


# ---------------------------------------------------------------------------------------------- PUISegLoss
def test_the_fixture_feeds_the_balance_term_a_constant(golden_dir):
    """the blind spot, stated: on a softmax the per-pixel class mean is 1 / k on every pixel"""
    npz = fx.load(golden_dir)
    for tag, (shape, _) in fx.PUISEG_CASES.items():
        for x in fx.inputs(npz, tag):
            assert ps.pixel_mean_spread(x) - 1.0 < 1e-6, tag
            assert float((x.double().mean(1) - 1.0 / shape[1]).abs().max()) < 1e-7, tag


def test_puiseg_inputs_are_not_simplex():
    for c in ps.SEG_CASES:
        a, b = ps.seg_inputs(c)
        assert a.shape == c.shape and b.shape == c.shape
        assert ps.pixel_mean_spread(a) > 2.0 and ps.pixel_mean_spread(b) > 2.0, c.name
        assert c.pad < min(c.shape[2:]), c.name
        v, grads = pc.reference(ps.seg_formula(c), [a, b])
        assert math.isfinite(float(v)) and all(bool(torch.isfinite(g).all()) for g in grads), c.name


def test_puiseg_cases():
    c = ps.by_name(ps.SEG_CASES, "cap")
    n, k, H, W = c.shape
    assert (c.shape, c.pad, c.lamda) == ((1, 2, 513, 513), 1, 2.0) and ps.trips(n * H * W) == 2
    c = ps.by_name(ps.SEG_CASES, "tt289")
    TT = (2 * c.pad + 1) ** 2
    assert c.shape == (1, 2, 20, 20) and TT == 289 and TT > 256 and c.pad < min(c.shape[2:])
    assert max((2 * p + 1) ** 2 for _, p in fx.PUISEG_CASES.values()) <= 256, "no fixture case goes past 256"
    c = ps.by_name(ps.SEG_CASES, "k64")
    assert c.shape == (1, ps.PK_KMAX, 6, 5) and c.pad == 1 and c.shape[1] ** 2 == 4096
    small = [c for c in ps.SEG_CASES if c.name != "cap"]
    assert all({f for f, _ in c.runs} == {"nchw", "nhwc"} for c in small), "both memory formats for the small cases"
    needs = {n for c in ps.SEG_CASES for _, n in c.runs}
    assert needs == {ps.BOTH, ps.X1_ONLY, ps.X2_ONLY}


def test_puiseg_balance_term_dominates_at_lamda_2():
    c0, c2 = ps.by_name(ps.SEG_CASES, "lam0"), ps.by_name(ps.SEG_CASES, "lam2")
    assert (c0.shape, c0.pad, c0.lamda) == ((2, 5, 13, 11), 2, 0.0)
    assert (c2.shape, c2.pad, c2.lamda) == (c0.shape, 2, 2.0)
    xs0, xs2 = ps.seg_inputs(c0), ps.seg_inputs(c2)
    assert all(torch.equal(a, b) for a, b in zip(xs0, xs2)), "the same input"
    v0, g0 = pc.reference(ps.seg_formula(c0), xs0)
    v2, g2 = pc.reference(ps.seg_formula(c2), xs2)
    balance, ce = g2[0] - g0[0], g0[0]
    assert float(balance.norm()) > 10 * float(ce.norm()), "the balance part of dx1 exceeds the ce part by 10x"
    assert float(balance.abs().min()) > 10 * float(ce.abs().max()), "on every element"
    assert abs(float(v2 - v0)) > 10 * abs(float(v0))
    assert torch.equal(g0[1], g2[1]), "dx2 has no balance part"
    # a kernel reading a neighbouring pixel would be seen: the balance gradient differs from pixel to pixel
    per_pixel = balance[:, 0].flatten()
    assert float((per_pixel[1:] - per_pixel[:-1]).abs().min()) > 0
    assert float(balance.std()) > 0.05 * float(balance.abs().mean())
    assert float((balance - balance[:, :1]).abs().max()) < 1e-12, "the same number on every class of a pixel"


def test_same_bits_cases_are_past_cap():
    assert set(ps.SAME_BITS) == {"jsd", "prior", "pui", "seg"}
    c = ps.by_name(ps.JSD_CASES, ps.SAME_BITS["jsd"])
    assert ps.trips(ps.jsd_positions(c)) == 2
    c = ps.by_name(ps.PRIOR_CASES, ps.SAME_BITS["prior"])
    assert ps.trips(c.shape[0]) == 2
    c = ps.by_name(ps.PUI_CASES, ps.SAME_BITS["pui"])
    assert ps.trips(c.N * c.K) == 2
    c = ps.by_name(ps.SEG_CASES, ps.SAME_BITS["seg"])
    assert ps.trips(c.shape[0] * c.shape[2] * c.shape[3]) == 2


def test_the_tolerance_rule(golden_dir):
    stored = ps.fixture_e_ref(fx.load(golden_dir))
    assert set(stored) == set(fx.KINDS)
    assert fx.tolerances(fx.load(golden_dir)) == {k: ps.bound(v, 0.0) for k, v in stored.items()}, "the fixture's rule"
    assert ps.bound(1e-9, 1e-9) == 1e-6 and ps.bound(1e-9, 1e-5) == pytest.approx(4e-5) and ps.bound(1e-4, 1e-5) == 4e-4
    t = ps.tolerances(stored, 0.0, (0.0, 0.0))
    assert set(t) == {"scalar", "grad2", "gradmax"}
