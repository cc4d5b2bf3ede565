"""tests/test_gpu_step_kernels.py claims to reach the grid-stride loops, the channel tails, the geometric edges of the
affine kernels and both branches of the RAdam step (csrc/cy_misc.hip).  The claims are conditions on the case tables
(tests/step_kernel_cases.py) and on the reference alone, so they are checked here on the CPU: none of them depends on
the code under test.  Each assertion names its condition: deleting a case fails here, by name, without a GPU."""
import re
from pathlib import Path

import pytest
import torch

from tests import step_kernel_cases as sc

REPO = Path(__file__).resolve().parents[1]


def picks(theta, H, W):
    """(src [H*W], valid [H*W], px [H*W]) of one theta, from the oracle's definition"""
    from oracle.losses import affine_source_index
    t = torch.tensor([theta.rows], dtype=torch.float32)
    src, valid = affine_source_index(t, H, W)
    t64 = t.double()[0]
    xo = ((2 * torch.arange(W, dtype=torch.float64) + 1) / float(W) - 1.0).view(1, W)
    yo = ((2 * torch.arange(H, dtype=torch.float64) + 1) / float(H) - 1.0).view(H, 1)
    xi = (t64[0, 0] * xo + t64[0, 1] * yo) + t64[0, 2]
    px = ((xi + 1.0) * float(W) - 1.0) * 0.5
    return src[0], valid[0], px.reshape(-1)


def contributions(theta, H, W):
    src, valid, _ = picks(theta, H, W)
    return torch.bincount(src[valid], minlength=H * W).view(H, W)


def test_grid_cap_matches_the_source():
    text = (REPO / "contrast-you_amd" / "csrc" / "cy_misc.hip").read_text()
    assert re.findall(r"constexpr int GRID_CAP = (\d+);", text) == [str(sc.GRID_CAP)], "the cap of the four grids"
    # every grid of the file is cy_blocks(items, 256, GRID_CAP) (csrc/cy_common.h): 256 items per block, that cap
    calls = re.findall(r"\bcy_blocks\((.*?), (\w+), (\w+)\)[;)]", text)
    assert len(calls) == 4 and {c[1:] for c in calls} == {("256", "GRID_CAP")}, calls
    assert sc.ONE_TRIP == sc.GRID_CAP * 256
    # every kernel of the four walks `+= (long)gridDim.x * 256L` from `blockIdx.x * 256L + threadIdx.x`
    assert text.count("+= (long)gridDim.x * 256L") == 4 and text.count("dim3(256)") >= 4


def test_element_counts_and_past_cap_cases():
    assert sc.ELEMENT_COUNTS == (1, 255, 256, 257, sc.ONE_TRIP, sc.ONE_TRIP + 257)
    big = sc.ELEMENT_COUNTS[-1]
    # second trip: workgroup 0 takes 256 items, thread 0 of workgroup 1 the last
    assert big - sc.ONE_TRIP == 256 + 1
    g = sc.AFFINE_CAP
    items = g.N * g.H * g.W * (-(-g.C // 8))
    assert items == 2102784
    for what, n in (("EMA / RAdam", big), ("affine", items)):
        assert sc.ONE_TRIP < n < 1.05 * sc.ONE_TRIP, f"{what}: past one trip by less than 5 %"
        assert n % sc.ONE_TRIP, what
    assert g.C % 8 and g.C > 8, "the past-cap affine case has a full channel group and a tail group"
    assert sc.AFFINE_CAP_TYPE == "bf16"
    assert set(sc.RADAM_COUNTS_ALL_SETS) == {257, sc.ONE_TRIP + 257}
    cases = sc.radam_cases()
    for s in sc.RADAM_SETS:
        counts = {n for t, _, n in cases if t is s}
        assert counts >= set(sc.RADAM_COUNTS_ALL_SETS), s.name
        assert (counts == set(sc.ELEMENT_COUNTS)) == (s.name == "trainer"), s.name
    assert sc.SLICE_OFF == 3 and sc.GUARD >= 1
    assert set(sc.EMA_ALPHAS) == {0.0, 0.5, 0.999} and set(sc.EMA_WDS) == {0.0, 1e-5}


def test_affine_geometries_types_and_channel_tails():
    want = {(3, 12, 10, 23), (3, 12, 23, 10), (2, 4, 16, 16), (2, 1, 16, 16), (2, 8, 7, 9), (2, 20, 7, 9), (1, 3, 1, 1),
            (1, 3, 1, 9), (1, 3, 9, 1)}
    assert {tuple(g) for g in sc.AFFINE_GEOMS} == want
    assert set(sc.TYPES) == {"f32", "bf16", "f16"}
    groups = {(g.C // 8, g.C % 8) for g in sc.AFFINE_GEOMS}
    assert (0, 4) in groups and (1, 0) in groups and (1, 4) in groups and (2, 4) in groups and (0, 1) in groups, \
        "tail only, one full group, full + tail, two full + tail, one channel"
    assert {g.C for g in sc.GAMMA_GEOMS} == {1, 4, 12} and set(sc.GAMMAS) == {0.5, 1.0, 1.7, 2.0}
    assert all(g.N == len(sc.GAMMAS) for g in sc.GAMMA_GEOMS), "one gamma per image"
    # every theta meets every image index of every geometry
    for g in sc.AFFINE_GEOMS:
        for n in range(g.N):
            assert {sc.batch_thetas(k, g.N)[n].name for k in range(len(sc.THETAS))} == set(sc.THETA_NAMES)


def test_theta_list():
    from oracle.losses import make_theta
    args = {"prod-identity": (1.0, 0.0, 0.0, 0.0, False, False),
            "prod-1.25-30-flipw": (1.25, 30.0, 0.08, -0.05, False, True),
            "prod-0.82-m41-fliph": (0.82, -41.0, -0.1, 0.1, True, False),
            "prod-1.1-12-flipboth": (1.1, 12.0, 0.02, 0.03, True, True),
            "scale-0.25": (0.25, 0.0, 0.0, 0.0, False, False), "scale-4": (4.0, 0.0, 0.0, 0.0, False, False)}
    by_name = {t.name: t for t in sc.THETAS}
    for name, a in args.items():
        assert torch.equal(torch.tensor(by_name[name].rows, dtype=torch.float32), make_theta(*a)), name
        assert sc.make_theta_rows(*a) == by_name[name].rows
    assert len(sc.THETAS) == 13 and len(set(sc.THETA_NAMES)) == 13
    assert len(sc.PRODUCTION_THETAS) == 5 and by_name["identity"].rows == ((1, 0, 0), (0, 1, 0))
    for t in sc.THETAS:   # the entries are f32 values: the tensor the kernel reads holds exactly these
        assert all(sc.f32(v) == v for r in t.rows for v in r), t.name
    assert abs(by_name["scale-0.25"].rows[0][0] - 4) < 1e-6 and abs(by_name["scale-4"].rows[0][0] - 0.25) < 1e-6
    assert by_name["half-pixel"].rows[0][2] == 1 / 16 and by_name["translate-3"].rows[0][2] == 3.0
    assert sc.det(by_name["rank-1"].rows) == 0 and sc.det(by_name["rank-0"].rows) == 0
    near = by_name["near-singular"]
    d = sc.det(near.rows)
    assert f"{d:.3e}" in near.note, "the determinant is recorded in the case note"
    assert abs(d) < 1e-6 * abs(near.rows[0][0] * near.rows[1][1]), "near-singular: |det| below 1e-6 of its terms"
    first = [sc.f32(v) for v in (0.9, 0.4, 0.02)]
    assert list(near.rows[0]) == first and list(near.rows[1]) == [sc.f32(v * (1 + 1e-6)) for v in (0.9, 0.4, 0.02)]
    assert near.rows[1] != near.rows[0], "1 + 1e-6 survives the rounding to f32"
    assert all(sc.det(t.rows) != 0 for t in sc.THETAS if t.kind in ("production", "wide"))


def test_valid_fraction_of_every_geometry_and_theta():
    """a kernel that returns zero must not pass: enough of every output is inside the source image"""
    for g in sc.AFFINE_GEOMS:
        for t in sc.THETAS:
            _, valid, _ = picks(t, g.H, g.W)
            frac = valid.double().mean().item()
            if t.name == "translate-3":
                assert frac == 0, "every source outside: output and dx all zero"
            elif g.H * g.W == 1:
                continue
            elif t.name == "scale-0.25":
                # entries of 4 put 1/16 of the output plane inside the source whatever the size, so 25 % cannot hold
                # for this theta; half of what the geometry allows must.  test_sparse_and_dense_pre_images asks for
                # the gaps between its picks
                assert frac >= 1 / 32, f"{sc.ident(g)} under {t.name}: only {frac:.3f} of the output pixels are valid"
            else:
                assert frac >= 0.25, f"{sc.ident(g)} under {t.name}: only {frac:.2f} of the output pixels are valid"


def test_sparse_and_dense_pre_images():
    by_name = {t.name: t for t in sc.THETAS}
    most = {t.name: max(int(contributions(t, g.H, g.W).max()) for g in sc.AFFINE_GEOMS) for t in sc.THETAS}
    assert most["scale-4"] >= 8 and most["rank-0"] >= 8, most
    assert most["rank-0"] == 16 * 16, "rank 0: every output pixel of the largest image picks one source pixel"
    gaps = 0
    for g in sc.AFFINE_GEOMS:
        k = contributions(by_name["scale-0.25"], g.H, g.W)
        if g.W > 1:
            gaps += int(((k[:, :-1] == 0) & (k[:, 1:] > 0)).sum())
    assert gaps > 0, "scale 0.25: a pixel without contributions next to one with some"
    # rank 1: contributions only on a line, several per pixel
    k = contributions(by_name["rank-1"], 16, 16)
    assert int((k > 0).sum()) <= 16 and int(k.max()) >= 8


def test_half_pixel_theta_produces_ties():
    t = {t.name: t for t in sc.THETAS}["half-pixel"]
    hit = False
    for g in sc.AFFINE_GEOMS:
        src, _, px = picks(t, g.H, g.W)
        ties = (px - torch.floor(px)) == 0.5
        if g.W == 16:
            assert bool(ties.all()), "px = ox + 0.5 exactly on a width of 16"
            assert set((src % g.W).tolist()) <= {0, 2, 4, 6, 8, 10, 12, 14, 15}, "ties go to the even pixel"
            hit = True
    assert hit, "a geometry of width 16"


def test_non_square_geometries_differ_from_their_transposes():
    """the W/H and H/W factors of the backward window are 1 on a square image"""
    a, b = sc.AFFINE_GEOMS[0], sc.AFFINE_GEOMS[1]
    assert (a.H, a.W) == (b.W, b.H) and a.H != a.W
    rotated = [t for t in sc.THETAS if t.rows[0][1] != 0 and t.kind in ("production", "wide")]
    assert len(rotated) >= 4
    for t in rotated:
        sa, va, _ = picks(t, a.H, a.W)
        sb, vb, _ = picks(t, b.H, b.W)
        # picks of the transposed geometry, read back in the first one's coordinates
        sy, sx = sb.view(b.H, b.W) // b.W, sb.view(b.H, b.W) % b.W
        sb_t = (sx * a.W + sy).t().reshape(-1)
        vb_t = vb.view(b.H, b.W).t().reshape(-1)
        assert not (torch.equal(va, vb_t) and torch.equal(sa[va], sb_t[vb_t])), t.name


def test_radam_steps_straddle_the_rectification_switch():
    assert [tuple(s[1:]) for s in sc.RADAM_SETS] == [(0.9, 0.999, 1e-8, 1e-5, 1e-3), (0.9, 0.999, 1e-8, 0.0, 1e-3),
                                                    (0.8, 0.99, 1e-6, 1e-2, 1e-2), (0.9, 0.5, 1e-8, 0.0, 1e-3)]
    assert any(s.wd == 0 for s in sc.RADAM_SETS) and any(s.wd != 0 for s in sc.RADAM_SETS), "both weight-decay branches"
    for s in sc.RADAM_SETS:
        steps = sc.radam_steps(s)
        assert 1 in steps and 1000 in steps and 100000 in steps, s.name
        if sc.rho_inf(s.beta2) <= 5.0:   # rho_t = rho_inf - (a positive term): never above 5
            assert s.name == "never-rectified" and sc.rho_inf(s.beta2) == 3.0
            assert not any(sc.rectified(s.beta2, t) for t in steps)
            assert not any(sc.rectified(s.beta2, t) for t in (10, 10 ** 4, 10 ** 7))
            continue
        t = sc.first_rectified_step(s.beta2)
        assert {t - 1, t, t + 1} <= set(steps), s.name
        assert not sc.rectified(s.beta2, t - 1) and sc.rectified(s.beta2, t) and sc.rectified(s.beta2, t + 1), s.name
        assert sc.rho_t(s.beta2, t - 1) <= 5.0 < sc.rho_t(s.beta2, t)
        assert sc.rectified(s.beta2, 1000) and not sc.rectified(s.beta2, 1)
        # saturated bias corrections at 100 000: 1 - beta^t rounds to 1 in f32
        assert sc.f32(1.0 - sc.f32(s.beta1) ** 100000) == 1.0 and sc.f32(1.0 - sc.f32(s.beta2) ** 100000) == 1.0


def test_measured_bounds_follow_the_rule():
    """bound = 4 x yardstick"""
    assert sc.GAMMA_BOUND == pytest.approx(4 * sc.GAMMA_YARDSTICK)
    assert set(sc.RADAM_BOUND) == {"p", "exp_avg", "exp_avg_sq"}
    for k, v in sc.RADAM_YARDSTICK.items():
        assert sc.RADAM_BOUND[k] == pytest.approx(4 * v)
    # a yardstick is the error of an f32 computation: a few units of 2^-24, or it was measured on something else
    for v in (sc.GAMMA_YARDSTICK, *sc.RADAM_YARDSTICK.values()):
        assert 2.0 ** -26 <= v <= 2.0 ** -20


def test_fused_case():
    import math
    offs = [0]
    for shp in sc.FUSED_SHAPES:
        offs.append(offs[-1] + math.prod(shp))
    assert offs == [0, 35, 42, 63], "slices at element offsets that are no multiple of 4"
    assert sc.FUSED_STEPS == 12 and sc.FUSED_SKIP_UNTIL == 3 and sc.FUSED_RESUME_AFTER == 6
    assert (sc.FUSED_LR, sc.FUSED_WD) == (1e-2, 1e-5)
    # from step 4 on the lagging count of the second parameter crosses the switch later than its neighbours do
    t = sc.first_rectified_step(0.999)
    assert sc.FUSED_SKIP_UNTIL < t <= sc.FUSED_STEPS - sc.FUSED_SKIP_UNTIL, "both counts cross the switch within the run"
