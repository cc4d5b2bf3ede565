"""SLIC superpixels without a GPU: the properties of the NumPy restatement (tests/slic_cases.py) that make its output
usable by the superpixel hook, the refusals and the launch plan of csrc/cy_slic.hip against the cases, and the
kernel's f32 blur arithmetic against scipy's float64 blur."""
import numpy as np
import pytest
from scipy import ndimage

import slic_cases as sc


@pytest.mark.parametrize("name", list(sc.CASES))
def test_restatement_regions_are_connected_and_large_enough(name):
    """every final id is one 4-connected region, every region but a possible root-0 one has >= min_size pixels, and the
    ids fit the hook's uint8 read"""
    c = sc.case(name)
    _, _, ys, xs = sc.grid(c["H"], c["W"], c["n_segments"])
    min_size = (c["H"] * c["W"]) // (2 * len(ys) * len(xs))
    for n in range(c["N"]):
        ids, count = c["ids"][n], int(c["count"][n])
        assert count < 207
        assert sorted(np.unique(ids).tolist()) == list(range(count))
        for i in range(count):
            region = ids == i
            assert ndimage.label(region)[1] == 1, (name, n, i)
            assert region.sum() >= min_size or region.flat[0], (name, n, i, int(region.sum()))


def test_restatement_connect_on_long_and_tiny_components():
    sp = sc.spirals()
    comp, roots, sizes = sc.components(sp[0])
    assert len(roots) == 2 and sizes.min() > 1900  # two interleaved spirals, each about half the image
    assert sc.connect(sp, 4)[1].tolist() == [2]  # min_size 512: both kept
    ids, count = sc.connect(sp, 1)  # min_size 2048: the spiral of 0s (root in column 0) joins the pixel above it
    assert count.tolist() == [1] and not ids.any()
    speckle = sc.speckle(37, 53, 2, 9)
    assert len(sc.components(speckle[0])[1]) > 300
    ids, count = sc.connect(speckle, 20)
    assert 1 < int(count[0]) < 207
    assert all(ndimage.label(ids[0] == i)[1] == 1 for i in range(int(count[0])))


REFUSALS = [
    # N, H, W, n_segments, sigma, compactness, max_iter -> status
    ((1, 224, 224, 40, 5.0, 0.1, 10), sc.OK),
    ((1, 224, 224, 40, 5.0, 0.1, 0), sc.OK),
    ((0, 224, 224, 40, 5.0, 0.1, 10), sc.ERR_ARG),
    ((1, 224, 224, 40, 5.0, 0.1, -1), sc.ERR_ARG),
    ((1, 0, 224, 40, 5.0, 0.1, 10), sc.ERR_SHAPE),
    ((1, 1025, 224, 40, 5.0, 0.1, 10), sc.ERR_SHAPE),
    ((1, 224, 1025, 40, 5.0, 0.1, 10), sc.ERR_SHAPE),
    ((1, 1024, 1024, 40, 5.0, 0.1, 10), sc.OK),
    ((65536, 64, 64, 4, 1.0, 0.1, 10), sc.ERR_SHAPE),
    ((1, 224, 224, 40, -1.0, 0.1, 10), sc.ERR_ARG),
    ((1, 224, 224, 40, float("nan"), 0.1, 10), sc.ERR_ARG),
    ((1, 224, 224, 40, 16.0, 0.1, 10), sc.OK),
    ((1, 224, 224, 40, 16.5, 0.1, 10), sc.ERR_SHAPE),
    ((1, 20, 224, 4, 5.0, 0.1, 10), sc.OK),          # r = 20 = min(H, W)
    ((1, 19, 224, 4, 5.0, 0.1, 10), sc.ERR_SHAPE),   # r = 20 > 19
    ((1, 224, 224, 40, 5.0, 0.0, 10), sc.ERR_ARG),   # M = 0
    ((1, 224, 224, 40, 5.0, 7e-6, 10), sc.ERR_ARG),  # M = round(0.46) = 0
    ((1, 224, 224, 40, 5.0, 8e-6, 10), sc.OK),       # M = round(0.52) = 1
    ((1, 224, 224, 40, 5.0, 1.0, 10), sc.OK),        # M = 65535
    ((1, 224, 224, 40, 5.0, 1.01, 10), sc.ERR_ARG),
    ((1, 224, 224, 40, 5.0, float("inf"), 10), sc.ERR_ARG),
    ((1, 224, 224, 0, 5.0, 0.1, 10), sc.ERR_ARG),
    ((1, 224, 224, 100, 5.0, 0.1, 10), sc.OK),       # S = 22, K = 100
    ((1, 224, 224, 121, 5.0, 0.1, 10), sc.ERR_SHAPE),  # K = 121 > 100
    ((1, 37, 53, 40, 1.0, 0.1, 10), sc.ERR_SHAPE),   # K = 40: 64 K = 2560 > 1961 pixels
    ((1, 48, 48, 40, 1.0, 0.1, 10), sc.OK),          # K = 36: 64 K = 2304 = H W
    ((1, 30, 300, 1, 1.0, 0.1, 10), sc.ERR_SHAPE),   # start = 47 is past H: no centre
    ((1, 8, 8, 200, 0.0, 0.1, 10), sc.ERR_SHAPE),    # s = 0.57: S = 1, K = 64, 64 K > 64 pixels
    ((1, 8, 8, 1000, 0.0, 0.1, 10), sc.ERR_SHAPE),   # S = 0
]


@pytest.mark.parametrize("args,want", REFUSALS)
def test_plan_refusals_have_their_exact_status(args, want):
    from cyhip import _lib, ops
    assert sc.status(*args) == want  # the restatement's reading of the header agrees with the table
    plan = ops.slic_plan(*args)
    assert plan["status"] == want, plan
    N, H, W, n_segments = args[:4]
    nbytes = _lib.load().cy_slic_ws_bytes(N, H, W, n_segments)
    if want == sc.OK:
        assert nbytes >= 6 * 4 * N * H * W
    else:
        assert all(v == 0 for k, v in plan.items() if k != "status"), plan
        # the entry point refuses the same arguments before any launch (dummy pointers: nothing is read through them)
        p = 4096
        assert _lib.load().cy_slic(p, p, p, N, H, W, n_segments, args[4], args[5], args[6], p, 1 << 40, None) == want


def test_entry_points_refuse_null_pointers_and_short_workspaces():
    from cyhip import _lib
    lib = _lib.load()
    p, N, H, W, ns = 4096, 2, 64, 64, 16
    need = lib.cy_slic_ws_bytes(N, H, W, ns)
    assert need > 0 and lib.cy_slic_ws_bytes(N, H, W, 0) == 0 and lib.cy_slic_ws_bytes(N, 2000, W, ns) == 0
    assert lib.cy_slic(None, p, p, N, H, W, ns, 1.0, 0.1, 10, p, need, None) == sc.ERR_ARG
    assert lib.cy_slic(p, p, p, N, H, W, ns, 1.0, 0.1, 10, None, need, None) == sc.ERR_ARG
    assert lib.cy_slic(p, p, p, N, H, W, ns, 1.0, 0.1, 10, p, need - 1, None) == sc.ERR_WORKSPACE
    assert lib.cy_slic_blur_q(p, None, N, H, W, 1.0, p, need, None) == sc.ERR_ARG
    assert lib.cy_slic_blur_q(p, p, N, H, W, 17.0, p, need, None) == sc.ERR_SHAPE
    assert lib.cy_slic_blur_q(p, p, N, H, W, 1.0, p, 4 * N * H * W - 1, None) == sc.ERR_WORKSPACE
    assert lib.cy_slic_cluster(p, None, p, N, H, W, ns, 0.1, 10, p, need, None) == sc.ERR_ARG
    assert lib.cy_slic_cluster(p, p, p, N, H, W, ns, 0.0, 10, p, need, None) == sc.ERR_ARG
    assert lib.cy_slic_cluster(p, p, p, N, H, W, ns, 0.1, 10, p, need - 1, None) == sc.ERR_WORKSPACE
    assert lib.cy_slic_connect(p, p, None, N, H, W, ns, p, need, None) == sc.ERR_ARG
    assert lib.cy_slic_connect(p, p, p, N, H, W, 1000, p, need, None) == sc.ERR_SHAPE
    assert lib.cy_slic_connect(p, p, p, N, H, W, ns, p, need - 1, None) == sc.ERR_WORKSPACE
    assert lib.cy_slic_plan(N, H, W, ns, 1.0, 0.1, 10, None) == sc.ERR_ARG
    plan = _lib.SlicPlan()
    assert lib.cy_slic_plan(N, H, W, ns, 1.0, 0.1, 10, plan) == sc.OK and plan.K == 16


def test_plan_matches_the_cases_and_the_cases_reach_every_form():
    """the plan's geometry is the restatement's, and between them the cases reach both blur forms, more than one block
    in every grid direction, the largest blur tile, K = 1 and more than one tile of the numbering block"""
    from cyhip import _lib, ops
    plans = {}
    for name, c in sc.CASES.items():
        p = plans[name] = ops.slic_plan(c["N"], c["H"], c["W"], c["n_segments"], c["sigma"], c["compactness"])
        assert p["status"] == sc.OK, (name, p)
        S, start, ys, xs = sc.grid(c["H"], c["W"], c["n_segments"])
        HW = c["H"] * c["W"]
        assert (p["S"], p["start"], p["Ky"], p["Kx"], p["K"]) == (S, start, len(ys), len(xs), len(ys) * len(xs)), name
        assert p["r"] == sc.radius(c["sigma"]) and p["M"] == round(c["compactness"] * 65535), name
        assert p["min_size"] == HW // (2 * p["K"]) and HW >= 64 * p["K"], name
        assert p["K"] == sc.case(name)["centres"].shape[1]
        assert p["pixel_grid_x"] == -(-HW // 256) and p["scan_tiles"] == -(-HW // 1024), name
        assert p["update_grid"] == -(-c["N"] * p["K"] // 256), name
        assert p["assign_lds"] == 12 * _lib.CY_SLIC_MAX_K
        if c["sigma"] == 0:
            assert p["blur_form"] == _lib.CY_SLIC_BLUR_QUANT and p["launches"] == 1 + 1 + 20 + 5
            assert (p["blur_grid_x"], p["blur_grid_y"]) == (-(-HW // 256), c["N"])
            assert (p["blur_lds_h"], p["blur_lds_w"]) == (0, 0)
        else:
            assert p["blur_form"] == _lib.CY_SLIC_BLUR_TWO_PASS and p["launches"] == 2 + 1 + 20 + 5
            assert (p["blur_grid_x"], p["blur_grid_y"]) == (-(-c["W"] // 64), -(-c["H"] // 16)), name
            assert p["blur_lds_h"] == (16 + 2 * p["r"]) * 64 * 4 and p["blur_lds_w"] == 16 * (64 + 2 * p["r"]) * 4
            assert max(p["blur_lds_h"], p["blur_lds_w"]) + 4 * 65 <= 64 * 1024  # static + dynamic LDS of a block
    every = list(plans.values())
    assert {p["blur_form"] for p in every} == {_lib.CY_SLIC_BLUR_QUANT, _lib.CY_SLIC_BLUR_TWO_PASS}
    assert any(p["blur_grid_x"] > 1 and p["blur_grid_y"] > 1 and p["blur_form"] == 1 for p in every)
    assert any(p["r"] == 64 for p in every)  # the widest blur the family accepts: the largest LDS tile
    assert any(p["K"] == 1 for p in every) and any(p["K"] > 32 for p in every)
    assert any(p["pixel_grid_x"] > 1 for p in every) and any(p["scan_tiles"] > 1 for p in every)
    assert {c["N"] for c in sc.CASES.values()} >= {1, 5}
    # a window clipped on every side: the first and the last centre are nearer than 2S to the image's edges
    p, c = plans["odd_37x53"], sc.CASES["odd_37x53"]
    assert c["H"] % 2 and c["W"] % 2 and p["start"] < 2 * p["S"]
    assert c["H"] - 1 - (p["start"] + (p["Ky"] - 1) * p["S"]) < 2 * p["S"]
    assert c["W"] - 1 - (p["start"] + (p["Kx"] - 1) * p["S"]) < 2 * p["S"]


@pytest.mark.parametrize("H,W,sigma", sc.BLUR_CASES)
def test_f32_blur_in_tap_order_against_float64(H, W, sigma):
    """the kernel's arithmetic restated in NumPy f32 against scipy's float64 blur: |dq| <= 1, under 1 % of the pixels
    differ (two f32 passes of at most 129 taps err by about 1e-5, under one step of 1/65535)"""
    images = sc.blobs(2, H, W, seed=11)
    want, got = sc.blur_q_f64(images, sigma), sc.blur_q_f32(images, sigma)
    d = np.abs(want - got)
    print(f"{H}x{W} sigma {sigma}: max |dq| {d.max()}, {100 * (d > 0).mean():.3f} % differ")
    assert d.max() <= 1
    assert (d > 0).mean() < 0.01


def test_sigma_zero_only_quantises():
    images = sc.noise(1, 37, 53, 3)
    assert np.array_equal(sc.blur_q_f32(images, 0.0), sc.blur_q_f64(images, 0.0))
    assert np.array_equal(sc.blur_q_f32(images, 0.0)[0], np.floor(images[0].astype(np.float64) * 65535 + 0.5))


def test_python_surface_refuses_cpu_tensors_and_keeps_the_hooks_format():
    import torch
    from cyhip import ops
    from semi_seg import superpixel
    from semi_seg.hooks import OnlineSuperPixelInfoNCEHook, SuperPixelInfoNCEHook
    assert issubclass(OnlineSuperPixelInfoNCEHook, SuperPixelInfoNCEHook)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.slic(torch.rand(1, 1, 64, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        superpixel.slic_superpixels(torch.rand(1, 64, 64))
    ids = torch.arange(256, dtype=torch.uint8).view(1, 16, 16)
    entry = superpixel.as_batch_entry(ids)
    assert isinstance(entry, list) and entry[0].shape == (1, 1, 16, 16) and entry[0].dtype == torch.float32
    # what _SuperPixelInfoNCEEPochHook does with it gives every id back
    assert torch.equal((entry[0] * 255.0).type(torch.uint8)[:, 0], ids)
