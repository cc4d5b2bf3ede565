"""Every dispatch branch of the 1x1 head and every launch cap of the head / loss / cluster-head kernels is reached by
a parity case of tests/test_gpu_head_dispatch.py.  The launch plan is a pure host-side function of (npix, C, K)
(cy_head1x1_plan, cy_cluster_head_plan), so the claim is checked here on the CPU, against the same case lists the GPU
tests are parametrised with (tests/head_cases.py).  Where a feature is reached by one case only, the failure message of
its assertion names the feature, so removing that case shows up here and not as silently lost coverage."""
import pytest

from tests import head_cases as hc


def _plans():
    return [(c, hc.plan(c)) for c in hc.HEAD_CASES]


def _runs(c, what):
    """does the GPU test of case c launch the forward / the data gradient / the parameter gradients?"""
    return {"all": True, "fwd": what == "fwd", "dx": what == "dx", "dw": what == "dw", "mc": True}[c.parts]


def _need(have, want, what):
    missing = sorted(set(want) - set(have), key=str)
    assert not missing, f"no head case reaches {what}: {missing}"


def test_every_instantiation_and_load_path_has_a_case():
    plans = _plans()
    fwd = [(c, p) for c, p in plans if _runs(c, "fwd")]
    dx = [(c, p) for c, p in plans if _runs(c, "dx")]
    dw = [(c, p) for c, p in plans if _runs(c, "dw")]
    _need({(p["fwd_kernel"], c.dtype) for c, p in fwd}, {(k, d) for k in (0, 1, 2) for d in hc.DTYPES},
          "(fwd_kernel, dtype)")
    _need({p["fwd_waves"] for c, p in fwd if p["fwd_kernel"] == 2}, {8, 4}, "fwd_waves on the matrix cores")
    _need({p["fwd_quads"] for c, p in fwd if p["fwd_kernel"] == 2}, {0, 1}, "fwd_quads on the matrix cores")
    assert all(p["fwd_waves"] == 0 and p["fwd_quads"] == 0 for c, p in plans if p["fwd_kernel"] != 2)
    _need({(p["dx_kernel"], c.dtype) for c, p in dx}, {(k, d) for k in (0, 1, 2) for d in hc.DTYPES},
          "(dx_kernel, dtype)")
    # the dlogits load of head_bwd_dw_kernel<T,4> / <T,16>: 16-byte groups only, scalar groups only, both in one launch
    loads = {(p["dw_group"], p["dw_vec_groups"] > 0, p["dw_scalar_groups"] > 0) for c, p in dw if p["dw_group"]}
    _need(loads, {(4, True, False), (4, False, True), (16, True, False), (16, False, True), (16, True, True)},
          "(dw_group, 16-byte groups, scalar groups)")
    # (with four outputs per pass a K that is a multiple of 4 has whole groups only, any other K scalar groups only:
    # no K mixes the two there, and K = 20 is the smallest that does with sixteen)
    from cyhip import ops
    both = {g: [K for K in range(1, 129) if (p := ops.head_plan(306, 8, K))["dw_group"] == g
                and p["dw_vec_groups"] and p["dw_scalar_groups"]] for g in (4, 16)}
    assert both[4] == [] and both[16][0] == 20, both
    assert any(c.K == 20 and p["dw_group"] == 16 for c, p in dw)
    rows = {(p["dw_rows"], c.C) for c, p in dw if p["dw_group"]}
    assert any(r == 256 for r, C in rows), "no case with 256 pixel rows per dW block (C = 8)"
    assert any(r * (C // 8) < 256 for r, C in rows), "no case whose dW block leaves threads idle (C = 40)"
    assert any(1 < r < 256 and C >= 128 for r, C in rows), "no case with 1 < dw_rows < 256 at C >= 128"
    assert any(not c.bias for c in hc.HEAD_CASES) and any(hc.npix(c) < 256 for c, p in dw if p["dw_group"])


def _within_5_percent(n, floor):
    return floor <= n <= floor * 1.05


def test_every_launch_cap_is_passed_by_a_small_case():
    """one case per launch of the cap table with two trips (or more, where one case serves two launches), each within
    5 % of the smallest pixel count that gives two trips of that launch"""
    plans = _plans()

    def some(what, floor, pred):
        hit = [c for c, p in plans if pred(c, p)]
        assert hit, f"no head case sends {what} round its loop a second time"
        assert all(_within_5_percent(hc.npix(c), floor) for c in hit), (what, [hc.case_id(c) for c in hit])
        return hit

    # head_fwd_kernel past 2048 blocks; the same cases run softmax-KL / -MSE on their logits: the backward kernels
    # (2048 blocks) make two trips, the forward kernels (1024 blocks) three
    fwd = some("head_fwd_kernel", 524289, lambda c, p: c.parts == "fwd" and p["fwd_kernel"] < 2 and p["fwd_trips"] >= 2)
    assert {c.K == 4 for c in fwd} == {True, False}, "the losses need a K = 4 (16-byte rows) and a K != 4 case"
    assert all(c.K <= 16 and hc.npix(c) > 2048 * 256 for c in fwd)
    some("head_bwd_dx_kernel", 524289, lambda c, p: c.parts == "dx" and p["dx_kernel"] == 0 and p["dx_trips"] >= 2)
    some("head_bwd_dx_wide_kernel", 524289, lambda c, p: c.parts == "dx" and p["dx_kernel"] == 1 and p["dx_trips"] >= 2)
    dw = some("head_bwd_dw_kernel", 131073, lambda c, p: c.parts == "dw" and p["dw_group"] and p["dw_per"] > 256)
    assert {p["dw_group"] for c in dw for p in [hc.plan(c)]} == {4, 16}
    for c in dw:  # more than one block, the last one short but not empty
        p = hc.plan(c)
        tail = hc.npix(c) - (p["dw_blocks"] - 1) * p["dw_per"]
        assert p["dw_blocks"] > 1 and 0 < tail < p["dw_per"], (hc.case_id(c), p, tail)
    mc = lambda c, p: c.parts == "mc" and p["fwd_kernel"] == 2  # noqa: E731
    some("the matrix-core forward with 8 waves", 65537, lambda c, p: mc(c, p) and p["fwd_waves"] == 8 and p["fwd_trips"] >= 2)
    some("the matrix-core forward with 4 waves", 32769, lambda c, p: mc(c, p) and p["fwd_waves"] == 4 and p["fwd_trips"] >= 2)
    some("the matrix-core backward", 65537, lambda c, p: mc(c, p) and p["dx_trips"] >= 2 and p["dw_per"] >= 256)
    # dice_counts_kernel: 64 blocks per sample
    assert hc.DICE_CASES and all(_within_5_percent(h * w, 64 * 256 + 1) for n, h, w, k in hc.DICE_CASES)
    assert {k == 4 for n, h, w, k in hc.DICE_CASES} == {True, False}


def test_cluster_head_cases_pass_the_caps_at_both_wave_counts():
    from cyhip import ops
    plans = [(c, ops.cluster_head_plan(c.M, c.C, c.S, c.k)) for c in hc.CLUSTER_CASES]
    for waves, floor in ((8, 65537), (4, 32769)):
        hit = [c for c, p in plans if p["fwd_waves"] == waves and p["fwd_trips"] >= 2]
        assert hit and all(_within_5_percent(c.M, floor) for c in hit), (waves, hit)
    hit = [c for c, p in plans if p["bwd_trips"] >= 2]
    assert hit and all(_within_5_percent(c.M, 65537) for c in hit), hit
    assert {c.k % 4 == 0 for c in hit} == {True}  # (the scalar-row form makes its second trip in the forward case)
    assert {c.k % 4 == 0 for c, p in plans if p["fwd_trips"] >= 2} == {True, False}
    assert {c.M for c in hc.CLUSTER_CASES} >= {31, 33}
    for c, p in plans:
        assert p["slabs"] == 4 * p["bwd_grid"] and p["fwd_grid"] <= 256 and p["bwd_grid"] <= 512
        # the workspace query of the launch is the plan's slabs + the 64 staged group sums
        assert ops._lib.load().cy_cluster_head_bwd_ws_bytes(c.M, c.C) == (p["slabs"] + 64) * (128 * c.C + 128) * 4


def test_boundaries_of_the_rule():
    from cyhip import _lib, ops
    a, b = ops.head_plan(306, 32, 16), ops.head_plan(306, 32, 17)
    assert (a["fwd_kernel"], a["dx_kernel"], a["dw_group"]) == (0, 0, 4)
    assert (b["fwd_kernel"], b["dx_kernel"], b["dw_group"]) == (2, 2, 0)
    a, b = ops.head_plan(306, 32, 100), ops.head_plan(306, 96, 100)
    assert (a["fwd_kernel"], a["dx_kernel"], a["dw_group"]) == (2, 2, 0)
    assert (b["fwd_kernel"], b["dx_kernel"], b["dw_group"]) == (1, 1, 16)
    # where eight waves' tiles stop fitting the LDS next to the weights of a 32-channel head: found by query, and the
    # case list holds both sides of it
    waves = [ops.head_plan(306, 32, K)["fwd_waves"] for K in range(17, 129)]
    first4 = 17 + waves.index(4)
    assert waves == [8] * (first4 - 17) + [4] * (129 - first4), waves
    ks = {c.K for c in hc.HEAD_CASES if c.C == 32 and c.parts == "all"}
    assert {first4 - 1, first4} <= ks, (first4, sorted(ks))
    assert all(ops.head_plan(306, 64, K)["fwd_waves"] in (8, 4) for K in range(17, 129))
    # refused: what the launches refuse
    p = _lib.HeadPlan()
    lib = _lib.load()
    for npix, C, K in ((306, 128, 128), (306, 12, 4), (306, 32, 0), (306, 32, 129), (306, 0, 4), (306, 4096, 1)):
        assert lib.cy_head1x1_plan(npix, C, K, 1, 1, p) == -2, (npix, C, K)
        assert lib.cy_head1x1_fwd(None, None, None, None, npix, C, K, 0, None) == -1  # (NULL pointers come first)
    assert lib.cy_head1x1_plan(306, 4096, 1, 1, 0, p) == 0  # (the parameter gradient is what refuses C > 2048)
    assert lib.cy_head1x1_plan(0, 32, 4, 1, 1, p) == -1 and lib.cy_head1x1_plan(306, 32, 4, 1, 1, None) == -1
    with pytest.raises(_lib.HipKernelError):
        ops.head_plan(306, 128, 128)


@pytest.mark.parametrize("case", hc.HEAD_CASES, ids=hc.case_id)
def test_plan_is_consistent_with_the_other_queries(case):
    """what the plan says about grids and workspace, against first principles and the workspace query"""
    from cyhip import ops
    n = hc.npix(case)
    p = hc.plan(case)
    if p["fwd_kernel"] == 2:
        assert case.C in (32, 64) and case.K > 16
        assert p["ws_bytes"] == (4 * p["dw_blocks"] + 64) * (128 * case.C + 128) * 4
        tiles = -(-n // 32)
        assert p["fwd_grid"] == min(256, -(-tiles // p["fwd_waves"])) and p["dx_grid"] == min(512, -(-tiles // 4))
        assert (p["fwd_trips"] - 1) * p["fwd_grid"] * p["fwd_waves"] < tiles <= p["fwd_trips"] * p["fwd_grid"] * p["fwd_waves"]
        assert (p["dx_trips"] - 1) * p["dx_grid"] * 4 < tiles <= p["dx_trips"] * p["dx_grid"] * 4
    else:
        assert p["fwd_kernel"] == (0 if case.K <= 16 else 1) and p["dw_group"] == (4 if case.K <= 16 else 16)
        assert p["ws_bytes"] == p["dw_blocks"] * (case.K * case.C + case.K) * 4
        assert p["dw_vec_groups"] + p["dw_scalar_groups"] == -(-case.K // p["dw_group"])
        assert p["dw_rows"] == 256 // (case.C // 8) and p["dw_blocks"] == min(512, -(-n // 256))
        assert p["dw_per"] == -(-n // p["dw_blocks"])
        work = n * case.C // (32 if p["dx_kernel"] == 1 else 8)
        assert (p["fwd_trips"] - 1) * p["fwd_grid"] * 256 < n <= p["fwd_trips"] * p["fwd_grid"] * 256
        assert (p["dx_trips"] - 1) * p["dx_grid"] * 256 < work <= p["dx_trips"] * p["dx_grid"] * 256
        assert p["dx_kernel"] == (1 if case.K > 16 and case.K % 4 == 0 and case.C % 32 == 0 else 0)
    off = ops.head_plan(n, case.C, case.K, False, False)
    assert off["dx_kernel"] == -1 and off["ws_bytes"] == 0
    assert all(off[f] == 0 for f in ("dx_grid", "dx_trips", "dw_group", "dw_blocks", "dw_rows", "dw_per"))
    assert all(off[f] == p[f] for f in ("fwd_kernel", "fwd_waves", "fwd_quads", "fwd_grid", "fwd_trips"))
