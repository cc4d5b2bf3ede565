"""tests/test_gpu_norm_act_dispatch.py claims to reach every host-side branch and every capped loop of
csrc/cy_norm_act.hip.  Which branch a launch takes is decided by one host-side function, cy_norm_act_plan, so the claim
is checked here on the CPU, against the same case lists the GPU tests are parametrised with (tests/norm_act_cases.py).
Where one case alone reaches a feature, the assertion message names the feature: dropping that case fails here, by name,
without a GPU."""
import pytest

from tests import norm_act_cases as nc

KERNELS = {0: "apply", 1: "apply fold", 2: "apply_pool", 3: "apply_pool fold", 4: "bwd_reduce deep", 5: "bwd_reduce",
           6: "bwd_apply", 7: "bwd_apply fold", 8: "pool_bwd", 9: "pool_bwd stats", 10: "up_bwd", 11: "up_bwd stats",
           12: "finalize", 13: "bwd_finalize", 14: "fold_coef"}
CODE = {"f32": 0, "bf16": 1, "f16": 2}


def reduce_plans():
    return [(c, nc.reduce_plan(c)) for c in nc.REDUCE_CASES]


def launch_plans():
    """(what, plan) of every launch the GPU file makes"""
    out = [(nc.case_id(c), p) for c, p in reduce_plans()]
    for c in nc.EW_CASES:
        for kind, N, H, W, fold in nc.ew_kinds(c):
            out.append((f"{nc.case_id(c)}:{kind}", nc.plan(kind, N, H, W, c.C, c.dtype, fold)))
        if c.mixed:
            out.append((f"{nc.case_id(c)}:apply->f32", nc.plan("apply", c.N, c.H, c.W, c.C, c.dtype, 0, "f32")))
            out.append((f"{nc.case_id(c)}:apply fold->f32", nc.plan("apply", c.N, c.H, c.W, c.C, c.dtype, 2, "f32")))
    for b in nc.BIG_CASES:
        for kind in b.kinds:
            out.append((f"{b.name}:{kind}", nc.plan(kind, b.N, b.H, b.W, b.C, "bf16", b.fold)))
    N, H, W, C = nc.FOLD_GEOM
    for R in nc.FOLD_RS:
        for kind in nc.FOLD_KINDS:
            n, h, w = (1, 1, 1) if kind == "fold_coef" else (N, H // 2, W // 2) if kind == "apply_pool" else (N, H, W)
            out.append((f"R{R}:{kind}", nc.plan(kind, n, h, w, C, "f32", R)))
    for P in nc.FINALIZE_P:
        out.append((f"finalize P{P}", nc.plan("finalize", P, 1, 1, nc.FINALIZE_C, "f32")))
    for P in nc.BWD_FINALIZE_P:
        out.append((f"bwd_finalize P{P}", nc.plan("bwd_finalize", P, 1, 1, nc.BWD_FINALIZE_C, "f32")))
    return out


def test_every_kernel_variant_and_type_pair_is_launched():
    plans = launch_plans()
    ok = [(w, p) for w, p in plans if p["status"] == 0]
    assert {p["kernel"] for _, p in ok} == set(KERNELS), sorted(set(KERNELS) - {p["kernel"] for _, p in ok})
    pairs = {(p["kernel"], p["type_in"], p["type_out"]) for _, p in ok}
    same = [(t, t) for t in CODE.values()]
    mixed = [(CODE["bf16"], CODE["f32"]), (CODE["f16"], CODE["f32"])]
    for k in range(12):  # the kernels that are templates on the storage type
        for ti, to in same + (mixed if k in (0, 1) else []):
            assert (k, ti, to) in pairs, f"no case runs {KERNELS[k]} on types {ti} -> {to}"
    # the type pairs that have no kernel are refused, by the plan as by the launch
    assert nc.plan("apply", 1, 2, 2, 8, "f32", 0, "bf16")["status"] == -3
    assert nc.plan("apply_pool", 1, 2, 2, 8, "bf16", 0, "f32")["status"] == -3


def test_reduce_cases_reach_both_forms_and_every_loop():
    plans = reduce_plans()
    deep = [p for _, p in plans if p["deep"]]
    shallow = [p for _, p in plans if not p["deep"]]
    assert any(p["round4"] and p["tail1"] for p in deep), "deep form: no case runs the 4-pixel round and the 1-pixel tail"
    assert any(p["round4"] and p["tail1"] and p["grid"] > 1 and p["pages"] == 2 for p in deep), \
        "deep form, two pages, several workgroups"
    assert any(not p["round4"] and p["tail1"] for p in deep), "deep form with the 1-pixel loop alone"
    assert shallow and all(p["tail1"] and not p["round4"] and p["kernel"] == 5 for p in shallow), "non-deep form"
    assert any(p["idle_rows"] > 0 for p in deep) and any(p["idle_rows"] > 0 for p in shallow), "idle pixel rows"
    assert any(p["idle_threads"] == 1 and p["grid"] == 1 for p in deep), "idle thread 255 (C = 40), one workgroup"
    assert any(p["idle_threads"] == 1 and p["empty_workgroups"] for p in deep), "idle thread with empty workgroups"
    assert any(p["pages"] == 2 and p["last_page_groups"] == 1 for p in deep), "a second page of one channel group"
    assert any(p["rows"] == 1 and p["pages"] == 1 and p["groups_per_page"] == 256 for p in deep), "C = 2048: one row"
    assert {p["rows"] for _, p in plans} >= {256, 51, 32, 4, 1}
    for dt in nc.TYPES:
        assert any(c.dtype == dt and p["deep"] for c, p in plans), f"deep form in {dt}"
        assert any(c.dtype == dt and not p["deep"] for c, p in plans), f"non-deep form in {dt}"
        assert any(c.dtype == dt and p["empty_workgroups"] for c, p in plans), f"empty workgroups in {dt}"


def test_reduce_cases_sit_on_both_sides_of_each_boundary():
    by_n = {}
    for c, p in reduce_plans():
        by_n.setdefault(c.npix, p)
    for n in nc.REDUCE_PIXELS:
        assert n in by_n, f"no reduce case with {n} pixels"
    g = lambda n, f="grid": by_n[n][f]  # noqa: E731
    assert g(nc.ONE_WG) == 1
    # 32-pixel workgroups | the 511-workgroup plateau
    assert g(nc.LAST_32) == 511 and g(nc.LAST_32, "pixels_per_workgroup") == 32 and g(nc.LAST_32, "empty_workgroups") == 0
    assert g(nc.FIRST_511) == 511 and g(nc.FIRST_511, "pixels_per_workgroup") == 33
    assert g(nc.FIRST_511, "empty_workgroups") == 15, "first count on the plateau: 15 empty workgroups"
    # plateau (deep) | 128-pixel workgroups (non-deep)
    assert g(nc.LAST_511) == 511 and g(nc.LAST_511, "deep") == 1 and g(nc.LAST_511, "pixels_per_workgroup") == 128
    assert g(nc.FIRST_SHALLOW) == 512 and g(nc.FIRST_SHALLOW, "deep") == 0
    # 128-pixel workgroups | the cap of 1024
    assert g(nc.LAST_UNCAPPED) == 1024 and g(nc.LAST_UNCAPPED, "pixels_per_workgroup") == 128
    assert g(nc.LAST_UNCAPPED, "empty_workgroups") == 0
    assert g(nc.PAST_CAP) == 1024 and g(nc.PAST_CAP, "pixels_per_workgroup") == 129
    assert g(nc.PAST_CAP, "empty_workgroups") == 7, "past the cap: 7 empty workgroups"
    # the boundaries are where the table says: one pixel less or more changes nothing else
    assert nc.plan("bwd_reduce", 1, 1, nc.LAST_32 - 32, 8)["grid"] == 510
    assert nc.plan("bwd_reduce", 1, 1, nc.PAST_CAP + 1000, 8)["grid"] == 1024


def test_every_capped_loop_makes_a_second_trip_close_to_the_floor():
    seen = set()
    for b in nc.BIG_CASES:
        for kind in b.kinds:
            p = nc.plan(kind, b.N, b.H, b.W, b.C, "bf16", b.fold)
            what = f"{b.name}:{kind}"
            assert p["status"] == 0 and p["trips"] == 2, what
            floor = p["one_trip_items"] + 1
            assert floor <= p["items"] <= 1.05 * floor, (what, p["items"], floor)
            seen.add(p["kernel"])
            if b.name == "plain-c40-not-pow2":
                assert p["pow2"] == 0, "backward apply past the cap with a group count that is no power of two"
            if kind == "bwd_apply" and b.name == "plain-c512":
                assert p["pow2"] == 1
    assert any(nc.plan("bwd_apply", b.N, b.H, b.W, b.C, "bf16", 0)["pow2"] == 0 for b in nc.BIG_CASES
               if "bwd_apply" in b.kinds and not b.fold), "backward apply past the cap without the power-of-two switch"
    # every kernel with a capped grid-stride loop (the reduce has none: its workgroups take what is left)
    for k in (0, 1, 2, 3, 6, 7, 8, 9, 10, 11):
        assert k in seen, f"no case makes a second trip in {KERNELS[k]}"
    # both caps of the pooled apply, as the plan has them
    assert nc.plan("apply_pool", 1, 181, 182, 512)["one_trip_items"] == 8192 * 256
    assert nc.plan("apply_pool", 1, 45, 46, 1024, "bf16", 2)["one_trip_items"] == 256 * 1024
    # ... and no other case is big: everything else has one trip and about a million elements at the most
    for c in nc.EW_CASES:
        assert c.N * c.H * c.W * c.C < 10 ** 6
        for kind, N, H, W, fold in nc.ew_kinds(c):
            if kind != "bwd_reduce":
                assert nc.plan(kind, N, H, W, c.C, c.dtype, fold)["trips"] == 1
    # the reduce's three largest pixel counts are set by its boundaries; they stay at C <= 64 (1.05 M elements at C = 8,
    # 4.2 M and 8.4 M at C = 64); every other reduce case is under a million elements
    forced = (nc.FIRST_SHALLOW, nc.LAST_UNCAPPED, nc.PAST_CAP)
    assert all(c.npix * c.C < 10 ** 6 or (c.npix in forced and c.C <= 64) for c in nc.REDUCE_CASES)


def test_fused_forms_applicable_and_refused():
    for kind in ("pool_bwd_bn", "up_bwd_bn"):
        yes = [c for c in nc.EW_CASES if nc.plan(kind, c.N, c.H // 2, c.W // 2, c.C, c.dtype, 1)["fused_ok"]]
        no = [c for c in nc.EW_CASES if not nc.plan(kind, c.N, c.H // 2, c.W // 2, c.C, c.dtype, 1)["fused_ok"]]
        assert {c.C for c in yes} == {8, 1024}, f"{kind}: fused form on one lane per group and on 128 groups"
        assert {c.C for c in no} == set(nc.FUSED_REFUSED_C), f"{kind}: C/8 = 3 and 5 must be refused"
        for c in no:
            p = nc.plan(kind, c.N, c.H // 2, c.W // 2, c.C, c.dtype, 1)
            assert p["status"] == -2 and p["kernel"] in (8, 10) and p["partial_rows"] == 0, "refused: the unfused kernel"
        for dt in nc.TYPES:
            assert any(c.dtype == dt for c in yes) and any(c.dtype == dt for c in no), (kind, dt)
    from cyhip import _lib
    lib = _lib.load()
    for c in nc.EW_CASES:
        want = nc.plan("pool_bwd_bn", c.N, c.H // 2, c.W // 2, c.C)
        got = lib.cy_maxpool2_bwd_bn_num_partials(c.N, c.H // 2, c.W // 2, c.C)
        assert got == (want["grid"] if want["fused_ok"] else -2)
        assert lib.cy_upsample2_bwd_bn_workgroups(c.N, c.H // 2, c.W // 2, c.C) == got


def test_every_gather_path_by_replica_count():
    N, H, W, C = nc.FOLD_GEOM
    for R, code, path in ((1, 1, "direct 1"), (2, 1, "direct 2"), (4, 1, "direct 4"), (8, 1, "direct 8"),
                          (16, 2, "wide 16"), (32, 2, "wide 32"), (64, 3, "LDS atomics")):
        assert R in nc.FOLD_RS, f"gather path {path}: no case with R = {R}"
        assert nc.plan("apply", N, H, W, C, "f32", R)["gather"] == code, f"gather path {path}"
    wide = {R: nc.plan("apply", N, H, W, C, "f32", R)["gather"] for R in nc.FOLD_RS}
    assert wide == {1: 1, 2: 1, 4: 1, 8: 1, 16: 2, 32: 2, 64: 3}, wide
    for kind in ("apply_pool", "bwd_apply"):
        assert {R: nc.plan(kind, N, H // 2, W // 2, C, "f32", R)["gather"] for R in nc.FOLD_RS} == wide
    narrow = {R: nc.plan("fold_coef", 1, 1, 1, C, "f32", R)["gather"] for R in nc.FOLD_RS}
    assert narrow == {1: 1, 2: 1, 4: 1, 8: 1, 16: 3, 32: 3, 64: 3}, narrow
    # the consumers are checked on more than the leader workgroup
    assert nc.plan("apply", N, H, W, C, "f32", 4)["grid"] == 3 and nc.plan("bwd_apply", N, H, W, C, "f32", 4)["grid"] == 3
    assert nc.plan("apply_pool", N, H // 2, W // 2, C, "f32", 4)["grid"] == 3
    # the fold forms' limit, and one channel more than a fold may have
    assert any(c.C == 1024 for c in nc.EW_CASES)
    assert nc.plan("apply", 1, 2, 2, 1024, "bf16", 2)["status"] == 0 and nc.plan("apply", 1, 2, 2, 1032, "bf16", 2)["status"] == -2
    assert nc.plan("fold_coef", 1, 1, 1, 2048, "f32", 1)["status"] == 0 and nc.plan("fold_coef", 1, 1, 1, 2049, "f32", 1)["status"] == -2


def test_finalize_cases_cross_the_stride():
    f = {P: nc.plan("finalize", P, 1, 1, nc.FINALIZE_C, "f32") for P in nc.FINALIZE_P}
    assert [f[P]["trips"] for P in (1, 256, 257)] == [1, 1, 2], "forward finalize: a second round of 256 partial rows"
    assert f[1]["grid"] == 3 and f[1]["idle_threads"] == 2 * 256, "forward finalize: a half-empty last workgroup"
    b = {P: nc.plan("bwd_finalize", P, 1, 1, nc.BWD_FINALIZE_C, "f32") for P in nc.BWD_FINALIZE_P}
    assert [b[P]["trips"] for P in (1, 64, 65, 1024)] == [1, 1, 2, 16], "backward finalize: rounds of 64 partial rows"
    assert nc.RUNNING_LAYERS > 32 and nc.RUNNING_C > 256


def test_queries_and_plan_agree():
    """the count queries the Python side sizes its buffers with are the plan's numbers"""
    from cyhip import _lib
    lib = _lib.load()
    for n in list(nc.REDUCE_PIXELS) + [1, 32, 33, 511 * 32 + 1, 10 ** 7]:
        p = nc.plan("bwd_reduce", 1, 1, n, 64)
        assert lib.cy_bn_bwd_num_partials(n, 64) == p["grid"] == p["partial_rows"] == lib.cy_bn_relu_bwd_workgroups(n, 64)
        assert p["deep"] == (p["grid"] < 512)
        assert p["chain"] == p["trips"] + p["rows"] - p["idle_rows"]
    with pytest.raises(_lib.HipKernelError):
        nc.plan("apply", 0, 1, 1, 8)
    with pytest.raises(_lib.HipKernelError):
        nc.plan("apply", 1, 1, 1, 8, "bf16", 3)  # replicas are a power of two
    with pytest.raises(_lib.HipKernelError):
        nc.plan("fold_coef", 1, 1, 1, 8, "f32", 0)


def test_launches_answer_what_the_plan_answers():
    """the status the plan reports for a refused shape or type is what the launch returns, before anything is launched
    (host buffers: a launch would fault).  dtype 7 is no type; 17 would read as bf16 if only its low bits were looked at"""
    import ctypes as C
    from cyhip import _lib
    lib = _lib.load()
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    acc = _lib.BnAcc(p, 2, 8)

    def status(kind, N, H, W, Cc, dtype, fold=0):
        pl = _lib.NormActPlan()
        assert lib.cy_norm_act_plan(_lib.NORM_ACT_KINDS.index(kind), N, H, W, Cc, dtype, fold, C.byref(pl)) == 0
        return pl.status
    F32, BF16 = _lib.CY_F32, _lib.CY_BF16
    out = lambda t: (t + 1) << 4  # noqa: E731
    for Cc, ti, to, want in ((12, BF16, BF16, -2), (8, F32, BF16, -3), (8, 7, 7, -3), (8, 17, 17, -3), (8, BF16, 7, -3)):
        assert lib.cy_bn_relu_apply(p, p, p, p, 4, Cc, ti, to, None) == want, (Cc, ti, to)
        if max(ti, to) < 15:
            assert status("apply", 1, 2, 2, Cc, ti | out(to)) == want, (Cc, ti, to)
    assert lib.cy_bn_relu_apply_pool(p, p, p, p, p, 1, 1, 1, 8, BF16, F32, None) == -3 == status("apply_pool", 1, 1, 1, 8, BF16 | out(F32))
    f = _lib.BnFold(p, 2, 1032, None, None, 4.0, 1e-5, 0, p)
    assert lib.cy_bn_relu_apply_fold(p, C.byref(f), p, 4, BF16, BF16, None) == -2 == status("apply", 1, 2, 2, 1032, BF16, 2)
    for dt in (7, 17):
        want = status("bwd_reduce", 1, 2, 2, 8, dt) if dt < 15 else -3
        assert want == -3
        assert lib.cy_bn_relu_bwd_reduce(p, 8, p, p, p, p, p, p, 4, 8, dt, None) == want
        assert lib.cy_bn_relu_bwd_reduce_acc(p, 8, p, p, C.byref(acc), 4, 8, dt, None) == want
        assert lib.cy_bn_relu_bwd_apply(p, 8, p, p, p, p, p, 4, 8, dt, None) == want
        assert lib.cy_bn_relu_bwd_apply_fold(p, 8, p, p, C.byref(acc), 4.0, 1, None, None, 0, p, 4, 8, dt, None) == want
        assert lib.cy_maxpool2_bwd(p, p, None, 8, p, 1, 1, 1, 8, dt, None) == want
        assert lib.cy_maxpool2_bwd_bn(p, p, None, 8, p, p, p, p, p, p, p, 1, 1, 1, 8, dt, None) == want
        assert lib.cy_upsample2_bwd(p, 8, p, 1, 1, 1, 8, dt, None) == want
        assert lib.cy_upsample2_bwd_bn_acc(p, 8, p, p, p, C.byref(acc), 1, 1, 1, 8, dt, None) == want
    acc24 = _lib.BnAcc(p, 1, 24)
    assert status("pool_bwd_bn", 1, 1, 1, 24, BF16, 1) == -2 == status("up_bwd_bn", 1, 1, 1, 24, BF16, 1)
    assert lib.cy_maxpool2_bwd_bn(p, p, None, 24, p, p, p, p, p, p, p, 1, 1, 1, 24, BF16, None) == -2
    assert lib.cy_upsample2_bwd_bn_acc(p, 24, p, p, p, C.byref(acc24), 1, 1, 1, 24, BF16, None) == -2
    f = _lib.BnFold(p, 1, 2056, None, None, 4.0, 1e-5, 0, p)
    assert lib.cy_bn_fold_coef(C.byref(f), None) == -2 == status("fold_coef", 1, 1, 1, 2056, F32, 1)
