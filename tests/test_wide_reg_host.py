"""Host-side checks of the wide-K regularisers (csrc/cy_wide_reg.hip: entropy, self-MSE, UA-MT and ICT's mix-MSE on
multi-prototype logits, 16 < K <= 64), no GPU: the twelve entries and their launch rule are exported and typed, every
refusal carries its status before any launch, the plan's figures, the coverage of the GPU cases, the dispatch by K in
cyhip.ops, and that the K <= 16 entries answer K = 17 as they did.  No kernel runs here."""
import ctypes as C

import pytest

OK, ARG, SHAPE, WORKSPACE = 0, -1, -2, -5
FAMILIES = ("softmax_entropy", "softmax_selfmse", "uamt_mse", "softmax_mixmse")
CAP, ROWS = 4096, 16
BIG = 1 << 20


@pytest.fixture(scope="module")
def lib():
    from cyhip import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def P():
    """a 16-byte-aligned host address: no launch may ever see it"""
    buf = (C.c_float * 72)()
    p = C.addressof(buf)
    p += (-p) % 16
    P.keep = buf
    return p


# (entry, its arguments with "P" for a pointer, "npix" / "N", "HW" and "K" for the sizes, "ws" for the workspace bytes)
ENTRIES = {
    "cy_softmax_entropy_row_fwd": ("P", "P", "npix", "K", 1e-16, "P", "ws", None),
    "cy_softmax_entropy_row_bwd": ("P", "P", "P", "npix", "K", 1e-16, None),
    "cy_softmax_selfmse_row_fwd": ("P", "P", "npix", "K", "P", "ws", None),
    "cy_softmax_selfmse_row_bwd": ("P", "P", "P", "npix", "K", None),
    "cy_uamt_mse_row_fwd": ("P", "P", "P", "npix", "K", 1.0, 0, "P", "ws", None),
    "cy_uamt_mse_row_bwd": ("P", "P", "P", "P", "P", "npix", "K", 1.0, 0, None),
    "cy_softmax_mixmse_row_fwd": ("P", "P", "P", 0.5, 0.5, "P", "N", "HW", "K", "P", "ws", None),
    "cy_softmax_mixmse_row_bwd": ("P", "P", "P", 0.5, 0.5, "P", "P", "N", "HW", "K", None),
}


def call(lib, P, name, npix=286, K=20, ws=BIG, null=None, odd=None):
    """the entry with host pointers; `null`: which pointer (in order) is NULL; `odd`: which one is 2 bytes off"""
    args, seen = [], 0
    for a in ENTRIES[name]:
        if a == "P":
            args.append(None if seen == null else P + 2 if seen == odd else P)
            seen += 1
        elif a == "npix":
            args.append(npix)
        elif a == "N":
            args.append(2 if npix % 2 == 0 and npix > 0 else 1 if npix > 0 else npix)
        elif a == "HW":
            args.append(npix // 2 if npix % 2 == 0 and npix > 0 else npix if npix > 0 else 10)
        else:
            args.append({"K": K, "ws": ws}.get(a, a) if isinstance(a, str) else a)
    return getattr(lib, name)(*args)


def pointers(name):
    return sum(a == "P" for a in ENTRIES[name])


# ---- 1. exports -------------------------------------------------------------------------------------------------------
def test_the_twelve_entries_and_the_plan_are_exported_and_typed(lib):
    from cyhip import _lib
    sigs = _lib._SIGS
    for fam in FAMILIES:
        for suffix in ("ws_bytes", "fwd", "bwd"):
            new, old = f"cy_{fam}_row_{suffix}", f"cy_{fam}_{suffix}"
            assert hasattr(lib, new) and new in _lib.exported_names(), new
            assert sigs[new] == sigs[old], new  # the arguments of the K <= 16 counterpart
            assert getattr(lib, new).argtypes == sigs[new][1]
        assert sigs[f"cy_{fam}_row_ws_bytes"][0] is C.c_size_t and sigs[f"cy_{fam}_row_fwd"][0] is C.c_int
    assert sigs["cy_wide_reg_plan"] == (C.c_int, [C.c_int, C.c_long, C.c_int, C.c_int, C.POINTER(_lib.WideRegPlan)])
    assert [_lib.CY_WIDE_ENTROPY, _lib.CY_WIDE_SELFMSE, _lib.CY_WIDE_UAMT, _lib.CY_WIDE_MIXMSE] == [0, 1, 2, 3]
    assert lib.cy_abi_version() == _lib.ABI_VERSION == 19
    assert len(_lib._STRUCTS) == 27 and _lib._STRUCTS["cy_wide_reg_plan_t"] is _lib.WideRegPlan  # a header struct


# ---- 2. refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_every_refusal_carries_its_status_before_any_launch(lib, P, name):
    for K in (1, 16, 65, 0, -4):
        assert call(lib, P, name, K=K) == SHAPE, K
    for i in range(pointers(name)):
        assert call(lib, P, name, null=i) == ARG, i
    for npix in (0, -1):
        assert call(lib, P, name, npix=npix) == ARG, npix
    for i in LOGIT_ROWS[name]:  # a base of logits or of their gradient that is not a float's alignment
        assert call(lib, P, name, odd=i) == ARG, i


# which pointers (in order) are [npix][K] rows; the others are scalars, the index or the workspace
LOGIT_ROWS = {"cy_softmax_entropy_row_fwd": (0,), "cy_softmax_entropy_row_bwd": (0, 2),
              "cy_softmax_selfmse_row_fwd": (0,), "cy_softmax_selfmse_row_bwd": (0, 2),
              "cy_uamt_mse_row_fwd": (0, 1), "cy_uamt_mse_row_bwd": (0, 1, 4),
              "cy_softmax_mixmse_row_fwd": (0, 1), "cy_softmax_mixmse_row_bwd": (0, 1, 4)}


@pytest.mark.parametrize("fam", FAMILIES)
def test_a_short_workspace_is_refused(lib, P, fam):
    per = 16 if fam == "uamt_mse" else 8
    query = getattr(lib, f"cy_{fam}_row_ws_bytes")
    for npix in (2, 286, CAP * ROWS, CAP * ROWS + 2, 16 * 224 * 224):
        need = query(2, npix // 2) if fam == "softmax_mixmse" else query(npix)
        assert need == per * min(CAP, -(-npix // ROWS)), (npix, need)
        assert call(lib, P, f"cy_{fam}_row_fwd", npix=npix, ws=need - 1) == WORKSPACE
    if fam == "softmax_mixmse":
        assert query(0, 10) == 0 and query(2, 0) == 0
    else:
        assert query(0) == 0 and query(-1) == 0


def test_the_plan_refuses_with_the_status_of_the_launches(lib):
    from cyhip import _lib
    plan = _lib.WideRegPlan()
    assert lib.cy_wide_reg_plan(0, 286, 20, 16, None) == ARG
    assert lib.cy_wide_reg_plan(4, 286, 20, 16, plan) == ARG and lib.cy_wide_reg_plan(-1, 286, 20, 16, plan) == ARG
    for fam in range(4):
        assert lib.cy_wide_reg_plan(fam, 0, 20, 16, plan) == ARG and lib.cy_wide_reg_plan(fam, -1, 20, 16, plan) == ARG
        for align in (0, 1, 2, 6):
            assert lib.cy_wide_reg_plan(fam, 286, 20, align, plan) == ARG, align
        for K in (1, 16, 65):
            assert lib.cy_wide_reg_plan(fam, 286, K, 16, plan) == SHAPE, K
        for K in (17, 64):
            assert lib.cy_wide_reg_plan(fam, 286, K, 16, plan) == OK, K


def test_the_wrapper_raises_on_a_refused_plan():
    from cyhip import _lib, ops
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_SHAPE"):
        ops.wide_reg_plan("entropy", 286, 16)
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_ARG"):
        ops.wide_reg_plan("uamt", 0, 20)


# ---- 3. the plan's figures ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["entropy", "selfmse", "uamt", "mixmse"])
def test_plan_figures(family):
    from cyhip import ops
    for K in (17, 20, 40, 63, 64):
        for align in (4, 8, 16, 32):
            p = ops.wide_reg_plan(family, 286, K, align)
            assert p["vec"] == (4 if K % 4 == 0 and align % 16 == 0 else 1), (K, align, p)
            assert p["rows_per_block"] == ROWS
    want = {1: (1, 1), 15: (1, 1), 16: (1, 1), 17: (2, 1), 286: (18, 1), CAP * ROWS: (CAP, 1), CAP * ROWS + 1: (CAP, 2),
            16 * 224 * 224: (CAP, 13)}
    for npix, (grid, trips) in want.items():
        p = ops.wide_reg_plan(family, npix, 20)
        assert (p["fwd_grid"], p["fwd_trips"], p["bwd_grid"], p["bwd_trips"]) == (grid, trips, grid, trips), (npix, p)
        assert p["fwd_grid"] * p["fwd_trips"] * ROWS >= npix  # every pixel has a row
    assert ops.wide_reg_plan(family, 1 << 40, 20)["fwd_trips"] == (1 << 40) // (CAP * ROWS)


def test_the_gpu_cases_reach_every_form_of_the_launch_rule():
    """tests/test_gpu_wide_reg.py: the fixture's K and shape, the second-trip size, the guarded slices"""
    from cyhip import ops
    import semi_wide_fixture as fx
    npix = fx.SHAPE[0] * fx.SHAPE[1] * fx.SHAPE[2]
    assert npix == 286 and npix % ROWS == 14  # a partial group
    plans = [ops.wide_reg_plan("entropy", npix, K) for K in fx.KS]
    assert {p["vec"] for p in plans} == {1, 4}
    assert [p["vec"] for p in plans] == [1, 4, 4, 1, 4]  # 17, 20, 40, 63, 64
    sliced = ops.wide_reg_plan("entropy", npix, 20, align=4)  # a base one float into a buffer
    assert sliced["vec"] == 1
    one = ops.wide_reg_plan("entropy", 1, 20, align=4)
    assert (one["fwd_grid"], one["fwd_trips"]) == (1, 1)
    first = ops.wide_reg_plan("entropy", npix, 20)
    second = first["rows_per_block"] * CAP + 1
    assert second == 65537
    p = ops.wide_reg_plan("entropy", second, 20)
    assert p["fwd_trips"] == 2 and p["bwd_trips"] == 2 and p["fwd_grid"] == CAP


# ---- 4. the dispatch by K and the old entries ----------------------------------------------------------------------------
def test_ops_choose_the_entry_by_k():
    from cyhip import ops
    for K in (2, 4, 16, 1, 0, 65, 100):
        assert ops._by_k("softmax_entropy", K) == "cy_softmax_entropy", K  # (and their refusals stay what they were)
    for K in (17, 20, 63, 64):
        assert ops._by_k("uamt_mse", K) == "cy_uamt_mse_row", K


def test_the_old_entries_still_answer_k_17_as_they_did(lib, P):
    assert lib.cy_softmax_entropy_fwd(P, P, 286, 17, 1e-16, P, BIG, None) == ARG
    assert lib.cy_softmax_entropy_bwd(P, P, P, 286, 17, 1e-16, None) == ARG
    assert lib.cy_softmax_selfmse_fwd(P, P, 286, 17, P, BIG, None) == ARG
    assert lib.cy_softmax_selfmse_bwd(P, P, P, 286, 17, None) == ARG
    assert lib.cy_uamt_mse_fwd(P, P, P, 286, 17, 1.0, 0, P, BIG, None) == ARG
    assert lib.cy_uamt_mse_bwd(P, P, P, P, P, 286, 17, 1.0, 0, None) == ARG
    assert lib.cy_softmax_mixmse_fwd(P, P, P, 0.5, 0.5, P, 2, 143, 17, P, BIG, None) == SHAPE
    assert lib.cy_softmax_mixmse_bwd(P, P, P, 0.5, 0.5, P, P, 2, 143, 17, None) == SHAPE
    from cyhip import _lib
    plan = _lib.MixPlan()
    assert lib.cy_mix_plan(2, 2, 143, 17, 16, plan) == SHAPE
    for npix in (286, 16 * 224 * 224):  # and their workspace is what it was: a partial per block of 256 pixels
        blocks = min(max((npix + 255) // 256, 1), 1024)
        assert lib.cy_softmax_entropy_ws_bytes(npix) == blocks * 8 and lib.cy_uamt_mse_ws_bytes(npix) == blocks * 16
