"""tests/test_gpu_unet2_dispatch.py claims to reach every host-side branch and every capped loop of csrc/cy_groupnorm.hip
and csrc/cy_unet2.hip.  The claim is checked here on the CPU, against the same tables (tests/unet2_cases.py).  Slice
counts come from the library's own workspace queries and glue._auto_ksplit; the geometry the library does not export is
restated in the case module next to its source line.  Each assertion names its branch: deleting a case fails here, by
name, without a GPU.  The rejections of these entry points are asserted here too: a refused call launches nothing, so
host buffers do."""
import ctypes as C

import pytest

from tests import unet2_cases as uc


@pytest.fixture(scope="module")
def lib():
    from cyhip import _lib
    return _lib.load()


# ---------------------------------------------------------------- slice counts, read from the library
def colsum_slices(lib, M):
    return lib.cy_colsum_ws_bytes(M, 1) // 4


def ln_slices(lib, M):
    return (lib.cy_chan_layernorm_bwd_ws_bytes(M, 1) // 4 - 2 * M) // 2


def col_slices(lib, n):
    return (lib.cy_col_softmax_ws_bytes(1, n, 1) // 4 - 2) // 2


def empty_slices(total, S):
    per = -(-total // S)
    return sum(1 for s in range(S) if s * per >= total)


def test_row_slices_reach_one_middle_and_the_cap_with_an_empty_slice(lib):
    assert set(uc.ROWS_M) == {c.M for c in uc.ROWS_CASES}, "every M of the issue has a case"
    assert set(uc.ROWS_N) == {c.N for c in uc.ROWS_CASES}, "every N / C of the issue has a case"
    S = {M: colsum_slices(lib, M) for M in uc.ROWS_M}
    assert S == {M: ln_slices(lib, M) for M in uc.ROWS_M}, "colsum and LayerNorm share slices_for"
    assert S[1] == 1 and S[256] == 1, "S = 1"
    assert S[257] == 2, "1 < S < cap"
    assert S[131072] == uc.SLICE_CAP and empty_slices(131072, S[131072]) == 0, "S = cap, every slice full (256 rows)"
    assert S[131073] == uc.SLICE_CAP and -(-131073 // S[131073]) == 257, "S = cap with rows_per > 256"
    assert empty_slices(131073, S[131073]) >= 1, "S = cap with an empty last slice"
    assert colsum_slices(lib, 10 ** 7) == uc.SLICE_CAP
    assert any(c.N > 256 and colsum_slices(lib, c.M) > 1 for c in uc.ROWS_CASES), "two column blocks with several slices"
    assert any(c.N == 1 and c.M >= uc.LONG_M for c in uc.ROWS_CASES), "LayerNorm with one channel past the cap"
    assert uc.LONG_M == 131073


def test_col_softmax_slices_reach_one_middle_and_the_cap_with_an_empty_slice(lib):
    assert set(uc.COL_N) == {c.n for c in uc.COL_CASES}, "every n of the issue has a case"
    S = {n: col_slices(lib, n) for n in uc.COL_N}
    assert S[1] == 1 and S[128] == 1, "S = 1"
    assert S[129] == 2, "1 < S < cap"
    assert S[32768] == uc.COL_SLICE_CAP and empty_slices(32768, S[32768]) == 0, "S = cap, every slice full"
    assert S[32769] == uc.COL_SLICE_CAP and empty_slices(32769, S[32769]) == 1, \
        "S = cap with an empty last slice (the o[1] > 0 guard of col_softmax_final_kernel)"
    assert any(c.Ch > 256 and col_slices(lib, c.n) > 1 for c in uc.COL_CASES), "Ch = 257: two channel blocks, two slices"
    assert any(c.B == 3 for c in uc.COL_CASES) and any(c.off > 0 and c.ld > c.off + c.Ch for c in uc.COL_CASES)
    # the workspace query is what the cases are sized with: B slabs of S x Ch pairs and B x Ch final pairs
    for c in uc.COL_CASES:
        assert lib.cy_col_softmax_ws_bytes(c.B, c.n, c.Ch) == (c.B * col_slices(lib, c.n) * c.Ch * 2 + c.B * c.Ch * 2) * 4
    p = uc.LINATTN_LONG
    assert p["H"] * p["W"] > 32768 and col_slices(lib, p["H"] * p["W"]) == uc.COL_SLICE_CAP, "LinearAttentionFn past the cap"
    assert set(uc.ROW_N) >= {1, 255, 256, 257, 784, 1000}, "row_softmax: below, at and past one trip of 256, 784, 1000"
    assert uc.ATTN_784["H"] * uc.ATTN_784["W"] == 784


def test_gemm_variants_splits_and_k_ranges(lib):
    from cyhip import glue
    for v, want in uc.GEMM_VARIANTS.items():
        for M, N, K in uc.GEMM_SIZES + (uc.GEMM_LONG,):
            la, lb, _, _ = uc.gemm_layouts(v, M, N, K)
            assert uc.gemm_loader(la, lb) == want, f"loader variant {v} at {M}x{N}x{K}"
    assert set(uc.GEMM_VARIANTS.values()) == {(a, b) for a in (True, False) for b in (True, False)}, "all four loaders"
    assert (65, 63, 17) in uc.GEMM_SIZES and (64, 64, 16) in uc.GEMM_SIZES and (1, 1, 3) in uc.GEMM_SIZES
    assert any(K < uc.GEMM_KSTEP for _, _, K in uc.GEMM_SIZES), "K < 16"
    M, N, K = uc.GEMM_LONG
    ks = glue._auto_ksplit(M, N, K, 1)
    assert K >= 2048 and ks > 1, "automatic split-K above 1"
    assert all(glue._auto_ksplit(m, n, k, 1) == 1 for m, n, k in uc.GEMM_SIZES)
    assert lib.cy_gemm_strided_ws_bytes(M, N, 1, ks) == ks * M * N * 4 and lib.cy_gemm_strided_ws_bytes(M, N, 1, 1) == 0
    ranges = {c.name: uc.gemm_kranges(c.K, c.ksplit) for c in uc.GEMM_SPLITS}
    assert ranges["last-split-one-element"][-1] == (32, 33), "split-K: last split of one element"
    assert ranges["last-split-empty"][-1] == (32, 32), "split-K: empty last split"
    p = uc.GEMM_COMBINED
    r = uc.gemm_kranges(p["K"], p["ksplit"])
    assert p["nb1"] * p["nb2"] == 6 and p["alpha"] != 1 and 0 < r[-1][1] - r[-1][0] < uc.GEMM_KSTEP, \
        "split-K with bias, alpha, accumulate and 3 x 2 batches, partial last split"
    p = uc.LINATTN_LONG
    assert glue._auto_ksplit(p["dh"], p["dh"], p["H"] * p["W"], p["N"] * p["heads"]) == 64, "context GEMM: 64 splits"


def test_groupnorm_reduction_geometry():
    geo = {c.name: uc.gn_geometry(c.C, c.HW) for c in uc.GN_SHAPES}
    assert {g["rows"] for g in geo.values()} >= {1, 32, 51, 85, 256}, "rows in {1, 32, 51, 85, 256}"
    assert geo["three-groups-idle-thread"]["idle_threads"] == 1 and geo["three-groups-idle-thread"]["rows"] == 85, \
        "a channel-group count that does not divide 256: thread 255 idle"
    assert geo["round-then-tail"]["rows"] == 51 and geo["round-then-tail"]["per"] == 206 and geo["round-then-tail"]["both"], \
        "4-pixel round, then the tail"
    assert geo["round-only"]["round"] and not geo["round-only"]["tail"] and geo["round-only"]["rows"] == 32, "round only"
    assert geo["tail-only"]["tail"] and not geo["tail-only"]["round"] and geo["tail-only"]["rows"] == 32, "tail only"
    assert geo["host-limits"]["rows"] == 1 and geo["host-limits"]["both"], "C = 2048: one pixel row, round and tail"
    hl = next(c for c in uc.GN_SHAPES if c.name == "host-limits")
    assert hl.C == 2048 and hl.C // hl.G == 256, "both host limits"
    assert geo["one-channel-per-group"]["rows"] == 256 and geo["one-channel-per-group"]["empty_splits"] == 27, \
        "HW < GN_SPLIT: empty splits"
    zv = next(c for c in uc.GN_SHAPES if c.name == "zero-variance")
    assert zv.fill == "const" and zv.HW == 1 and geo["zero-variance"]["empty_splits"] == 31
    assert any(c.C // c.G == 1 for c in uc.GN_SHAPES), "one channel per group"
    assert uc.GN_GRADS.N == 3 and len(uc.GN_NULL_SETS) == 5 and (0, 0, 0) in uc.GN_NULL_SETS
    assert {s for s in uc.GN_NULL_SETS if sum(s) == 2} == {(0, 1, 1), (1, 0, 1), (1, 1, 0)}, "each gradient null in turn"
    assert all(v % 8 == 0 and v > 0 for v in uc.GN_STRIDES.values()) and set(uc.GN_STRIDES) == {"ldy", "ldo", "ldd", "ldu"}


def test_block_caps_are_exceeded_and_not_by_a_multiple():
    def past(items, cap, what):
        assert items > cap * 256, f"{what}: past the cap of {cap} blocks"
        assert items % (cap * 256), f"{what}: not a multiple of cap * 256"

    c = uc.GN_CAP
    past(c.N * c.HW * c.C // 8, uc.GN_GRID_CAP, "GroupNorm apply kernels (bf16)")
    b = uc.BILINEAR_CASES[0]
    past(b.N * b.h * b.w * b.C, uc.GN_GRID_CAP, "bilinear")
    g = uc.IM2COL_CAP
    Ho, Wo = uc.conv_out(g)
    past(g.N * Ho * Wo * g.K * g.K * g.C, uc.U2_GRID_CAP, "im2col")
    g = uc.COL2IM_CAP
    past(g.N * g.H * g.W * g.C, uc.U2_GRID_CAP, "col2im")
    h = uc.HEAD_CASES[0]
    past(h.M * h.heads, uc.U2_GRID_CAP, "head_softmax")
    k = uc.COL_CASES[0]
    past(k.B * k.n * k.Ch, uc.U2_GRID_CAP, "col_softmax apply / backward")
    past(uc.ACT_N, uc.ACT_GRID_CAP, "cy_act_*")
    # the cap-sized case of a family is the first of its table: it runs before any smaller case
    assert uc.BILINEAR_CASES[0].name == uc.HEAD_CASES[0].name == "past-cap" and uc.COL_CASES[0].n == 32769
    # the largest tensor is about 35 MB
    ho, wo = uc.conv_out(g)
    assert c.N * c.HW * c.C * 2 < 36e6 and ho * wo * g.K * g.K * g.C * 4 < 40e6 and h.M * h.ld * 4 < 36e6


def test_ragged_conv_geometries_and_other_tables():
    for g in uc.CONV_RAGGED:
        assert (g.H + 2 * g.pad - g.K) % g.stride and (g.W + 2 * g.pad - g.K) % g.stride, g.name
    g = uc.CONV_RAGGED[1]
    Ho, Wo = uc.conv_out(g)
    assert (Ho - 1) * g.stride - g.pad + g.K < g.H and (Wo - 1) * g.stride - g.pad + g.K < g.W, \
        "a geometry whose last input row and column are in no window"
    assert any(c.off > 0 and c.ld > c.off + c.heads * c.dh for c in uc.HEAD_CASES) and any(c.dh == 1 for c in uc.HEAD_CASES)
    assert {c.dim for c in uc.EMB_CASES} == {4, 6, 128} and all(c.B * c.dim // 2 > 256 for c in uc.EMB_CASES)
    assert set(uc.ACT_KINDS) == {0, 1}, "both activation kinds"
    assert set(uc.TYPES) == {"f32", "bf16", "f16"}, "every storage type for the templated kernels"
    up = [c for c in uc.BILINEAR_CASES if c.h > c.H and c.h % c.H and c.w % c.W]
    down = [c for c in uc.BILINEAR_CASES if c.h < c.H and c.H % c.h and c.W % c.w]
    assert up and down, "bilinear: up- and down-scaling with non-integer ratios"


def test_long_reduction_bounds_follow_the_rule():
    """bound = max(4 x yardstick, the small-size number)"""
    pairs = [(uc.GEMM_LONG_YARDSTICK, uc.GEMM_LONG_BOUND, uc.TOL_GEMM_FWD),
             (uc.COLSUM_LONG_YARDSTICK, uc.COLSUM_LONG_BOUND, uc.TOL_GEMM_GRAD),
             (uc.COL_LONG_YARDSTICK, uc.COL_LONG_BOUND, uc.TOL_SOFTMAX),
             (max(uc.LN_LONG_YARDSTICK.values()), uc.LN_LONG_BOUND, uc.TOL_LN)]
    pairs += [(uc.GN_OFFSET_YARDSTICK[k], uc.GN_OFFSET_BOUND[k], uc.TOL_GN) for k in ("out", "du")]
    pairs += [(uc.LINATTN_LONG_YARDSTICK["out"], uc.LINATTN_LONG_BOUND["out"], uc.TOL_SOFTMAX),
              (uc.LINATTN_LONG_YARDSTICK["dqkv"], uc.LINATTN_LONG_BOUND["dqkv"], uc.TOL_ATTN_GRAD)]
    for yard, bound, floor in pairs:
        assert bound == pytest.approx(max(4 * yard, floor)), (yard, bound, floor)


# ---------------------------------------------------------------- rejections
def gn_status(lib, p, *, bwd, mod, C_=16, G=2, ld=None, ws_short=0, mod_null=0):
    ld = C_ if ld is None else ld
    nbytes = lib.cy_gn_ws_bytes(1, C_) - (4 if ws_short else 0)
    ms, mt = (p, None if mod_null else p)
    if not bwd:
        if mod:
            return lib.cy_gn_silu_mod_fwd(p, ld, p, p, p, ms, mt, p, ld, p, 1, 4, C_, G, 1e-5, 0, p, nbytes, None)
        return lib.cy_gn_silu_fwd(p, ld, p, p, p, p, ld, p, 1, 4, C_, G, 1e-5, 0, p, nbytes, None)
    if mod:
        return lib.cy_gn_silu_mod_bwd(p, ld, p, ld, p, p, p, ms, mt, p, p, ld, p, p, p, p, p, 0, 1, 4, C_, G, 0, p, nbytes, None)
    return lib.cy_gn_silu_bwd(p, ld, p, ld, p, p, p, p, p, ld, p, p, p, 0, 1, 4, C_, G, 0, p, nbytes, None)


def test_groupnorm_rejections_return_the_exact_code(lib):
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    assert len(uc.GN_REJECTS) == 8
    for what, over, want in uc.GN_REJECTS:
        kw = {("C_" if k == "C" else k): v for k, v in over.items()}
        for bwd in (False, True):
            for mod in ((True,) if "mod_null" in kw else (False, True)):
                assert gn_status(lib, p, bwd=bwd, mod=mod, **kw) == want, f"GroupNorm {what} (bwd={bwd}, mod={mod})"
    # each ld on its own
    for i in range(3):
        for bad in (20, 8):
            lds = [16, 16, 16]
            lds[i] = bad
            assert lib.cy_gn_silu_bwd(p, lds[0], p, lds[1], p, p, p, p, p, lds[2], p, p, p, 0, 1, 4, 16, 2, 0, p,
                                      lib.cy_gn_ws_bytes(1, 16), None) == uc.ERR_SHAPE, f"backward ld #{i} = {bad}"
    for lds in ((20, 16), (16, 20), (8, 16), (16, 8)):
        assert lib.cy_gn_silu_fwd(p, lds[0], p, p, p, p, lds[1], p, 1, 4, 16, 2, 1e-5, 0, p, lib.cy_gn_ws_bytes(1, 16),
                                  None) == uc.ERR_SHAPE, f"forward ld {lds}"
    # a type code that is no type
    assert lib.cy_gn_silu_fwd(p, 16, p, p, p, p, 16, p, 1, 4, 16, 2, 1e-5, 7, p, lib.cy_gn_ws_bytes(1, 16), None) == uc.ERR_DTYPE


def test_other_rejections_return_the_exact_code(lib):
    from cyhip._lib import MatLayout
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    seen = []

    def expect(what, got, want):
        assert what in uc.OTHER_REJECTS, what
        assert got == want, f"{what}: {got}, expected {want}"
        seen.append(what)

    lay = MatLayout(4, 1, 0, 0)
    r = C.byref(lay)

    def gemm(nb1, nb2, ksplit, ws, ws_bytes):
        return lib.cy_gemm_strided(p, r, p, r, p, r, None, 4, 4, 4, nb1, nb2, 1.0, 0, ksplit, ws, ws_bytes, None)

    expect("gemm nbatch*ksplit > 65535", gemm(256, 128, 2, p, 1 << 40), uc.ERR_SHAPE)
    full = lib.cy_gemm_strided_ws_bytes(4, 4, 1, 2)
    assert full == 2 * 16 * 4
    expect("gemm split-K null workspace", gemm(1, 1, 2, None, full), uc.ERR_WORKSPACE)
    expect("gemm split-K short workspace", gemm(1, 1, 2, p, full - 1), uc.ERR_WORKSPACE)
    expect("col_softmax B > 65535", lib.cy_col_softmax_fwd(p, 4, 0, p, 65536, 1, 4, p, 1 << 40, None), uc.ERR_SHAPE)
    expect("act kind 2", lib.cy_act_fwd(p, p, 4, 2, None), uc.ERR_SHAPE)
    assert lib.cy_act_bwd(p, p, p, 4, 2, None) == uc.ERR_SHAPE and lib.cy_act_fwd(p, p, 4, -1, None) == uc.ERR_SHAPE
    expect("sinusoidal dim 2", lib.cy_sinusoidal_emb(p, p, 1, 2, None), uc.ERR_SHAPE)
    expect("sinusoidal dim 5", lib.cy_sinusoidal_emb(p, p, 1, 5, None), uc.ERR_SHAPE)
    expect("colsum short workspace", lib.cy_colsum(p, p, 257, 4, 0, p, lib.cy_colsum_ws_bytes(257, 4) - 1, None),
           uc.ERR_WORKSPACE)
    expect("layernorm bwd short workspace",
           lib.cy_chan_layernorm_bwd(p, p, p, p, p, p, 257, 4, 1e-5, p, lib.cy_chan_layernorm_bwd_ws_bytes(257, 4) - 1, None),
           uc.ERR_WORKSPACE)
    expect("col_softmax short workspace",
           lib.cy_col_softmax_fwd(p, 4, 0, p, 1, 129, 4, p, lib.cy_col_softmax_ws_bytes(1, 129, 4) - 1, None),
           uc.ERR_WORKSPACE)
    assert sorted(seen) == sorted(uc.OTHER_REJECTS)
    # softmax row layouts narrower than what they hold
    assert lib.cy_head_softmax_fwd(p, 7, 0, p, 1, 2, 4, 1.0, None) == uc.ERR_SHAPE
    assert lib.cy_head_softmax_bwd(p, p, p, 8, 1, 1, 2, 4, 1.0, None) == uc.ERR_SHAPE
    assert lib.cy_col_softmax_fwd(p, 4, 1, p, 1, 1, 4, p, 1 << 20, None) == uc.ERR_SHAPE
    assert lib.cy_col_softmax_bwd(p, p, p, p, 4, 1, 1, 1, 4, None) == uc.ERR_SHAPE
