"""tests/test_gpu_contrast_dispatch.py claims to reach every host-side branch and every capped loop of
csrc/cy_contrast.hip and csrc/cy_proj_head.hip.  The claim is checked here on the CPU, against the same tables (tests/contrast_cases.py).  The
column-split count of the fused SupCon kernels comes from the library's own workspace query; the geometry the library
does not export is restated in the case module next to its source line.  Each assertion names its branch: deleting a
case fails here, by name, without a GPU.  The rejections of these entry points are asserted here too: a refused call
launches nothing, so host buffers do."""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import contrast_cases as cc


@pytest.fixture(scope="module")
def lib():
    from cyhip import _lib
    return _lib.load()


def splits(lib, R, D=8):
    """ns from cy_supcon_fused_ws_bytes: (R + 4 + ns * R * max(3, D)) floats"""
    return (lib.cy_supcon_fused_ws_bytes(R // 2, D) // 4 - R - 4) // (R * max(3, D))


# ---------------------------------------------------------------- the golden masks
def test_golden_masks_are_what_their_names_promise(golden_dir):
    g = np.load(golden_dir / cc.GOLDEN_FILE)
    n, D = g["z1"].shape
    assert (n, D) == (cc.GOLDEN_N, cc.GOLDEN_D) == (70, 16) and float(g["t"]) == cc.T
    assert cc.row_blocks(2 * n) == 3, "R = 140 spans three 64-row tiles"
    assert cc.SC_TM < n < 2 * cc.SC_TM, "the fold row - n crosses a tile boundary inside tile 1"
    assert set(cc.GOLDEN_MASKS) == {"a", "b", "c", "d", "z"}, "the five masks of the issue"
    for name, (neither, symmetric) in cc.GOLDEN_MASKS.items():
        m = torch.from_numpy(g[f"{name}_mask"])
        assert m.shape == (n, n)
        assert bool(((m != 0) & (m != 1)).any()) == neither, f"mask {name}: pairs that are neither"
        assert torch.equal(m == 1, (m == 1).t()) == symmetric, f"mask {name}: symmetry of the positives"
        diag = 0 if name == "z" else 1
        assert bool((m.diagonal() == diag).all()), f"mask {name}: diagonal"
        assert int(g[f"{name}_pos"].sum(1).min()) >= 1, f"mask {name}: every row has a positive"
        for e in (0, 1):
            assert g[f"{name}_e{e}_dz1"].shape == g[f"{name}_e{e}_dz2"].shape == (n, D) and np.isfinite(g[f"{name}_e{e}_loss"])
    assert set(np.unique(g["c_mask"]).tolist()) == {0, 1, -1} and set(np.unique(g["d_mask"]).tolist()) == set(cc.MASK_D_VALUES)
    assert g["d_sim_logits"].shape == g["d_sim_exp"].shape == (2 * n, 2 * n)
    assert (golden_dir / cc.GOLDEN_FILE).stat().st_size < 300_000, "well under the other goldens"
    assert set(cc.PATHS) == {"materialised", "fused", "exclude_other_pos"}


def test_kind_d_masks_of_the_generated_cases():
    for n, seed in ((cc.WIDTH_N, 61), (cc.CAP_N, 62)):
        m = cc.kind_d_mask(n, seed)
        assert set(m.unique().tolist()) == set(cc.MASK_D_VALUES) == {0, 1, -1, 2}
        assert bool((m.diagonal() == 1).all()) and not torch.equal(m == 1, (m == 1).t()) and not torch.equal(m == 0, (m == 0).t())
        assert set(m.to(torch.uint8).unique().tolist()) == {0, 1, 2, 255}, "as uint8 codes: two values that are neither"


# ---------------------------------------------------------------- column splits of the fused kernels
def test_column_split_geometry_by_name(lib):
    by = {c.name: c for c in cc.SPLIT_CASES}
    got = {c.name: (2 * c.n, cc.row_blocks(2 * c.n), splits(lib, 2 * c.n, c.D)) for c in cc.SPLIT_CASES}
    assert got["one-pair"] == (2, 1, 1) and by["one-pair"].positives == "simclr", "R = 2: n = 1, SimCLR labels"
    assert got["one-full-tile"] == (64, 1, 1), "R = 64: exactly one full tile"
    assert got["two-row-second-tile"] == (66, 2, 2), "R = 66: a second tile of two rows"
    assert got["splits-of-one-and-two-blocks"] == (1040, 17, 15), "R = 1040: 17 row blocks, 15 splits"
    assert sorted(set(cc.split_blocks(1040, 15))) == [1, 2], "R = 1040: splits of one and of two column blocks"
    assert got["129-row-blocks"] == (8200, 129, 1), "R = 8200: 129 row blocks, one split"
    assert got["past-the-split-budget"] == (16400, 257, 1), "R = 16400: 256 / rb = 0, clamped to one"
    assert cc.SC_SPLIT_BUDGET // 257 == 0 and cc.SC_SPLIT_BUDGET // 129 == 1
    for c in cc.SPLIT_CASES:
        assert got[c.name][1:] == (c.row_blocks, c.splits), f"{c.name}: the table's own counts"
        if 2 * c.n >= cc.CHUNKED_FROM:
            assert c.paths == ("fused",) and c.D == 8 and c.positives == "mod3", f"{c.name}: fused only, D = 8, labels i % 3"
        else:
            assert set(c.paths) == set(cc.PATHS), f"{c.name}: all three paths"
    assert cc.CHUNK_ROWS <= 512 and cc.CHUNKED_FROM == 8200
    assert by["one-pair"].twins and not any(c.twins for c in cc.SPLIT_CASES if c.name != "one-pair")
    rows = cc.twin_rows(1, by["one-pair"].D)
    assert sum(v * v for v in rows[0]) == 1.0 and {abs(v) for v in rows[0]} == {0.25} and len(set(rows[0])) == 2
    # R = 4096 is not repeated: it runs in test_gpu_kernels.py
    ct = cc.SPLIT_CITED
    assert (ct["R"], cc.row_blocks(ct["R"]), splits(lib, ct["R"], 256)) == (4096, ct["row_blocks"], ct["splits"]) == (4096, 64, 4)
    src = (Path(__file__).resolve().parent / ct["file"]).read_text()
    m = re.search(r"@pytest\.mark\.parametrize\(\"n,D\", \[(.*?)\]\)\ndef " + ct["test"] + r"\(", src)
    assert m and ct["param"] in m.group(1), "the cited R = 4096 case is still there"


def test_chunked_reference_is_the_oracle():
    """the row-chunked float64 reference of the two largest cases against the oracle's whole-matrix one, at a size with
    three chunks, the last one short"""
    from tests import test_gpu_contrast_dispatch as gd
    n, D = 520, 8
    assert 2 * n > 2 * cc.CHUNK_ROWS and (2 * n) % cc.CHUNK_ROWS
    loss, dP = gd.chunked_ref(n, D, 77, "mod3")
    oloss, odP = gd.oracle_ref(n, D, 77, "mod3", False)
    assert abs(loss - oloss) <= 1e-12 * abs(oloss)
    assert (dP - odP).abs().max().item() <= 1e-12 * odP.abs().max().item()


# ---------------------------------------------------------------- embedding widths
def fused_status(lib, p, D, *, bwd, ws_bytes):
    n = 4
    if bwd:
        return lib.cy_supcon_fused_bwd(p, p, None, p, p, p, p, ws_bytes, n, D, cc.T, None)
    return lib.cy_supcon_fused_fwd(p, p, None, p, p, None, p, ws_bytes, n, D, cc.T, None)


def test_widths_and_which_of_them_the_fused_path_refuses(lib):
    from cyhip import ops
    assert set(cc.FUSED_WIDTHS) == {8, 40, 96, 136, 248, 256} and set(cc.MATERIALISED_WIDTHS) == {1, 17, 257, 264}
    tiles = {D: -(-D // cc.DP_TILE) for D in cc.FUSED_WIDTHS}
    assert tiles == {8: 1, 40: 2, 96: 3, 136: 5, 248: 8, 256: 8}, "1, 2, 3, 5 and 8 column tiles of the second product"
    assert 248 % cc.DP_TILE and not 256 % cc.DP_TILE, "the eighth tile ragged, and full"
    ks = cc.MATERIALISED_WIDTHS
    assert min(ks) < cc.SGEMM_KSTAGE < 17 <= max(ks) and 17 % cc.SGEMM_KSTAGE, "K below, across and past the 16-wide stage"
    assert cc.row_blocks(2 * cc.WIDTH_N) == 2 and splits(lib, 2 * cc.WIDTH_N) == 2
    # supcon_fused_ok and the two entry points agree on every width up to 272: a refused width is CY_ERR_SHAPE, an
    # accepted one gets as far as the workspace check (one byte short: nothing is launched)
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    assert ops.SUPCON_FUSED
    for D in range(1, 273):
        ok = ops.supcon_fused_ok(SimpleNamespace(shape=(8, D)))
        want = cc.ERR_WORKSPACE if ok else cc.ERR_SHAPE
        short = lib.cy_supcon_fused_ws_bytes(4, D) - 1
        for bwd in (False, True):
            assert fused_status(lib, p, D, bwd=bwd, ws_bytes=short) == want, f"width {D} (bwd={bwd}), supcon_fused_ok={ok}"
    assert all(ops.supcon_fused_ok(SimpleNamespace(shape=(70, D))) for D in cc.FUSED_WIDTHS)
    assert not any(ops.supcon_fused_ok(SimpleNamespace(shape=(70, D))) for D in cc.MATERIALISED_WIDTHS)


def test_block_cap_is_exceeded_and_not_by_a_multiple():
    R = 2 * cc.CAP_N
    assert R == 1450 and R * R > cc.GRID_CAP * 256 == 2097152 and (R * R) % (cc.GRID_CAP * 256), "R = 1450 past GRID_CAP"
    N, HW, Cc = cc.POOL_CAP
    assert 0 < N * HW * Cc - cc.GRID_CAP * 256 < 1024, "avgpool backward just above 2 097 152 elements"
    assert cc.GSCALE != 1 and cc.SGEMM_ALPHA != 1


# ---------------------------------------------------------------- sgemm and the projector pieces
def test_sgemm_and_piece_tables():
    assert set(cc.SGEMM_SIZES) == {(1, 1, 1), (64, 64, 16), (65, 63, 17), (130, 5, 2), (3, 200, 45)}
    assert any(M > 128 for M, _, _ in cc.SGEMM_SIZES) and any(N > 192 for _, N, _ in cc.SGEMM_SIZES), "three and four tiles"
    assert {K % cc.SGEMM_KSTAGE == 0 for _, _, K in cc.SGEMM_SIZES} == {True, False}
    assert set(cc.POOL_HW) == {1, 3, 4, 7} and {(hw // 4 > 0, hw % 4 > 0) for hw in cc.POOL_HW} == {(False, True), (True, False), (True, True)}, \
        "the four-way unroll: tail only, rounds only, both"
    assert set(cc.POOL_C) == {8, 256, 264} and -(-264 // 256) == 2, "a second channel block, partly idle"
    assert set(cc.LINEAR_I) == {1, 63, 64, 65} and set(cc.LINEAR_O) == {1, 3, 4, 5}
    assert {(o // 4 > 0, o % 4 > 0) for o in cc.LINEAR_O} == {(False, True), (True, False), (True, True)}, "the four-chain loop and its tail"
    assert set(cc.LINEAR_ACTS) == {0, 1} and len(set(cc.LINEAR_WANTS)) == 8, "both activations; each combination of null dx / dw / db"
    assert (cc.LINEAR_M * max(cc.LINEAR_O)) % 4 and cc.LINEAR_M * min(cc.LINEAR_I) < 256, "a part-filled last block"
    assert set(cc.L2_D) == {1, 63, 64, 65, 300} and set(cc.L2_M) == {1, 4, 5} and cc.L2_ZERO_ROW == 0
    assert set(cc.TYPES) == {"f32", "bf16", "f16"}


# ---------------------------------------------------------------- the one-launch projection head
def test_proj_head_tables_and_paths():
    from cyhip import ops
    assert set(cc.HEAD_SHAPES) == {(8, 4, 1), (512, 512, 512), (264, 260, 3), (128, 256, 256)}
    assert set(cc.HEAD_HW) == {1, 5, 16, 17, 196} and set(cc.HEAD_B) == {1, 3}
    nsl = {(s[0], dt): cc.pool_slices(s[0], dt) for s in cc.HEAD_SHAPES for dt in cc.TYPES}
    assert nsl[(512, "f32")] == 8 and nsl[(264, "f32")] == 15 and nsl[(128, "f32")] == nsl[(8, "bf16")] == 16
    full = [k for k, v in nsl.items() if v == cc.PH_NW]
    assert full and {hw < 16 for hw in cc.HEAD_HW} == {True, False} and 16 in cc.HEAD_HW and 17 in cc.HEAD_HW, \
        "fewer positions than pooling slices, equal, one more"
    assert any(s[2] < cc.PH_NW for s in cc.HEAD_SHAPES) and any(s[1] % 64 for s in cc.HEAD_SHAPES)
    fake = lambda *shape: SimpleNamespace(shape=shape, is_cuda=True, dtype=torch.float32)  # noqa: E731
    for s in cc.HEAD_SHAPES:
        assert ops.proj_head_ok(fake(1, s[0], 1, 1), fake(s[1], s[0]), fake(s[2], s[1])), f"{s}: one launch"
    assert [s for s in cc.HEAD_SHAPES if s[2] == 1] == [(8, 4, 1)], "the one shape whose gradients cancel to zero"
    assert set(cc.HEAD_OUT1_BOUND) == {"dfeat", "dw1", "db1", "dw2", "db2"}
    for k, yard in cc.HEAD_OUT1_YARDSTICK.items():
        assert cc.HEAD_OUT1_BOUND[k] == pytest.approx(2 * yard) and yard < 1e-6, f"{k}: twice the float32 yardstick"
    z = cc.HEAD_ZERO
    assert z["shape"] in cc.HEAD_SHAPES and 0 <= z["sample"] < z["B"]
    names = {c[0]: c for c in cc.MODULE_CASES}
    assert set(names) == {"one-launch", "wide-input", "odd-hidden"}
    for name, Cc, hid, out, one in cc.MODULE_CASES:
        assert ops.proj_head_ok(fake(3, Cc, 3, 2), fake(hid, Cc), fake(out, hid)) == one, f"{name}: which path"
    assert names["wide-input"][1] == 520 and names["odd-hidden"][2] == 6 and names["one-launch"][4]


# ---------------------------------------------------------------- rejections
def supcon_status(lib, entry, p, *, n=4, D=8, t=cc.T, null="", ws_short=0):
    P = None if null == "P" else p
    lab = None if null == "labels+mask" else p
    out = None if null == "out" else p
    ws = None if null == "ws" else p
    nbytes = lib.cy_supcon_fused_ws_bytes(max(n, 1), max(D, 1)) - ws_short
    if entry == "cy_supcon_fwd":
        return lib.cy_supcon_fwd(P, lab, None, p, out, p, n, D, t, None)
    if entry == "cy_supcon_bwd":
        return lib.cy_supcon_bwd(P, lab, None, p, p, p, p, out, n, D, t, None)
    if entry == "cy_supcon_excl_fwd":
        return lib.cy_supcon_excl_fwd(P, lab, None, p, out, p, p, n, D, t, None)
    if entry == "cy_supcon_excl_bwd":
        return lib.cy_supcon_excl_bwd(P, lab, None, p, p, p, p, p, out, n, D, t, None)
    if entry == "cy_supcon_fused_fwd":
        return lib.cy_supcon_fused_fwd(P, lab, None, out, p, None, ws, nbytes, n, D, t, None)
    assert entry == "cy_supcon_fused_bwd"
    return lib.cy_supcon_fused_bwd(P, lab, None, p, p, out, ws, nbytes, n, D, t, None)


def test_supcon_rejections_return_the_exact_code(lib):
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    whats = [r[0] for r in cc.SUPCON_REJECTS]
    for needed in ("P null", "neither labels nor mask", "an output null", "n = 0", "n < 0", "D = 0", "D < 0", "t = 0", "t < 0",
                   "fused D = 257", "fused D = 12", "fused workspace one byte short", "fused workspace null"):
        assert needed in whats, needed
    for what, over, want, entries in cc.SUPCON_REJECTS:
        for entry in entries:
            assert supcon_status(lib, entry, p, **over) == want, f"{entry}: {what}"
    # a mask alone is accepted as far as the next check; cy_supcon_matrices has one status for everything
    assert lib.cy_supcon_fused_fwd(p, None, p, p, p, None, p, 0, 4, 8, cc.T, None) == cc.ERR_WORKSPACE
    assert lib.cy_supcon_matrices(p, p, None, None, p, p, p, p, 4, None) == cc.ERR_ARG
    assert lib.cy_supcon_matrices(None, p, p, None, p, p, p, p, 4, None) == cc.ERR_ARG
    assert lib.cy_supcon_matrices(p, p, p, None, p, p, p, p, 0, None) == cc.ERR_ARG
    assert lib.cy_supcon_fused_ws_bytes(0, 8) == 0 and lib.cy_supcon_fused_ws_bytes(4, 0) == 0
    assert lib.cy_sgemm(None, p, p, 1, 1, 1, 1.0, 0, None) == cc.ERR_ARG and lib.cy_sgemm(p, p, p, 1, 0, 1, 1.0, 0, None) == cc.ERR_ARG


def head_status(lib, p, *, bwd, C_=8, hid=4, out=1, dtype=0, ws_short=0, null=0):
    first = None if null else p
    if not bwd:
        return lib.cy_proj_head_fwd(first, p, p, p, p, p, p, p, p, p, 1, 1, C_, hid, out, 0.01, 1e-12, dtype, None)
    nbytes = lib.cy_proj_head_bwd_ws_bytes(1, hid, out) - ws_short
    return lib.cy_proj_head_bwd(first, p, p, p, p, p, p, p, p, p, p, p, 0, p, nbytes, 1, 1, C_, hid, out, 0.01, 1e-12, dtype,
                                None)


def test_proj_head_rejections_return_the_exact_code(lib):
    from cyhip import _lib
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    whats = [r[0] for r in cc.HEAD_REJECTS]
    for needed in ("C = 520", "C = 12", "hid = 6", "hid = 516", "out = 513", "unknown dtype code", "short workspace",
                   "feat / dz null"):
        assert needed in whats, needed
    assert 7 not in (_lib.CY_F32, _lib.CY_BF16, _lib.CY_F16)
    for what, over, want in cc.HEAD_REJECTS:
        kw = {("C_" if k == "C" else k): v for k, v in over.items()}
        for bwd in ((True,) if "ws_short" in kw else (False, True)):
            assert head_status(lib, p, bwd=bwd, **kw) == want, f"proj_head {what} (bwd={bwd})"
    assert lib.cy_proj_head_bwd_ws_bytes(3, 256, 256) == 3 * 512 * 4
    # the pieces: null pointers and empty shapes
    assert lib.cy_avgpool_fwd(None, p, 1, 1, 8, 0, None) == cc.ERR_ARG and lib.cy_avgpool_bwd(p, p, 1, 0, 8, 0, None) == cc.ERR_ARG
    assert lib.cy_linear_fwd(p, None, p, p, 1, 1, 1, 0, 0.0, None) == cc.ERR_ARG
    assert lib.cy_linear_bwd(p, p, p, None, p, p, p, 1, 1, 1, 0, 0.0, None) == cc.ERR_ARG
    assert lib.cy_linear_bwd_into(p, p, p, p, p, p, p, 1, 1, 0, 0, 0.0, None) == cc.ERR_ARG
    assert lib.cy_l2norm_fwd(p, p, None, 1, 1, 1e-12, None) == cc.ERR_ARG and lib.cy_l2norm_bwd(p, p, p, p, 0, 1, 1e-12, None) == cc.ERR_ARG
