"""DenseProjectionHead without pooling, and the C ABI of the per-row projector it runs on (csrc/cy_pixel_mlp.hip), as
far as a machine without a GPU can check them: construction and parameter names, the argument errors of the four entry
points (none of which launches), the workspace rule, what the parity cases of tests/test_gpu_dense_options.py reach
according to the host-side plan, and that the recorded 16-bit emulation errors are what the emulation gives."""
import ctypes as C

import pytest
import torch

from tests import dense_option_cases as dc

POOLS = ("identical", "none", None)
ARG, SHAPE, WORKSPACE = -1, -2, -5


def _head(pool, head_type, **kw):
    from contrastyou.projectors import DenseProjectionHead
    return DenseProjectionHead(input_dim=16, hidden_dim=32, output_dim=24, head_type=head_type, normalize=True,
                               pool_name=pool, **kw)


@pytest.mark.parametrize("head_type", ("mlp", "linear"))
@pytest.mark.parametrize("pool", POOLS)
def test_unpooled_head_constructs_with_the_reference_layout(pool, head_type):
    from contrastyou.projectors.nn import Identical
    head = _head(pool, head_type)
    assert isinstance(head._pooling_module, Identical)
    want = ["_projector.0.bias", "_projector.0.weight"]
    if head_type == "mlp":
        want += ["_projector.2.bias", "_projector.2.weight"]
    assert sorted(head.state_dict()) == want
    assert tuple(head._projector[0].weight.shape) == ((32 if head_type == "mlp" else 24), 16, 1, 1)
    features = torch.zeros(2, 16, 7, 9)
    assert head.output_size(features) == (7, 9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head(features)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head.project_points(features, [[(0, 0)], [(6, 8)]])


def test_output_size_of_the_pooling_heads_is_the_pooling_grid():
    features = torch.zeros(2, 16, 7, 9)
    assert _head("adaptive_avg", "mlp", spatial_size=(4, 3)).output_size(features) == (4, 3)
    assert _head("adaptive_max", "linear", spatial_size=5).output_size(features) == (5, 5)
    assert _head("adaptive_avg", "mlp").output_size(features) == (16, 16)


def test_function_refuses_cpu_tensors():
    from cyhip.functions import PixelMLPFn
    x, w1, b1 = torch.zeros(4, 8), torch.zeros(5, 8), torch.zeros(5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PixelMLPFn.apply(x, None, w1, b1, None, None, 0.01, True)


def test_fused_range():
    from cyhip import ops
    assert ops.pixel_mlp_ok(1, 0, 1) and ops.pixel_mlp_ok(256, 256, 256) and ops.pixel_mlp_ok(8, 1, 5)
    assert not any(ops.pixel_mlp_ok(*s) for s in ((0, 8, 8), (257, 8, 8), (8, 257, 8), (8, 8, 0), (8, 8, 257), (8, -1, 8)))


def _fwd(lib, p, *, M=10, Cc=8, ldx=8, hid=16, out=4, x=True, w1=True, b1=True, w2=True, b2=True, y=True, inv=True,
         normalize=1, dtype=0):
    a = lambda on: p if on else None  # noqa: E731
    return lib.cy_pixel_mlp_fwd(a(x), None, a(w1), a(b1), a(w2), a(b2), a(y), a(inv), M, Cc, ldx, hid, out, 0.01,
                                normalize, dtype, None)


def _bwd(lib, p, *, M=10, Cc=8, ldx=8, hid=16, out=4, x=True, w1=True, b1=True, w2=True, y=True, inv=True, dy=True,
         normalize=1, dtype=0, ws=True, ws_bytes=None):
    a = lambda on: p if on else None  # noqa: E731
    if ws_bytes is None:
        ws_bytes = lib.cy_pixel_mlp_bwd_ws_bytes(M, Cc, hid, out, dtype)
    return lib.cy_pixel_mlp_bwd(a(x), None, a(w1), a(b1), a(w2), a(y), a(inv), a(dy), p, p, p, p, p, 0, M, Cc, ldx, hid,
                                out, 0.01, normalize, dtype, a(ws), ws_bytes, None)


def test_argument_errors_come_before_any_launch():
    """(the pointers are host addresses nothing dereferences: every call here returns before its launch)"""
    from cyhip import _lib
    lib = _lib.load()
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    plan = _lib.PixelMlpPlan()
    assert lib.cy_pixel_mlp_plan(10, 8, 16, 4, 0, plan) == 0 and lib.cy_pixel_mlp_plan(10, 8, 16, 4, 0, None) == ARG
    for name in ("x", "w1", "b1", "w2", "b2", "y", "inv"):
        assert _fwd(lib, p, **{name: False}) == ARG, name
    for name in ("x", "w1", "b1", "w2", "y", "inv", "dy"):
        assert _bwd(lib, p, **{name: False}) == ARG, name
    for bad in (dict(Cc=257, ldx=257), dict(hid=257), dict(out=0), dict(out=257), dict(Cc=0), dict(M=0), dict(hid=-1)):
        s = dict(M=10, Cc=8, hid=16, out=4)
        s.update({k: v for k, v in bad.items() if k != "ldx"})
        assert lib.cy_pixel_mlp_plan(s["M"], s["Cc"], s["hid"], s["out"], 0, plan) == SHAPE, bad
        assert _fwd(lib, p, **bad) == SHAPE, bad
        assert _bwd(lib, p, ws_bytes=1 << 30, **bad) == SHAPE, bad
        assert lib.cy_pixel_mlp_bwd_ws_bytes(s["M"], s["Cc"], s["hid"], s["out"], 0) == 0
    assert _fwd(lib, p, ldx=7) == SHAPE and _bwd(lib, p, ldx=7) == SHAPE  # pixel stride < C
    assert lib.cy_pixel_mlp_plan(10, 8, 16, 4, 3, plan) == -3  # CY_ERR_DTYPE
    # the linear head takes no second layer: its arguments pass, and the missing workspace is what refuses the call
    assert _bwd(lib, p, hid=0, w2=False, ws_bytes=0) == WORKSPACE
    need = lib.cy_pixel_mlp_bwd_ws_bytes(10, 8, 16, 4, 0)
    assert need > 0
    assert _bwd(lib, p, ws_bytes=need - 1) == WORKSPACE and _bwd(lib, p, ws=False) == WORKSPACE


def test_workspace_follows_the_plan_and_stops_growing_at_the_cap():
    from cyhip import _lib, ops
    lib = _lib.load()
    for Cc, hid, out, dt, code in ((32, 256, 256, torch.bfloat16, 1), (8, 0, 5, torch.float32, 0), (256, 64, 32, torch.float16, 2)):
        assert lib.cy_pixel_mlp_bwd_ws_bytes(10 ** 6, Cc, hid, out, code) == lib.cy_pixel_mlp_bwd_ws_bytes(10 ** 7, Cc, hid, out, code)
        for M in (1, 100, 10 ** 6):
            p = ops.pixel_mlp_plan(M, Cc, hid, out, dt)
            up = lambda v: -(-v // 32) * 32  # noqa: E731
            j = up(hid) if hid else up(out)
            slab = j * up(Cc) + j + (up(out) * up(hid) + up(out) if hid else 0)
            assert lib.cy_pixel_mlp_bwd_ws_bytes(M, Cc, hid, out, code) == 4 * p["slabs"] * slab
            tiles = -(-M // p["rows_per_tile"])
            assert p["fwd_grid"] == min(tiles, 1024) and p["bwd_grid"] == min(tiles, 256) == p["slabs"]
            assert (p["fwd_trips"] - 1) * p["fwd_grid"] < tiles <= p["fwd_trips"] * p["fwd_grid"]
            assert (p["bwd_trips"] - 1) * p["bwd_grid"] < tiles <= p["bwd_trips"] * p["bwd_grid"]
            assert p["lds_bytes"] <= 160 * 1024
    assert ops.pixel_mlp_plan(10, 256, 256, 256, torch.float32)["lds_bytes"] <= 160 * 1024


def test_cases_reach_every_form_of_the_plan():
    from cyhip import _lib
    plans = [(c, dc.plan(c)) for c in dc.CASES]
    forms = {(p["form"], c.dtype) for c, p in plans}
    assert forms == {(_lib.CY_PIXEL_MLP_MFMA32, "f32"), (_lib.CY_PIXEL_MLP_MFMA16, "bf16"), (_lib.CY_PIXEL_MLP_MFMA16, "f16")}
    assert {p["rows_per_tile"] for c, p in plans} == {32, 64}
    for form in (_lib.CY_PIXEL_MLP_MFMA16, _lib.CY_PIXEL_MLP_MFMA32):
        mine = [(c, p) for c, p in plans if p["form"] == form]
        assert any(c.M == 1 for c, p in mine), "no one-row problem"
        assert any(c.M > p["rows_per_tile"] and c.M % p["rows_per_tile"] for c, p in mine), "no partial last tile behind a full one"
        assert any(p["fwd_trips"] > 1 for c, p in mine), "no second trip of the forward loop"
        assert any(p["bwd_trips"] > 1 and c.hid > 0 for c, p in mine), "no second trip of the backward loop (mlp)"
        assert any(p["slabs"] > 1 for c, p in mine)
        assert {c.hid == 0 for c, p in mine} == {True, False}, "linear and mlp"
        assert {c.idx for c, p in mine} == {True, False} and {c.normalize for c, p in mine} == {True, False}
    # the smallest row count that passes the forward cap, exactly
    for c, p in plans:
        if p["fwd_trips"] > 1:
            assert c.M == 1024 * p["rows_per_tile"] + 1
    assert {c.C for c in dc.CASES} == {8, 32, 256} and {c.hid for c in dc.CASES} == {0, 64, 256}
    assert {c.out for c in dc.CASES} == {5, 32, 256} and {c.M for c in dc.CASES} >= {1, 63, 126}
    assert any(c.ldx > c.C for c in dc.CASES)
    assert any(c.dtype == "bf16" and c.hid and p["bwd_trips"] > 1 for c, p in plans)


def test_recorded_emulation_errors_are_what_the_emulation_gives():
    """the 16-bit bounds of the GPU test are twice these numbers: they are measured (tests/dense_option_cases.emulate
    against the float64 reference), not chosen, and this keeps the record honest when a case or the emulation changes"""
    from tests.test_gpu_dense_options import EMU_ERR
    ids = {dc.case_id(c) for c in dc.CASES if c.dtype != "f32"}
    assert set(EMU_ERR) == ids
    for c in dc.CASES:
        if c.dtype == "f32":
            continue
        ref, emu = dc.reference(c), dc.emulate(c)
        rec = EMU_ERR[dc.case_id(c)]
        assert set(rec) == set(ref)
        for k in ref:
            e = dc.rel_err(emu[k], ref[k])
            assert rec[k] / 1.1 <= e <= rec[k] * 1.1, (dc.case_id(c), k, e, rec[k])
