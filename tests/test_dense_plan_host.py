"""cy_dense_proj_plan, the host-side rule cy_dense_proj_fwd / _bwd / _bwd_ws_bytes follow when they choose between the
VALU kernels, the register-resident matrix-core form (C = 32 / 64 / 128) and the streamed form (C = 256 / 512) of the
dense projector: which form each map gets, what the streamed form asks of LDS and of the workspace, the argument
errors, and the CY_DENSE_MFMA=0 switch (read once per process, so asked of a fresh child).  No GPU."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parents[1]
ARG, SHAPE, DTYPE = -1, -2, -3
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
LDS_MAX = 160 * 1024
PARTIALS = 512 * 68 * 64 * 4  # the dW1 kernels' workgroup partials
REC = 64                      # bytes of a job record


@pytest.fixture(scope="module")
def lib():
    from cyhip import _lib
    return _lib.load()


@pytest.mark.parametrize("cin,hid,dtype", [(256, 256, BF16), (256, 128, F16), (512, 256, BF16), (512, 128, F16)])
def test_wide_maps_run_the_streamed_form(cin, hid, dtype):
    from cyhip import _lib, ops
    p = ops.dense_proj_plan(cin, hid, dtype)
    assert p["form"] == _lib.CY_DENSE_PROJ_MFMA_STREAM
    assert p["channel_blocks"] == cin // 32
    assert 0 < p["lds_bytes"] <= LDS_MAX
    assert p["fwd_passes"] == hid // 128
    assert p["dw_passes"] == 1  # (dW1 / db1 of these maps run the VALU kernel)
    # W1 of one pass in 16 bits beside the per-wave tiles: 128 units x C x 2 bytes at least, all of it at most
    assert p["lds_bytes"] >= 128 * cin * 2
    # the dx kernel contracts over every hidden unit: where hid x C x 2 bytes do not fit beside its tiles it reads W1 from
    # the workspace
    assert p["w1_image_in_ws"] == (1 if 32 * 1024 + hid * cin * 2 > LDS_MAX else 0)
    # VALU dW1 + slab sum + job table (+ W1 image), then dx per block of 32 channels (x 4 colour classes with a bin list)
    assert p["bwd_launches"] == 3 + p["w1_image_in_ws"] + p["channel_blocks"]
    assert p["bwd_launches_list"] == 3 + p["w1_image_in_ws"] + 4 * p["channel_blocks"]


def test_c512_takes_more_than_one_pass_over_the_hidden_units():
    from cyhip import ops
    assert ops.dense_proj_plan(512, 256, BF16)["fwd_passes"] == 2
    assert ops.dense_proj_plan(512, 256, BF16)["w1_image_in_ws"] == 1
    assert ops.dense_proj_plan(256, 256, BF16)["w1_image_in_ws"] == 0


@pytest.mark.parametrize("cin", [32, 64, 128])
@pytest.mark.parametrize("hid", [128, 256])
@pytest.mark.parametrize("dtype", [BF16, F16])
def test_narrow_maps_keep_the_register_resident_form(cin, hid, dtype):
    from cyhip import _lib, ops
    p = ops.dense_proj_plan(cin, hid, dtype)
    assert p["form"] == _lib.CY_DENSE_PROJ_MFMA_REG
    assert p["channel_blocks"] == cin // 32
    assert p["lds_bytes"] == 0 and p["w1_image_in_ws"] == 0  # (its LDS is static)
    assert p["dw_passes"] == hid // 128
    assert p["fwd_passes"] == {32: 1, 64: hid // 128, 128: hid // 64}[cin]


@pytest.mark.parametrize("cin,hid,dtype,slope", [
    (256, 256, F32, 0.01), (32, 128, F32, 0.01),    # f32 maps
    (256, 256, BF16, 1.5), (64, 128, F16, 1.5),     # slope > 1: lrelu is not max(t, slope t)
    (96, 256, BF16, 0.01), (1024, 128, BF16, 0.01), (8, 128, F16, 0.01),
    (256, 64, BF16, 0.01), (512, 192, F16, 0.01), (32, 64, BF16, 0.01),
])
def test_everything_else_stays_on_the_valu_kernels(cin, hid, dtype, slope):
    from cyhip import _lib, ops
    p = ops.dense_proj_plan(cin, hid, dtype, slope)
    assert p["form"] == _lib.CY_DENSE_PROJ_VALU
    assert p["lds_bytes"] == 0 and p["w1_image_in_ws"] == 0 and p["bwd_launches"] == 6


def test_bad_arguments_return_error_codes_not_a_plan(lib):
    from cyhip import _lib
    plan = _lib.DenseProjPlan(*([-7] * 8))
    assert lib.cy_dense_proj_plan(256, 256, 1, 0.01, None) == ARG
    for cin, hid in ((0, 256), (-32, 256), (100, 256), (256, 0), (256, -1)):
        assert lib.cy_dense_proj_plan(cin, hid, 1, 0.01, plan) == SHAPE, (cin, hid)
    for dt in (3, -1, 17):
        assert lib.cy_dense_proj_plan(256, 256, dt, 0.01, plan) == DTYPE, dt
    assert [getattr(plan, f) for f, _ in plan._fields_] == [-7] * 8, "an error must not write a plan"
    assert lib.cy_dense_proj_plan(256, 256, 1, 0.01, plan) == 0 and plan.form == 2


@pytest.mark.parametrize("cin,hid", [(256, 256), (256, 128), (512, 256), (512, 128), (128, 256), (32, 128), (96, 64)])
def test_workspace_covers_the_planned_form(lib, cin, hid):
    from cyhip import _lib, ops
    for nb in (1, 6, 392, 2000):
        got = lib.cy_dense_proj_bwd_ws_bytes(nb, cin, hid)
        assert got > 0
        for dtype in (BF16, F16, F32):
            p = ops.dense_proj_plan(cin, hid, dtype)
            valu = min(nb, 256) * (hid * cin + hid) * 4   # one f32 slab of dW1 / db1 per workgroup
            # partials, job records (the cells of nb bins are fewer than 4 nb), the 16-bit image of W1
            mfma = PARTIALS + 4 * nb * REC + (hid * cin * 2 if p["w1_image_in_ws"] else 0)
            need = {_lib.CY_DENSE_PROJ_VALU: valu, _lib.CY_DENSE_PROJ_MFMA_REG: mfma,
                    _lib.CY_DENSE_PROJ_MFMA_STREAM: max(valu, mfma)}[p["form"]]  # (streamed: one after the other)
            assert got >= need, (nb, dtype, got, need)


def test_switch_sends_every_map_to_the_valu_kernels():
    """CY_DENSE_MFMA is read once per process: a fresh child"""
    code = ("import sys; sys.path.insert(0, %r); import torch; from cyhip import _lib, ops\n"
            "for c in (32, 64, 128, 256, 512):\n"
            "    for hid in (128, 256):\n"
            "        for dt in (torch.bfloat16, torch.float16):\n"
            "            p = ops.dense_proj_plan(c, hid, dt)\n"
            "            assert p['form'] == _lib.CY_DENSE_PROJ_VALU and p['lds_bytes'] == 0, (c, hid, p)\n"
            "print('valu everywhere')\n") % str(REPO / "contrast-you_amd")
    env = dict(os.environ, CY_DENSE_MFMA="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "valu everywhere" in r.stdout, r.stdout + r.stderr
