"""Host-side contract of the patch-wise IIC, PICA and JSD / entropy-prior losses (no kernel runs, no GPU): the patch
origins against the reference's `patch_generator` (recorded in tests/golden/patch_losses.npz), the C ABI's new entries
and their argument checks, the launch rule, the Python names and their signatures against the reference's
(tests/golden/patch_losses_signatures.txt), and the errors without a GPU tensor."""
import ctypes as C
import inspect

import pytest
import torch

import patch_losses_cases as pc
import patch_losses_fixture as fx

OK, ARG, SHAPE, WORKSPACE = 0, -1, -2, -5
P = 4096  # stands for a device pointer: every call below is refused before anything is launched or read

ENTRIES = {
    "cy_joint_patch_plan": (C.c_int, 8), "cy_joint_patch_ws_bytes": (C.c_size_t, 7), "cy_joint_patch_fwd": (C.c_int, 14),
    "cy_iid_patch_loss_ws_bytes": (C.c_size_t, 3), "cy_iid_patch_loss": (C.c_int, 14), "cy_joint_patch_bwd": (C.c_int, 14),
}


@pytest.fixture(scope="module")
def lib():
    from cyhip import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def npz(golden_dir):
    return fx.load(golden_dir)


def test_patch_origins_equal_the_reference(npz):
    from contrastyou.losses.discreteMI import patch_generator, patch_origins
    for L, p, s in fx.ORIGIN_CASES:
        want = [int(v) for v in npz[f"origins_{L}_{p}_{s}"]]
        assert patch_origins(L, p, s) == want, (L, p, s)
        ramp = torch.arange(L, dtype=torch.float32).view(1, 1, L, 1).expand(1, 1, L, 3)
        views = list(patch_generator(ramp, (p, 2), (s, 1)))
        assert sorted({int(v[0, 0, 0, 0]) for v in views}) == want
        assert all(v.shape[2] == min(p, L) and v.shape[3] == 2 for v in views)
        assert [int(v[0, 0, 0, 0]) for v in views[::len(views) // len(want)]] == want  # rows first
    assert patch_origins(224, 32, 16) == list(range(0, 192, 16)) + [192] and len(patch_origins(224, 32, 16)) == 13
    assert patch_origins(33, 16, 8) == [0, 8, 16, 17] and patch_origins(12, 16, 8) == [0]


def test_the_launch_rule_follows_the_origins(lib):
    from cyhip import _lib, ops
    for n, k, H, W, patch, pad in list(fx.PATCH_CASES.values()) + [pc.MULTI_TRIP, (16, 20, 224, 224, 32, 7)]:
        plan = ops.joint_patch_plan(n, H, W, k, pad, patch)
        oh, ow = pc.origins(H, patch), pc.origins(W, patch)
        assert (plan["nph"], plan["npw"], plan["P"]) == (len(oh), len(ow), len(oh) * len(ow))
        assert (plan["eh"], plan["ew"]) == (min(H, patch), min(W, patch))
        T = 2 * pad + 1
        assert plan["fwd_kernel"] == 1 and plan["grid_y"] == -(-T * T // 9) and plan["fwd_lds"] <= 150 * 1024
        assert plan["fwd_vec"] == plan["bwd_kernel"] == (k % 4 == 0)
        single = ops.joint_patch_plan(n, H, W, k, pad, patch, "per_displacement")
        assert single["fwd_kernel"] == 0 and single["grid_y"] == T * T
        for q in (plan, single):
            assert q["ws_bytes"] == (4 * q["P"] * T * T * k * k * q["nbx"] if q["nbx"] > 1 else 16)
    assert ops.joint_patch_plan(16, 224, 224, 20, 7, 32)["P"] == 169
    assert ops.joint_patch_plan(2, 24, 20, 4, 2, 16)["grid_y"] == 3  # case B: groups of 9, 9 and 7
    # a wide patch with large pad * k: the staged tile exceeds the LDS cap and the rule takes the fallback
    wide = ops.joint_patch_plan(1, 64, 64, 64, 7, 64)
    assert wide["staged_fits"] == 0 and wide["fwd_kernel"] == 0
    out = _lib.JointPatchPlan()
    assert lib.cy_joint_patch_plan(1, 64, 64, 64, 7, 64, 1, out) == SHAPE


def _fwd(lib, N=2, H=24, W=20, k=5, pad=1, patch=16, kernel=-1, ws_bytes=None, null=None):
    ptrs = [P, P, P]
    if null is not None and null < 3:
        ptrs[null] = None
    need = lib.cy_joint_patch_ws_bytes(N, H, W, k, pad, patch, kernel) if ws_bytes is None else ws_bytes
    return lib.cy_joint_patch_fwd(*ptrs, N, H, W, k, pad, patch, 0, kernel, None if null == 3 else P, need, None)


def _bwd(lib, N=2, H=24, W=20, k=5, pad=1, patch=16, null=None):
    ptrs = [P] * 6
    if null is not None:
        ptrs[null] = None
    return lib.cy_joint_patch_bwd(*ptrs, N, H, W, k, pad, patch, 0, None)


def _loss(lib, Pn=4, TT=9, k=5, mode=1, ws_bytes=None, null=None):
    ptrs = [P] * 5
    if null is not None and null < 5:
        ptrs[null] = None
    need = lib.cy_iid_patch_loss_ws_bytes(Pn, TT, k) if ws_bytes is None else ws_bytes
    return lib.cy_iid_patch_loss(*ptrs, Pn, TT, k, mode, 1.0, 1e-16, None if null == 5 else P, need, None)


def test_entries_are_declared_exported_and_typed(lib):
    from cyhip import _lib
    assert lib.cy_abi_version() == 19 == _lib.ABI_VERSION
    for name, (res, nargs) in ENTRIES.items():
        assert name in _lib.exported_names(), name
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs, (name, fn.restype, fn.argtypes)
        assert (name in _lib._INT_FUNCS) == (res is C.c_int), name


def test_every_rejection_has_its_status_before_any_launch(lib):
    from cyhip import _lib
    out = _lib.JointPatchPlan(*([-7] * 16))
    # NULL pointers
    for null in range(3):
        assert _fwd(lib, null=null) == ARG
    assert _fwd(lib, null=3) == WORKSPACE  # the workspace pointer
    for null in range(4):
        assert _bwd(lib, null=null) == ARG
    for null in range(2):
        assert _loss(lib, null=null) == ARG  # J, loss
    assert _loss(lib, null=2) == ARG  # losses
    assert _loss(lib, null=5) == WORKSPACE
    assert lib.cy_joint_patch_plan(2, 24, 20, 5, 1, 16, -1, None) == ARG
    # sizes
    for bad in (dict(N=0), dict(H=0), dict(W=-1), dict(kernel=2), dict(kernel=-2)):
        assert _fwd(lib, ws_bytes=1 << 30, **bad) == ARG, bad
    for bad in (dict(N=0), dict(H=0), dict(W=-1)):
        assert _bwd(lib, **bad) == ARG, bad
    for bad in (dict(Pn=0), dict(TT=0), dict(k=0)):
        assert _loss(lib, ws_bytes=1 << 30, **bad) == ARG, bad
    # shapes: k > 64, pad < 0, pad >= the smallest clipped patch extent, patch < 2
    for bad in (dict(k=65), dict(k=0), dict(pad=-1), dict(pad=16), dict(H=12, W=10, pad=10), dict(H=12, W=10, pad=11),
                dict(patch=1), dict(patch=0)):
        assert _fwd(lib, ws_bytes=1 << 30, **bad) == SHAPE, bad
        assert _bwd(lib, **bad) == SHAPE, bad
        a = dict(N=2, H=24, W=20, k=5, pad=1, patch=16)
        a.update(bad)
        assert lib.cy_joint_patch_ws_bytes(*a.values(), -1) == 0
        assert lib.cy_joint_patch_plan(*a.values(), -1, out) == SHAPE
    # 4225 patches * 225 displacements * 64 * 64 elements of J: past 32-bit indexing
    assert lib.cy_joint_patch_plan(1, 2112, 2112, 64, 7, 64, -1, out) == SHAPE
    assert [getattr(out, f) for f, _ in out._fields_] == [-7] * 16, "a refused query writes nothing"
    for bad in (dict(k=65), dict(mode=2), dict(mode=-1)):
        assert _loss(lib, ws_bytes=1 << 30, **bad) == SHAPE, bad
    # a short workspace
    for a in (dict(), dict(k=20, pad=7), dict(H=40, W=33, pad=3)):
        need = lib.cy_joint_patch_ws_bytes(a.get("N", 2), a.get("H", 24), a.get("W", 20), a.get("k", 5), a.get("pad", 1), 16, -1)
        assert need > 16 and _fwd(lib, ws_bytes=need - 1, **a) == WORKSPACE, a
    need = lib.cy_iid_patch_loss_ws_bytes(4, 9, 5)
    assert need == 4 * 4 * (4 * 9 * 25 + 2 * 9 * 5 + 9) and _loss(lib, ws_bytes=need - 1) == WORKSPACE
    assert lib.cy_iid_patch_loss_ws_bytes(4, 9, 65) == 0
    # NULL comes before the shape, the shape before the workspace
    assert _fwd(lib, k=65, ws_bytes=0, null=0) == ARG and _fwd(lib, k=65, ws_bytes=0) == SHAPE


def _names(fn):
    sig = inspect.signature(fn)
    return [("**" if p.kind is p.VAR_KEYWORD else "") + n for n, p in sig.parameters.items()
            if n != "self" and p.kind is not p.VAR_POSITIONAL]


def test_patch_names_and_signatures_equal_the_reference(golden_dir):
    import contrastyou.losses as losses
    import contrastyou.losses.discreteMI as mi
    want = dict(line.split(":") for line in (golden_dir / "patch_losses_signatures.txt").read_text().splitlines())
    got = {"IIDSegmentationSmallPathLoss": mi.IIDSegmentationSmallPathLoss.__init__,
           "IIDSegmentationSmallPathLoss.__call__": mi.IIDSegmentationSmallPathLoss.forward,
           "patch_generator": mi.patch_generator}
    for name, fn in got.items():
        assert _names(fn) == want[name].split(), name
    p = inspect.signature(mi.IIDSegmentationSmallPathLoss.__init__).parameters
    import sys
    assert (p["lamda"].default, p["padding"].default, p["eps"].default, p["patch_size"].default) == (
        1.0, 7, sys.float_info.epsilon, 32)
    assert {"IIDSegmentationSmallPathLoss", "patch_generator", "patch_origins"} <= set(mi.__all__)
    assert losses.IIDSegmentationSmallPathLoss is mi.IIDSegmentationSmallPathLoss
    crit = mi.IIDSegmentationSmallPathLoss()
    assert isinstance(crit, mi.IIDSegmentationLoss) and crit.symmetric is False
    assert crit._patch_size == (32, 32) and crit._step_size == (16, 16)
    assert repr(crit) == "IIDSegmentationSmallPathLoss with patch_size=(32, 32) and padding=7."
    with pytest.raises(RuntimeError):
        crit.get_joint_matrix()


def test_patch_cpu_tensors_are_refused():
    from contrastyou.losses.discreteMI import IIDSegmentationSmallPathLoss
    from cyhip import ops
    from cyhip.functions import IIDPatchFn
    x = torch.rand(1, 3, 12, 10).softmax(1)
    xr = x.permute(0, 2, 3, 1).contiguous()
    calls = [lambda: IIDSegmentationSmallPathLoss(padding=1, patch_size=16)(x, x),
             lambda: IIDPatchFn.apply(xr, xr, 1, 16, 1.0, 1e-16), lambda: ops.joint_patch_fwd(xr, xr, 1, 16, False),
             lambda: ops.iid_patch_loss(torch.rand(1, 9, 3, 3), 1, 1.0, 1e-16),
             lambda: ops.joint_patch_bwd(xr, xr, torch.rand(1, 9, 3, 3), torch.ones(1), 1, 16, False)]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---------------------------------------------------------------------------------------------- PICA, JSD, prior
PICA_ENTRIES = {
    "cy_pui_stats": (C.c_int, 6), "cy_pui_loss": (C.c_int, 9), "cy_rows_axpb": (C.c_int, 8),
    "cy_puiseg_ws_bytes": (C.c_size_t, 3), "cy_puiseg_loss": (C.c_int, 11), "cy_puiseg_balance_bwd": (C.c_int, 7),
    "cy_stream_sum_ws_bytes": (C.c_size_t, 1), "cy_jsd_fwd": (C.c_int, 11), "cy_jsd_bwd": (C.c_int, 10),
    "cy_entropy_prior_fwd": (C.c_int, 9), "cy_entropy_prior_bwd": (C.c_int, 8),
}


def test_pica_entries_are_declared_exported_and_typed(lib):
    from cyhip import _lib
    for name, (res, nargs) in PICA_ENTRIES.items():
        assert name in _lib.exported_names(), name
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == nargs, (name, fn.restype, fn.argtypes)


def test_pica_rejections_before_any_launch(lib):
    big = 1 << 20
    table = (C.c_void_p * 8)(*([P] * 8))
    hole = (C.c_void_p * 8)(P, None, P, P, P, P, P, P)
    # NULL pointers and counts
    assert lib.cy_pui_stats(None, P, P, 10, 5, None) == ARG and lib.cy_pui_stats(P, P, None, 10, 5, None) == ARG
    assert lib.cy_pui_stats(P, P, P, 0, 5, None) == ARG
    assert lib.cy_pui_loss(None, P, P, P, P, 10, 5, 2.0, None) == ARG
    assert lib.cy_pui_loss(P, P, P, P, None, 10, 5, 2.0, None) == ARG
    assert lib.cy_rows_axpb(P, None, P, P, P, 10, 5, None) == ARG and lib.cy_rows_axpb(P, P, P, P, P, 0, 5, None) == ARG
    assert lib.cy_puiseg_loss(None, P, P, P, 9, 5, 100, 2.0, P, big, None) == ARG
    assert lib.cy_puiseg_loss(P, P, P, P, 9, 5, 0, 2.0, P, big, None) == ARG
    assert lib.cy_puiseg_balance_bwd(P, None, P, 100, 5, 2.0, None) == ARG
    assert lib.cy_jsd_fwd(None, 2, P, 100, 5, 1, 1, 1e-16, P, big, None) == ARG
    assert lib.cy_jsd_fwd(table, 2, None, 100, 5, 1, 1, 1e-16, P, big, None) == ARG
    assert lib.cy_jsd_fwd(hole, 2, P, 100, 5, 1, 1, 1e-16, P, big, None) == ARG
    assert lib.cy_jsd_fwd(table, 2, P, 0, 5, 1, 1, 1e-16, P, big, None) == ARG
    assert lib.cy_jsd_fwd(table, 2, P, 100, 5, 1, 3, 1e-16, P, big, None) == ARG
    assert lib.cy_jsd_bwd(table, 2, None, table, 100, 5, 1, 1, 1e-16, None) == ARG
    assert lib.cy_jsd_bwd(table, 2, P, None, 100, 5, 1, 1, 1e-16, None) == ARG
    assert lib.cy_entropy_prior_fwd(None, P, P, 10, 5, 1e-16, P, big, None) == ARG
    assert lib.cy_entropy_prior_bwd(P, P, None, P, 10, 5, 1e-16, None) == ARG
    # shapes
    for K in (0, 65):
        assert lib.cy_pui_stats(P, P, P, 10, K, None) == SHAPE and lib.cy_pui_loss(P, P, P, P, P, 10, K, 2.0, None) == SHAPE
        assert lib.cy_rows_axpb(P, P, P, P, P, 10, K, None) == SHAPE
        assert lib.cy_puiseg_loss(P, P, P, P, 9, K, 100, 2.0, P, big, None) == SHAPE
        assert lib.cy_puiseg_balance_bwd(P, P, P, 100, K, 2.0, None) == SHAPE and lib.cy_puiseg_ws_bytes(100, 9, K) == 0
        assert lib.cy_jsd_fwd(table, 2, P, 100, K, 1, 1, 1e-16, P, big, None) == SHAPE
        assert lib.cy_jsd_bwd(table, 2, P, table, 100, K, 1, 1, 1e-16, None) == SHAPE
        assert lib.cy_entropy_prior_fwd(P, P, P, 10, K, 1e-16, P, big, None) == SHAPE
        assert lib.cy_entropy_prior_bwd(P, P, P, P, 10, K, 1e-16, None) == SHAPE
    for m in (1, 9):
        assert lib.cy_jsd_fwd(table, m, P, 100, 5, 1, 1, 1e-16, P, big, None) == SHAPE
        assert lib.cy_jsd_bwd(table, m, P, table, 100, 5, 1, 1, 1e-16, None) == SHAPE
    assert lib.cy_jsd_fwd(table, 2, P, 100, 5, 7, 1, 1e-16, P, big, None) == SHAPE  # R % S != 0
    # workspaces
    assert lib.cy_stream_sum_ws_bytes(0) == 0 and lib.cy_stream_sum_ws_bytes(257) == 16
    assert lib.cy_stream_sum_ws_bytes(1 << 30) == 8 * 1024
    assert lib.cy_puiseg_ws_bytes(286, 49, 5) == 8 * (2 + 2 * 49)
    assert lib.cy_puiseg_loss(P, P, P, P, 49, 5, 286, 2.0, P, 8 * 100 - 1, None) == WORKSPACE
    assert lib.cy_jsd_fwd(table, 2, P, 257, 5, 1, 1, 1e-16, P, 15, None) == WORKSPACE
    assert lib.cy_jsd_fwd(table, 2, P, 257, 5, 1, 2, 1e-16, None, 16, None) == WORKSPACE
    assert lib.cy_entropy_prior_fwd(P, None, P, 257, 5, 1e-16, P, 15, None) == WORKSPACE


def test_pica_names_and_signatures_equal_the_reference(golden_dir):
    import contrastyou.losses as losses
    from contrastyou.losses import kl, pica_loss
    want = dict(line.split(":") for line in (golden_dir / "patch_losses_signatures.txt").read_text().splitlines())
    got = {"PUILoss": pica_loss.PUILoss.__init__, "PUILoss.forward": pica_loss.PUILoss.forward,
           "PUISegLoss": pica_loss.PUISegLoss.__init__, "PUISegLoss.forward": pica_loss.PUISegLoss.forward,
           "JSD_div": kl.JSD_div.__init__, "JSD_div.forward": kl.JSD_div.forward,
           "EntropyPrior": kl.EntropyPrior.__init__, "EntropyPrior.forward": kl.EntropyPrior.forward}
    assert set(got) | {"IIDSegmentationSmallPathLoss", "IIDSegmentationSmallPathLoss.__call__",
                       "patch_generator"} == set(want)
    for name, fn in got.items():
        assert _names(fn) == want[name].split(), name
    assert inspect.signature(kl.JSD_div.forward).parameters["input_"].kind is inspect.Parameter.VAR_POSITIONAL
    assert inspect.signature(pica_loss.PUILoss.__init__).parameters["lamda"].default == 2.0
    p = inspect.signature(pica_loss.PUISegLoss.__init__).parameters
    assert (p["lamda"].default, p["padding"].default) == (2.0, 3)
    for cls in (kl.JSD_div, kl.EntropyPrior):
        p = inspect.signature(cls.__init__).parameters
        assert (p["reduction"].default, p["eps"].default) == ("mean", 1e-16)
    assert inspect.signature(kl.EntropyPrior.forward).parameters["prior"].default is None
    assert {"JSD_div", "EntropyPrior"} <= set(kl.__all__) and set(pica_loss.__all__) == {"PUILoss", "PUISegLoss"}
    assert losses.JSD_div is kl.JSD_div and losses.PUISegLoss is pica_loss.PUISegLoss
    assert issubclass(kl.EntropyPrior, kl.Entropy)
    with pytest.raises(AssertionError):
        kl.EntropyPrior(reduction="sum")
    with pytest.raises(AssertionError):
        kl.JSD_div(reduction="max")


def test_pica_cpu_tensors_are_refused():
    from contrastyou.losses import EntropyPrior, JSD_div, PUILoss, PUISegLoss
    from cyhip import ops
    x = torch.rand(2, 5, 6, 6).softmax(1)
    r = torch.rand(9, 5).softmax(1)
    calls = [lambda: PUILoss()(r, r), lambda: PUISegLoss()(x, x), lambda: JSD_div()(x, x), lambda: JSD_div()(r, r, r),
             lambda: EntropyPrior()(r), lambda: EntropyPrior()(r, torch.full((1, 5), 0.2)),
             lambda: ops.pui_loss(r, r, 2.0), lambda: ops.jsd_fwd([r, r], 9, 5, 1, "mean", 1e-16),
             lambda: ops.entropy_prior_fwd(r, None, 1e-16)]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
