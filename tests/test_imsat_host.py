"""Host-side contract of the IMSAT family (no kernel runs, no GPU): the C ABI's new entries and their argument checks,
the workspace formula, the Python names and their signatures against the reference's
(tests/golden/imsat_signatures.txt, written by tests/golden/gen_goldens_imsat.py), the errors without a GPU tensor, and
the scope limit: the two factories and the tiny hook that existing tests pin to NotImplementedError still raise."""
import ctypes as C
import inspect

import pytest
import torch

ENTRIES = {
    "cy_imsat_ws_bytes": (C.c_size_t, 2), "cy_imsat_fwd": (C.c_int, 10), "cy_imsat_bwd": (C.c_int, 8),
    "cy_imsat_pair_ws_bytes": (C.c_size_t, 2), "cy_imsat_pair_fwd": (C.c_int, 11), "cy_imsat_pair_bwd": (C.c_int, 10),
    "cy_softmax_imsat_ws_bytes": (C.c_size_t, 2), "cy_softmax_imsat_fwd": (C.c_int, 10),
    "cy_softmax_imsat_bwd": (C.c_int, 8), "cy_imsat_plan": (C.c_int, 5),
}
OK, ARG, SHAPE, WORKSPACE = 0, -1, -2, -5
P = 4096  # stands for a device pointer: every call below is refused before anything is launched or read


@pytest.fixture(scope="module")
def lib():
    from cyhip import _lib
    return _lib.load()


def test_entries_are_declared_exported_and_typed(lib):
    from cyhip import _lib
    assert lib.cy_abi_version() == 19 == _lib.ABI_VERSION
    for name, (res, nargs) in ENTRIES.items():
        assert name in _lib.exported_names(), name
        fn = getattr(lib, name)  # exported by the library
        assert fn.restype is res and len(fn.argtypes) == nargs, (name, fn.restype, fn.argtypes)
        assert (name in _lib._INT_FUNCS) == (res is C.c_int), name
    assert lib.cy_imsat_fwd.argtypes[4:7] == [C.c_long, C.c_int, C.c_float]
    assert lib.cy_imsat_plan.argtypes == [C.c_int, C.c_long, C.c_int, C.c_int, C.POINTER(_lib.ImsatPlan)]
    assert tuple(f for f, _ in _lib.ImsatPlan._fields_) == ("vec", "kt", "threads", "tile", "fwd_grid", "fwd_trips",
                                                            "bwd_grid", "bwd_trips", "slots")
    assert (_lib.CY_IMSAT_ROWS, _lib.CY_IMSAT_PAIR, _lib.CY_IMSAT_LOGITS) == (0, 1, 2)


def _fwd(lib, group, R, K, ws_bytes=None, null=None):
    """the forward of a group on stand-in pointers; `null`: index of the pointer argument passed as NULL"""
    query = getattr(lib, f"cy_{group}_ws_bytes")
    nbytes = query(R, K) if ws_bytes is None else ws_bytes
    ptrs = [P] * (5 if group == "imsat_pair" else 4)
    if null is not None and null < len(ptrs):
        ptrs[null] = None
    ws = None if null == len(ptrs) else P
    return getattr(lib, f"cy_{group}_fwd")(*ptrs, R, K, 1e-8, ws, nbytes, None)


def _bwd(lib, group, R, K, null=None):
    ptrs = [P] * (6 if group == "imsat_pair" else 4)
    if null is not None:
        ptrs[null] = None
    return getattr(lib, f"cy_{group}_bwd")(*ptrs, R, K, 1e-8, None)


@pytest.mark.parametrize("group", ["imsat", "imsat_pair", "softmax_imsat"])
def test_every_rejection_has_its_status_before_any_launch(lib, group):
    kmax = 16 if group == "softmax_imsat" else 64
    nfwd, nbwd = (5, 6) if group == "imsat_pair" else (4, 4)
    for null in range(nfwd + 1):  # every pointer, the workspace last
        assert _fwd(lib, group, 10, 3, null=null) == ARG, (group, null)
    for null in range(nbwd):
        assert _bwd(lib, group, 10, 3, null=null) == ARG, (group, null)
    for R in (0, -1):
        assert _fwd(lib, group, R, 3, ws_bytes=1 << 20) == ARG and _bwd(lib, group, R, 3) == ARG
    for K in (1, 0, kmax + 1, 65):
        assert _fwd(lib, group, 10, K, ws_bytes=1 << 20) == SHAPE, (group, K)
        assert _bwd(lib, group, 10, K) == SHAPE, (group, K)
        assert getattr(lib, f"cy_{group}_ws_bytes")(10, K) == 0
    if group == "softmax_imsat":
        assert _fwd(lib, group, 10, 17, ws_bytes=1 << 20) == SHAPE and _bwd(lib, group, 10, 17) == SHAPE
    for R, K in ((10, 3), (257, kmax), (100000, 2)):
        need = getattr(lib, f"cy_{group}_ws_bytes")(R, K)
        assert need > 0
        assert _fwd(lib, group, R, K, ws_bytes=need - 1) == WORKSPACE, (group, R, K)
    # NULL comes before the shape, the shape before the workspace
    assert _fwd(lib, group, 10, 1, ws_bytes=0, null=0) == ARG and _fwd(lib, group, 10, 1, ws_bytes=0) == SHAPE


def test_plan_rejections(lib):
    from cyhip import _lib, ops
    out = _lib.ImsatPlan(*([-7] * 9))

    def values():
        return [getattr(out, f) for f, _ in out._fields_]
    assert lib.cy_imsat_plan(0, 10, 3, 16, None) == ARG
    for form, R, K, align in ((3, 10, 3, 16), (-1, 10, 3, 16), (0, 0, 3, 16), (0, 10, 3, 0)):
        assert lib.cy_imsat_plan(form, R, K, align, out) == ARG
    for form, K in ((0, 1), (0, 65), (1, 65), (2, 17), (2, 1)):
        assert lib.cy_imsat_plan(form, 10, K, 16, out) == SHAPE
    # K == 4 logits are read 16 bytes at a time in every form
    for align in (4, 8):
        assert lib.cy_imsat_plan(2, 10, 4, align, out) == ARG
        assert lib.cy_softmax_imsat_fwd(P + align, P, P, P, 10, 4, 1e-8, P, 1 << 20, None) == ARG
        assert lib.cy_softmax_imsat_bwd(P, P, P, P + align, 10, 4, 1e-8, None) == ARG
    assert values() == [-7] * 9, "a refused query writes nothing"
    assert lib.cy_imsat_plan(2, 10, 4, 16, out) == OK and values() == [4, 4, 256, 256, 1, 1, 1, 1, 5]
    assert (out.vec, out.kt, out.threads, out.tile, out.slots) == (4, 4, 256, 256, 5)
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_SHAPE"):
        ops.imsat_plan("rows", 10, 65)


@pytest.mark.parametrize("K", [2, 3, 20, 63, 64])
@pytest.mark.parametrize("R", [1, 256, 257, 1 << 31])
def test_workspace_formula(lib, R, K):
    """as include/contrastyou_hip.h states it"""
    blocks = min(1024, -(-(R * K) // (4 * K * (256 // K))))
    assert lib.cy_imsat_ws_bytes(R, K) == 8 * (1 + K) * blocks
    assert lib.cy_imsat_pair_ws_bytes(R, K) == 8 * (3 + 2 * K) * blocks
    if K <= 16:
        assert lib.cy_softmax_imsat_ws_bytes(R, K) == 8 * (1 + K) * min(1024, -(-R // 256))


def _names(fn):
    sig = inspect.signature(fn)
    return [("**" if p.kind is p.VAR_KEYWORD else "") + n for n, p in sig.parameters.items() if n != "self"]


def test_names_and_signatures_equal_the_reference(golden_dir):
    import contrastyou.losses.discreteMI as mi
    import semi_seg.hooks as hooks
    from contrastyou.losses.discreteMI import IMSATDynamicWeight, IMSATLoss, imsat_loss, imsat_with_entropy
    from semi_seg.hooks import DiscreteIMSATTrainHook, IMSATTrainHook
    want = dict(line.split(": ") for line in (golden_dir / "imsat_signatures.txt").read_text().splitlines())
    got = {"imsat_loss": imsat_loss, "imsat_with_entropy": imsat_with_entropy, "IMSATLoss": IMSATLoss.__init__,
           "IMSATLoss.forward": IMSATLoss.forward, "IMSATDynamicWeight": IMSATDynamicWeight.__init__,
           "IMSATDynamicWeight.forward": IMSATDynamicWeight.forward, "IMSATTrainHook": IMSATTrainHook.__init__,
           "DiscreteIMSATTrainHook": DiscreteIMSATTrainHook.__init__}
    assert set(got) == set(want)
    for name, fn in got.items():
        assert _names(fn) == want[name].split(), name
    assert {"IMSATLoss", "IMSATDynamicWeight", "imsat_loss", "imsat_with_entropy"} <= set(mi.__all__)
    assert hooks.IMSATTrainHook is IMSATTrainHook and hooks.DiscreteIMSATTrainHook is DiscreteIMSATTrainHook
    # defaults and keyword-only hooks, as the reference writes them
    assert inspect.signature(imsat_loss).parameters["lamda"].default == 1.0
    assert inspect.signature(IMSATLoss.forward).parameters["x_tf_out"].default is None
    assert inspect.signature(IMSATDynamicWeight.__init__).parameters["use_dynamic"].default is True
    p = inspect.signature(IMSATTrainHook.__init__).parameters
    assert (p["hook_name"].default, p["weight"].default) == ("imsat", 0.1)
    p = inspect.signature(DiscreteIMSATTrainHook.__init__).parameters
    assert all(q.kind is q.KEYWORD_ONLY for n, q in p.items() if n != "self")
    assert (p["weight"].default, p["num_clusters"].default, p["num_subheads"].default) == (1.0, 20, 5)
    assert p["cons_weight"].default is inspect.Parameter.empty


def test_cpu_tensors_are_refused():
    from contrastyou.losses.discreteMI import IMSATDynamicWeight, IMSATLoss, imsat_loss, imsat_with_entropy
    from cyhip.functions import IMSATFn, IMSATPairFn, SoftmaxIMSATFn, softmax_imsat
    from cyhip import ops
    p = torch.rand(7, 5).softmax(1)
    z = torch.randn(2, 4, 3, 3)
    calls = [lambda: imsat_loss(p), lambda: imsat_with_entropy(p), lambda: IMSATLoss()(p), lambda: IMSATLoss()(p, p),
             lambda: IMSATDynamicWeight()(p), lambda: IMSATFn.apply(p), lambda: IMSATPairFn.apply(p, p),
             lambda: SoftmaxIMSATFn.apply(z), lambda: softmax_imsat(z), lambda: softmax_imsat(torch.randn(2, 20, 3, 3)),
             lambda: ops.imsat_fwd(p), lambda: ops.imsat_pair_fwd(p, p), lambda: ops.softmax_imsat_fwd(z)]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_dynamic_weight_buffer():
    from contrastyou.losses.discreteMI import IMSATDynamicWeight, IMSATLoss
    crit = IMSATDynamicWeight(lamda=1.5)
    assert list(crit.state_dict()) == ["dynamic_weight"]
    assert float(crit.state_dict()["dynamic_weight"]) == 1.5 and crit.use_dynamic_weight is True
    assert isinstance(crit, IMSATLoss) and crit.lamda == 1.5
    assert list(IMSATLoss().state_dict()) == []
    twin = IMSATDynamicWeight()
    twin.load_state_dict(crit.state_dict())
    assert float(twin.dynamic_weight) == 1.5


def test_intermediate_hook_refuses_an_encoder_feature():
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from semi_seg.hooks import DiscreteIMSATTrainHook
    for name in UNet.encoder_names:
        with pytest.raises(ValueError, match="decoder feature"):
            DiscreteIMSATTrainHook(name="imsat_mid", model=None, feature_name=name, cons_weight=0.1)
    assert "imsat_mid" not in type(TrainerHook).names  # nothing was registered on the way


def test_the_pinned_stubs_still_raise():
    """the scope limit, next to the feature: pointing these at the new hook classes edits the two test files that pin
    them (tests/test_semi_baselines_host.py, tests/test_cc_host.py)"""
    import semi_seg.hooks as hooks
    from semi_seg.hooks.ccblock import _IMSATHook
    with pytest.raises(NotImplementedError, match="create_imsat_hook"):
        hooks.create_imsat_hook(weight=0.1)
    with pytest.raises(NotImplementedError, match="create_intermediate_imsat_hook"):
        hooks.create_intermediate_imsat_hook(feature_name="Up_conv2", weight=0.1, num_clusters=10, cons_weight=0.1,
                                             model=None)
    with pytest.raises(NotImplementedError, match="IMSAT"):
        _IMSATHook(weight=0.1)
