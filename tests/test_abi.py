"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol
include/contrastyou_hip.h declares, and the product refuses to run without it / without a GPU.
No compute call is made here."""
import ctypes
import re
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
HEADER = REPO / "include" / "contrastyou_hip.h"


def header_symbols():
    text = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cy_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from cyhip import _lib
    lib = _lib.load()
    names = header_symbols()
    assert len(names) >= 40
    for n in names:
        assert hasattr(lib, n), f"{n} declared in the header but not exported"
    # and the binding declares a signature for each of them (no untyped calls)
    assert set(names) == set(_lib.exported_names())
    assert lib.cy_abi_version() == _lib.ABI_VERSION
    assert lib.cy_build_arch() == b"gfx950"


def test_conv_desc_layout_matches_header():
    from cyhip._lib import ConvDesc
    text = HEADER.read_text()
    body = re.search(r"typedef struct cy_conv_desc \{(.*?)\} cy_conv_desc;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl.startswith("int32_t"):
            fields += [f.strip() for f in decl[len("int32_t"):].split(",")]
    assert fields == [f[0] for f in ConvDesc._fields_]
    assert ctypes.sizeof(ConvDesc) == 4 * len(fields)


def test_argument_errors_are_reported_not_launched():
    from cyhip import _lib
    lib = _lib.load()
    # NULL pointers -> CY_ERR_ARG before any launch (safe without a GPU)
    assert lib.cy_conv3x3_pack_weights(None, None, None, 8, 8, 0, None) == -1
    assert lib.cy_bn_relu_apply(None, None, None, None, 10, 8, 0, 0, None) == -1
    with pytest.raises(_lib.HipKernelError):
        _lib.call("cy_sgemm", None, None, None, 4, 4, 4, 1.0, 0, None)
    a, b = ctypes.c_int(), ctypes.c_int()
    assert lib.cy_conv3x3_packed_dims(32, 1, ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) == (128, 64)


def test_product_refuses_cpu_tensors():
    import torch
    from contrastyou.arch import UNet
    net = UNet(input_dim=1, num_classes=4, max_channel=128)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.rand(1, 1, 32, 32))


def test_no_oracle_import_in_product():
    """the product tree must never import the oracle (it is test infrastructure)"""
    for p in (REPO / "contrast-you_amd").rglob("*.py"):
        src = p.read_text()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), p


def test_wgrad_plan_layout_matches_header():
    """cy_wgrad_plan (ABI v13: dma, blk_order appended) and its ctypes mirror name the same int32 fields in order"""
    from cyhip._lib import WgradPlan
    text = HEADER.read_text()
    body = re.search(r"typedef struct cy_wgrad_plan \{(.*?)\} cy_wgrad_plan;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            assert decl.startswith("int32_t "), decl
            fields += [f.strip() for f in decl[len("int32_t "):].split(",")]
    assert fields == [n for n, _ in WgradPlan._fields_]
    assert fields[-2:] == ["dma", "blk_order"]
    assert ctypes.sizeof(WgradPlan) == 4 * len(fields)


def _check_plan_layout(struct, mirror):
    from cyhip import _lib
    cls = getattr(_lib, mirror)
    text = HEADER.read_text()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            assert decl.startswith("int32_t "), decl
            fields += [f.strip() for f in decl[len("int32_t "):].split(",")]
    assert fields == [n for n, _ in cls._fields_]
    assert ctypes.sizeof(cls) == 4 * len(fields)
    return fields


@pytest.mark.parametrize("struct,mirror", [("cy_head_plan", "HeadPlan"), ("cy_cluster_plan", "ClusterPlan")])
def test_head_plan_layouts_match_header(struct, mirror):
    """cy_head_plan / cy_cluster_plan (ABI v16) and their ctypes mirrors name the same int32 fields in order"""
    from cyhip import _lib
    _check_plan_layout(struct, mirror)
    assert _lib.ABI_VERSION == 18


@pytest.mark.parametrize("struct,mirror", [("cy_joint_plan_t", "JointPlan"),
                                           ("cy_group_softmax_plan_t", "GroupSoftmaxPlan")])
def test_mi_plan_layouts_match_header(struct, mirror):
    """cy_joint_plan_t / cy_group_softmax_plan_t (ABI v17) and their ctypes mirrors name the same int32 fields in
    order; the plan entry points are exported and typed"""
    from cyhip import _lib
    fields = _check_plan_layout(struct, mirror)
    assert fields[0] in ("fwd_kernel", "fwd_rows")
    assert _lib.ABI_VERSION == 18 and _lib.load().cy_abi_version() == 18
    assert {"cy_joint_plan", "cy_group_softmax_plan"} <= set(_lib.exported_names()) & set(header_symbols())


def test_norm_act_plan_layout_matches_header():
    """cy_norm_act_plan_t (ABI v18) and its ctypes mirror name the same int32 fields in order; the kinds of the binding
    are the header's enum, in order; the plan entry point is exported and typed"""
    from cyhip import _lib
    fields = _check_plan_layout("cy_norm_act_plan_t", "NormActPlan")
    assert fields[0] == "status" and fields[-1] == "chain"
    assert _lib.ABI_VERSION == 18 and _lib.load().cy_abi_version() == 18
    assert "cy_norm_act_plan" in set(_lib.exported_names()) & set(header_symbols())
    enum = re.search(r"enum \{\s*(CY_NA_APPLY = 0.*?)\};", HEADER.read_text(), flags=re.S).group(1)
    names = [(m.group(1).lower(), int(m.group(2))) for m in re.finditer(r"CY_NA_([A-Z0-9_]+) = (\d+)", enum)]
    assert names == [(k, i) for i, k in enumerate(_lib.NORM_ACT_KINDS)]


def test_loading_the_library_first_leaves_one_hip_runtime():
    """a process that loads the library before it imports torch (__graft_entry__.build() followed by smoke() does) must
    not end up with two HIP runtimes mapped -- the system's and the copy in torch's wheel: launches on torch's streams
    then fail"""
    import subprocess
    import sys
    code = ("import sys; sys.path[:0] = %r\n"
            "from cyhip import _lib; _lib.load(); import torch\n"
            "print(len({l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l}))\n"
            % [str(REPO), str(REPO / "contrast-you_amd")])
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout.strip().splitlines()[-1]) == 1, r.stdout
