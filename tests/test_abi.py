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


def _check_plan_layout(struct, mirror):
    """the test's own reading of an all-int32 struct body, independent of the parser that derives the mirror"""
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
    assert all(t is ctypes.c_int32 for _, t in cls._fields_)
    assert ctypes.sizeof(cls) == 4 * len(fields)
    return fields


def test_conv_desc_layout_matches_header():
    _check_plan_layout("cy_conv_desc", "ConvDesc")


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
    fields = _check_plan_layout("cy_wgrad_plan", "WgradPlan")
    assert fields[-2:] == ["dma", "blk_order"]


@pytest.mark.parametrize("struct,mirror", [("cy_head_plan", "HeadPlan"), ("cy_cluster_plan", "ClusterPlan")])
def test_head_plan_layouts_match_header(struct, mirror):
    """cy_head_plan / cy_cluster_plan (ABI v16) and their ctypes mirrors name the same int32 fields in order"""
    from cyhip import _lib
    _check_plan_layout(struct, mirror)
    assert _lib.ABI_VERSION == _lib.load().cy_abi_version()


@pytest.mark.parametrize("struct,mirror", [("cy_joint_plan_t", "JointPlan"),
                                           ("cy_group_softmax_plan_t", "GroupSoftmaxPlan")])
def test_mi_plan_layouts_match_header(struct, mirror):
    """cy_joint_plan_t / cy_group_softmax_plan_t (ABI v17) and their ctypes mirrors name the same int32 fields in
    order; the plan entry points are exported and typed"""
    from cyhip import _lib
    fields = _check_plan_layout(struct, mirror)
    assert fields[0] in ("fwd_kernel", "fwd_rows")
    assert _lib.ABI_VERSION == _lib.load().cy_abi_version()
    assert {"cy_joint_plan", "cy_group_softmax_plan"} <= set(_lib.exported_names()) & set(header_symbols())


def test_norm_act_plan_layout_matches_header():
    """cy_norm_act_plan_t (ABI v18) and its ctypes mirror name the same int32 fields in order; the kinds of the binding
    are the header's enum, in order; the plan entry point is exported and typed"""
    from cyhip import _lib
    fields = _check_plan_layout("cy_norm_act_plan_t", "NormActPlan")
    assert fields[0] == "status" and fields[-1] == "chain"
    assert _lib.ABI_VERSION == _lib.load().cy_abi_version()
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


# ---- the binding is derived from the header: what the derivation must come to is written out here by hand ----------

def test_abi_version_has_one_source():
    """the number is written once in the header; the library returns the macro and the binding reads it.  This is the
    one place a test pins it: an ABI bump edits the header's define and this line"""
    from cyhip import _lib
    macro = int(re.search(r"^#define CY_ABI_VERSION (\d+)$", HEADER.read_text(), flags=re.M).group(1))
    assert macro == 19
    assert _lib.load().cy_abi_version() == 19
    assert _lib.ABI_VERSION == 19


def test_pinned_signatures():
    """ten signatures written out by hand; between them they use every row of the binding's type map"""
    from ctypes import (POINTER, c_char_p, c_double, c_float, c_int, c_long, c_longlong, c_size_t, c_ulonglong,
                        c_void_p)
    from cyhip import _lib
    P, PCD, PML = c_void_p, POINTER(_lib.ConvDesc), POINTER(_lib.MatLayout)
    pinned = {
        "cy_abi_version": (c_int, []),
        "cy_build_arch": (c_char_p, []),
        "cy_stream_capture_id": (c_ulonglong, [P]),
        "cy_conv3x3_packed_elems": (c_longlong, [c_int, c_int, c_int]),
        "cy_conv3x3_fwd": (c_int, [PCD, P, P, P, P, P, P, P, P, P, c_size_t, P]),
        "cy_bn_finalize": (c_int, [P, c_int, c_int, c_double, P, P, P, P, c_float, c_float, c_int, c_int, P, P, P, P,
                                   P]),
        "cy_gemm_strided": (c_int, [P, PML, P, PML, P, PML, P, c_int, c_int, c_int, c_int, c_int, c_float, c_int,
                                    c_int, P, c_size_t, P]),
        "cy_conv3x3_dgrad_bn": (c_int, [PCD, P, POINTER(_lib.BnBwdIn), P, P, P, P, c_size_t, P]),
        "cy_head1x1_plan": (c_int, [c_long, c_int, c_int, c_int, c_int, POINTER(_lib.HeadPlan)]),
        # the one override: the table of items travels as a tensor's data_ptr(), so argument 0 is not POINTER(PackItem)
        "cy_conv3x3_pack_weights_batched": (c_int, [P, c_int, c_longlong, P, P, c_int, P]),
    }
    lib = _lib.load()
    for name, (res, args) in pinned.items():
        assert _lib._SIGS[name][0] is res, name
        got = _lib._SIGS[name][1]
        assert len(got) == len(args) and all(a is b for a, b in zip(got, args)), (name, got)
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == args, name


def test_pinned_layouts():
    """four mixed-type structs written out by hand: field names, ctypes and order, and the size the C compiler gives
    them on x86-64 (LP64)"""
    from ctypes import POINTER, c_double, c_float, c_int32, c_long, c_longlong, c_void_p
    from cyhip import _lib
    P = c_void_p
    pinned = {
        "BnFold": (56, [("acc", P), ("R", c_int32), ("C", c_int32), ("gamma", P), ("beta", P), ("count", c_double),
                        ("eps", c_float), ("reserved", c_int32), ("coef", P)]),
        "PackItem": (72, [("w", P), ("off_f", c_longlong), ("off_d", c_longlong), ("first", c_longlong),
                          ("Cout", c_int32), ("Cin", c_int32), ("co_pad", c_int32), ("ci_pad", c_int32),
                          ("ci_pad2", c_int32), ("co_pad2", c_int32), ("off_ff", c_longlong), ("off_fd", c_longlong)]),
        "BnBwdIn": (64, [("y", P), ("coef", P), ("acc", POINTER(_lib.BnAcc)), ("count", c_double),
                         ("batch_stats", c_int32), ("accumulate", c_int32), ("dgamma", P), ("dbeta", P), ("dy", P)]),
        "MatLayout": (32, [("rs", c_long), ("cs", c_long), ("s1", c_long), ("s2", c_long)]),
    }
    for mirror, (size, fields) in pinned.items():
        cls = getattr(_lib, mirror)
        got = list(cls._fields_)
        assert [n for n, _ in got] == [n for n, _ in fields], mirror
        assert all(a[1] is b[1] for a, b in zip(got, fields)), (mirror, got)
        assert ctypes.sizeof(cls) == size, mirror


MIRRORS = {"cy_conv_desc": "ConvDesc", "cy_pack_item": "PackItem", "cy_conv_plan": "ConvPlan",
           "cy_wgrad_plan": "WgradPlan", "cy_head_plan": "HeadPlan", "cy_cluster_plan": "ClusterPlan",
           "cy_joint_plan_t": "JointPlan", "cy_group_softmax_plan_t": "GroupSoftmaxPlan",
           "cy_norm_act_plan_t": "NormActPlan", "cy_wgrad_reduce_entry": "WgradReduceEntry", "cy_bn_acc": "BnAcc",
           "cy_bn_fold": "BnFold", "cy_bn_bwd_in": "BnBwdIn", "cy_bn_dz_out": "BnDzOut", "cy_bn_run_item": "BnRunItem",
           "cy_mat_layout": "MatLayout",
           "cy_dense_proj_plan_t": "DenseProjPlan", "cy_joint_patch_plan_t": "JointPatchPlan",
           "cy_pixel_mlp_plan_t": "PixelMlpPlan", "cy_imsat_plan_t": "ImsatPlan", "cy_mix_plan_t": "MixPlan",
           "cy_prior_plan_t": "PriorPlan", "cy_teacher_plan_t": "TeacherPlan", "cy_optim_plan_t": "OptimPlan",
           "cy_wide_reg_plan_t": "WideRegPlan", "cy_slic_plan_t": "SlicPlan", "cy_aug_plan_t": "AugPlan"}

# the eleven plan structs of ABI v19: (struct, the ops function that reads it, one accepted call, the documented extras)
FAMILY_PLANS = [
    ("cy_dense_proj_plan_t", "dense_proj_plan", (64, 128), ()),
    ("cy_joint_patch_plan_t", "joint_patch_plan", (2, 24, 20, 5, 1, 16), ("ws_bytes",)),
    ("cy_pixel_mlp_plan_t", "pixel_mlp_plan", (100, 32, 64, 16), ()),
    ("cy_imsat_plan_t", "imsat_plan", ("rows", 100, 10), ("ws_bytes",)),
    ("cy_mix_plan_t", "mix_plan", ("mixkl", 2, 100, 4), ()),
    ("cy_prior_plan_t", "prior_plan", ("dae", 4, 1, 100), ()),
    ("cy_teacher_plan_t", "teacher_plan", ("gathermse", 100, 4), ()),
    ("cy_optim_plan_t", "optim_plan", ("sgd", 1000), ()),
    ("cy_wide_reg_plan_t", "wide_reg_plan", ("entropy", 286, 20), ()),
    ("cy_slic_plan_t", "slic_plan", (2, 64, 64, 16), ()),
    ("cy_aug_plan_t", "augment_plan", (4, 32, 32), ()),
]


@pytest.mark.parametrize("struct,fn,args,extras", FAMILY_PLANS, ids=[f[0] for f in FAMILY_PLANS])
def test_family_plan_layouts_match_header_and_ops(struct, fn, args, extras):
    """the plan structs of ABI v19 and their ctypes mirrors name the same int32 fields in order, and the dict the
    matching ops function answers has exactly those fields as its leading keys, in order"""
    from cyhip import _lib, ops
    fields = _check_plan_layout(struct, MIRRORS[struct])
    plan = getattr(ops, fn)(*args)
    assert list(plan) == fields + list(extras)
    assert all(type(v) is int for v in plan.values())
    assert plan.get("status", 0) == 0
    assert _lib.ABI_VERSION == _lib.load().cy_abi_version()


def test_header_has_no_array_plans():
    """a plan query answers through a struct of the header: no int32 array named `plan`, no index macros"""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert not re.search(r"int32_t\s*\*\s*plan\b", text)
    assert not re.search(r"CY_\w+_PLAN_LEN\b", text)
    assert not re.search(r"#define\s+CY_(SLIC|AUG)_PLAN_", text)
    for name, args in re.findall(r"\b(cy_\w+_plan)\s*\(([^()]*)\)\s*;", text):
        assert re.search(r"\bcy_\w+\s*\*\s*\w+\s*$", args), (name, args)  # the last parameter: a struct of the header


def test_every_struct_has_a_mirror_and_every_struct_pointer_resolves_to_it():
    from cyhip import _lib
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = re.findall(r"typedef struct[^{;]*\{[^}]*\}\s*(\w+)\s*;", text)
    assert len(declared) == 27 and sorted(declared) == sorted(MIRRORS)
    for struct, mirror in MIRRORS.items():
        assert issubclass(getattr(_lib, mirror), ctypes.Structure), mirror
    seen = set()
    for name, args in re.findall(r"\b(cy_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        for i, arg in enumerate(args.split(",")):
            m = re.match(r"\s*(?:const\s+)?(cy_\w+)\s*\*", arg)
            if m and (name, i) != ("cy_conv3x3_pack_weights_batched", 0):
                assert _lib._SIGS[name][1][i] is ctypes.POINTER(getattr(_lib, MIRRORS[m.group(1)])), (name, i)
                seen.add(m.group(1))
    # cy_pack_item travels as a device table (the override), cy_bn_acc also inside two structs
    assert seen == set(MIRRORS) - {"cy_pack_item"}


def test_binding_refuses_what_it_does_not_know(tmp_path):
    from cyhip import _lib
    with pytest.raises(TypeError, match=r"cy_x.*'short'"):
        _lib.parse_header("int cy_x(short a);")
    with pytest.raises(TypeError, match=r"cy_y.*'void\*'"):
        _lib.parse_header("void* cy_y(int a);")
    missing = tmp_path / "include" / "contrastyou_hip.h"
    with pytest.raises(_lib.HipExtensionMissing, match=re.escape(str(missing))):
        _lib.read_header(missing)
