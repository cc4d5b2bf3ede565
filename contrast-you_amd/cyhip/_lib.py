"""ctypes binding of libcontrastyou_hip.so, derived at import from the C ABI's header include/contrastyou_hip.h.

The header is the only place a signature, a struct, a constant or the ABI number is written: this module reads it once
and builds the struct mirrors, the table of signatures and the constants from it.
The library is the only compute backend of this package: there is no CPU or eager
fallback.  If it is missing, or a call is made without a GPU tensor, the error is loud.
"""
from __future__ import annotations

import ctypes as C
import re
from ctypes import POINTER, c_char_p, c_int, c_void_p
from pathlib import Path

_ERRORS = {-1: "CY_ERR_ARG (bad/NULL argument)", -2: "CY_ERR_SHAPE (unsupported shape)",
           -3: "CY_ERR_DTYPE (unsupported dtype)", -4: "CY_ERR_LAUNCH (HIP launch failed)",
           -5: "CY_ERR_WORKSPACE (workspace too small)"}

LIB_PATH = Path(__file__).resolve().parent.parent / "lib" / "libcontrastyou_hip.so"
HEADER_PATH = Path(__file__).resolve().parents[2] / "include" / "contrastyou_hip.h"


class HipExtensionMissing(RuntimeError):
    pass


class HipKernelError(RuntimeError):
    pass


# ---- the header -> ctypes.  Not a C parser: it knows the four forms this header is written in (prototypes
# `ret cy_name(args);`, `typedef struct [tag] { ... } name;`, `#define CY_X <integer or (-integer)>` and the enum of
# CY_NA_* = n) and refuses a type it has no row for.

# by value; a `const` is dropped.  Pointers: to a struct of the header POINTER(mirror), to anything else c_void_p;
# `const char*` is known as a return type only.
_SCALARS = {"int": c_int, "int32_t": C.c_int32, "long": C.c_long, "long long": C.c_longlong,
            "unsigned long long": C.c_ulonglong, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}


def read_header(path: Path = HEADER_PATH) -> str:
    if not Path(path).exists():
        raise HipExtensionMissing(f"{path} not found: the binding of libcontrastyou_hip.so is derived from it")
    return Path(path).read_text()


def _decl(decl: str):
    """'const float* w' -> ('float*', 'w')"""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    return " ".join(words[:-1]).replace(" *", "*"), words[-1]


def _ctype(ctype: str, structs: dict, where: str, ret: bool = False):
    if ret and ctype == "char*":
        return c_char_p
    if ctype.endswith("*") and not ret:
        return POINTER(structs[ctype[:-1]]) if ctype[:-1] in structs else c_void_p
    if ctype not in _SCALARS:
        raise TypeError(f"{where}: the C type {ctype!r} is not in the binding's type map (cyhip/_lib.py)")
    return _SCALARS[ctype]


def parse_header(text: str):
    """-> (constants {name: int}, the CY_NA_* kinds in value order, struct mirrors {C name: Structure},
    signatures {entry point: (restype, [argtypes])})"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    consts = {n: int(v) for n, v in re.findall(r"^#define[ \t]+(CY_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, flags=re.M)}
    kinds = sorted((int(v), n.lower()) for n, v in re.findall(r"\bCY_NA_(\w+)\s*=\s*(\d+)", text))
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = []
        for decl in filter(None, map(str.strip, body.split(";"))):
            first, *more = decl.split(",")  # `int32_t a, b, c`
            ctype, field = _decl(first)
            fields += [(f.strip(), _ctype(ctype, structs, name)) for f in (field, *more)]
        structs[name] = type(name, (C.Structure,), {"_fields_": fields, "__doc__": f"mirror of {name}"})
    sigs = {}
    for ret, name, args in re.findall(r"([\w \t*]+?)\s*\b(cy_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [] if args.strip() == "void" else [_decl(a)[0] for a in args.split(",")]
        sigs[name] = (_ctype(_decl(f"{ret} {name}")[0], structs, name, ret=True),
                      [_ctype(t, structs, name) for t in params])
    return consts, tuple(k for _, k in kinds), structs, sigs


# _SIGS: name -> (restype, argtypes).  restype c_int functions are status-checked.
_CONSTS, NORM_ACT_KINDS, _STRUCTS, _SIGS = parse_header(read_header())
globals().update(_CONSTS)  # CY_F32, CY_BF16, CY_F16, CY_SRC_*, CY_CONV_KERNEL_*, CY_WGRAD_REDUCE_*, ...
ABI_VERSION = _CONSTS["CY_ABI_VERSION"]
# the one signature kept by hand: ops.pack_weights_batched passes the table of items as a tensor's data_ptr(), an
# int, which POINTER(PackItem) would refuse
_SIGS["cy_conv3x3_pack_weights_batched"][1][0] = c_void_p

_struct = _STRUCTS.__getitem__
ConvDesc = _struct("cy_conv_desc")
PackItem = _struct("cy_pack_item")
ConvPlan = _struct("cy_conv_plan")
WgradPlan = _struct("cy_wgrad_plan")
HeadPlan = _struct("cy_head_plan")
ClusterPlan = _struct("cy_cluster_plan")
JointPlan = _struct("cy_joint_plan_t")
GroupSoftmaxPlan = _struct("cy_group_softmax_plan_t")
NormActPlan = _struct("cy_norm_act_plan_t")
DenseProjPlan = _struct("cy_dense_proj_plan_t")
JointPatchPlan = _struct("cy_joint_patch_plan_t")
PixelMlpPlan = _struct("cy_pixel_mlp_plan_t")
ImsatPlan = _struct("cy_imsat_plan_t")
MixPlan = _struct("cy_mix_plan_t")
PriorPlan = _struct("cy_prior_plan_t")
TeacherPlan = _struct("cy_teacher_plan_t")
OptimPlan = _struct("cy_optim_plan_t")
WideRegPlan = _struct("cy_wide_reg_plan_t")
SlicPlan = _struct("cy_slic_plan_t")  # (and AugPlan: a refusal is their `status` field, the struct zeroed)
AugPlan = _struct("cy_aug_plan_t")
WgradReduceEntry = _struct("cy_wgrad_reduce_entry")
BnAcc = _struct("cy_bn_acc")
BnFold = _struct("cy_bn_fold")
BnBwdIn = _struct("cy_bn_bwd_in")
BnDzOut = _struct("cy_bn_dz_out")
BnRunItem = _struct("cy_bn_run_item")
MatLayout = _struct("cy_mat_layout")  # element (i, j) of batch (b1, b2) at b1*s1 + b2*s2 + i*rs + j*cs

# the entry points whose int return call() checks: a status, or a count / size that is never negative
# (cy_maxpool2_bwd_bn_num_partials returns a count or a negative status: the caller tests the sign itself)
_INT_FUNCS = frozenset(n for n, (res, _) in _SIGS.items() if res is c_int)

_lib = None


def exported_names():
    return sorted(_SIGS)


def load():
    """Load (once) and return the ctypes library with typed signatures."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise HipExtensionMissing(
            f"{LIB_PATH} not found: build it with `python contrast-you_amd/build.py` "
            "(there is no CPU fallback for the hot path)")
    # torch first: its wheel carries a HIP runtime of its own (torch/lib/libamdhip64.so, asked for under the unversioned
    # name).  Loaded after torch, this library's libamdhip64.so.7 resolves to that copy by soname; loaded before it, the
    # system's copy comes in and torch then maps its own next to it -- two runtimes in one process, and every launch
    # here on one of torch's streams fails (CY_ERR_LAUNCH).
    import torch  # noqa: F401
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    ver = lib.cy_abi_version()
    if ver != ABI_VERSION:
        raise HipExtensionMissing(f"ABI mismatch: library {ver}, binding {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(rc: int, name: str) -> int:
    if rc < 0:
        raise HipKernelError(f"{name} failed: {_ERRORS.get(rc, rc)}")
    return rc


def call(name: str, *args) -> int:
    """Call a status-returning entry point and raise on error."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if name in _INT_FUNCS:
        return check(rc, name)
    return rc
