"""The 3x3 conv layers of the reference U-Net (contrastyou/arch/unet.py:72-103) as (name, H, C1, C2, Cout, mode,
prologue) tuples in forward order, the table of bench.py's workloads (WORKLOADS: input size, images per launch, storage
type, layers and how the weight gradient is called -- bench.py's own defaults), the launch plans every (layer, N,
direction) of a workload gets from the library's host-side plan queries, and the kernel-instantiation names those plans
stand for (as they appear, mangled, in profiles/*kernel_stats*).  Shared by tests/test_plan_coverage.py (CPU: every
profiled instantiation and every plan tuple of a workload is reached by a parity case) and
tests/test_gpu_c2_geometry.py (GPU: those parity cases)."""
from __future__ import annotations

import re
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]


def unet_layers(hw: int = 224, max_channel: int = 512):
    c = [max_channel // 16 * m for m in (1, 2, 4, 8, 16)]
    s = [hw // (2 ** i) for i in range(5)]
    layers = [("Conv1b", s[0], c[0], 0, c[0], 0, 1)]
    for i in range(1, 5):
        layers.append((f"Conv{i + 1}a", s[i], c[i - 1], 0, c[i], 0, 0))   # reads the pooled tensor the previous block wrote
        layers.append((f"Conv{i + 1}b", s[i], c[i], 0, c[i], 0, 1))       # BN+ReLU prologue
    for i in range(3, -1, -1):
        layers.append((f"Up{i + 2}", s[i], c[i + 1], 0, c[i], 2, 0))      # nearest x2 on load
        layers.append((f"Up_conv{i + 2}a", s[i], c[i], c[i], c[i], 0, 0))  # concat (skip, up)
        layers.append((f"Up_conv{i + 2}b", s[i], c[i], 0, c[i], 0, 1))
    return layers


ENCODER = ("Conv1b", "Conv2a", "Conv2b", "Conv3a", "Conv3b", "Conv4a", "Conv4b", "Conv5a", "Conv5b")


def conv_kernel_name(plan: dict, dtype_tag: str = "DF16b", cin: int = 0, stats: bool = False, pro: bool = False) -> str:
    """mangled-name fragment of the instantiation a cy_conv_plan stands for (cin / stats / pro: what the streaming
    kernel is additionally instantiated on)"""
    b = lambda v: f"Lb{int(bool(v))}E"  # noqa: E731
    i = lambda v: f"Li{int(v)}E"  # noqa: E731
    if plan["kernel"] == "conv3x3_plane_kernel":
        wgm, wgn, pitch, allt = (2, 2, 128, 0) if plan["bn"] == 128 else (4, 1, 64, 1)
        return ("conv3x3_plane_kernelI" + dtype_tag + i(plan["th"]) + i(plan["bn"]) + i(wgm) + i(wgn) + i(pitch)
                + b(allt) + b(plan["one_per_cu"]) + "E")
    if plan["kernel"] == "conv3x3_flow_kernel":
        wgm, wgn = (4, 2) if plan["bn"] == 128 else ((4, 1) if plan["th"] in (16, 32) else (8, 1))
        return ("conv3x3_flow_kernelI" + dtype_tag + i(plan["th"]) + i(plan["bn"]) + i(wgm) + i(wgn) + b(plan["tw"] == 16) + i(0) + "E")  # (MODE 0: the forward / plain data-gradient build)
    if plan["kernel"] == "conv3x3_stream_kernel":
        return ("conv3x3_stream_kernelI" + dtype_tag + i(cin // 32) + i(plan["bn"] // 32) + b(stats) + b(pro) + "E")
    wgm, wgn = ((1, 4) if (plan["th"], plan["tw"]) in ((8, 28), (16, 14)) else (2, 2)) if plan["bn"] == 128 else (4, 1)
    pitch, allt = (128, 0) if plan["bn"] == 128 else (64, 1)
    # <TI, TO, ...>: a repeated __bf16 mangles as a substitution (S0_), a repeated builtin type (_Float16, float) in full
    second = "S0_" if dtype_tag == "DF16b" else dtype_tag
    return ("conv3x3_igemm_kernelI" + dtype_tag + second + i(plan["th"]) + i(plan["tw"]) + i(plan["bn"]) + i(wgm)
            + i(wgn) + i(pitch) + b(allt) + "E")


def wgrad_kernel_name(plan: dict, dtype_tag: str = "DF16b") -> str:
    if plan["twelve"] == 2:  # wgrad12s_kernel<T, WCO, WCI, DMA, BLK>: five built forms (dispatch_wgrad12s)
        return (f"wgrad12s_kernelI{dtype_tag}Li{plan['wco']}ELi{plan['wci']}ELb{int(bool(plan['dma']))}E"
                f"Lb{int(bool(plan['blk_order']))}E")
    base = "wgrad12_kernel" if plan["twelve"] else "wgrad_kernel"
    return f"{base}<{plan['wco']}, {plan['wci']}, {plan['wk']}"  # (prefix: a trailing type argument may follow)


def profiled_conv_kernels(path: Path):
    """conv / weight-gradient kernel instantiations named in a `rocprofv3 --kernel-trace --stats` summary
    (profiles/rNN_bench_c2_kernel_stats_single_stream.txt).  Every row that names a conv3x3 / wgrad main kernel
    must parse into an instantiation -- a row this function cannot read would otherwise be invisible to the
    coverage gate (rocprofv3's own demangling mutilated the streaming kernel's template
    arguments; tools/profile_round.sh now keeps the names mangled)."""
    names = set()
    for line in path.read_text().splitlines():
        tok = line.split("  ")[0].strip()
        if not tok or tok.startswith("#") or tok == "kernel":
            continue
        is_conv = "conv3x3_" in tok and not any(k in tok for k in ("conv3x3_first", "splitk"))
        is_wgrad = "wgrad" in tok and not any(k in tok for k in ("reduce", "first_wgrad"))
        if not (is_conv or is_wgrad):
            continue
        found = False
        m = re.search(r"(conv3x3_(?:plane|igemm|stream|flow)_kernelI\w+?)Ev", tok)
        if m:
            names.add(m.group(1))
            found = True
        m = re.search(r"(wgrad12s_kernelI(?:DF16[b_]|f)Li\d+ELi\d+ELb[01]ELb[01]E)E", tok)
        if m:
            names.add(m.group(1))
            found = True
        m = re.match(r"(wgrad(?:12)?_kernel<)(?:[A-Za-z_]\w*, )?(\d+, \d+, \d+)", tok)
        if m:
            names.add(m.group(1) + m.group(2))
            found = True
        m = re.search(r"(wgrad(?:12)?_kernel)I(?:DF16[b_]|f)?Li(\d+)ELi(\d+)ELi(\d+)E", tok)  # mangled form
        if m:
            names.add(f"{m.group(1)}<{m.group(2)}, {m.group(3)}, {m.group(4)}")
            found = True
        if not found:
            raise AssertionError(f"{path.name}: cannot tell which instantiation this row is: {tok!r}")
    return names


def latest_profile(workload: str = "c2"):
    """the newest kernel summary of a workload's benchmark run under profiles/, or None"""
    files = sorted((REPO / "profiles").glob(f"r*_bench_{workload}_kernel_stats_single_stream.txt"))
    return files[-1] if files else None


# ---- bench.py's workloads ---------------------------------------------------------------------------------------------
# One row per `bench.py --workload`, from its defaults: build_step / build_step_c5 / run_epoch and the argument parser
# (--n-labeled 16, --n-unlabeled 16, --hw 224 -> 256 for c4, --max-channel 512; c5: 256 slices x 2 views, until=Conv5).
#   batches: images per launch (two-stage step: the labeled pass, and the unlabeled pass = slices + their views)
#   pair:    (images of segment a, images of segment b) of cy_conv3x3_wgrad_pair on the encoder layers: the two passes of
#            a two-stage step share one launch (cyhip/functions.py wgrad_into_sink; the library pairs every 16-bit type:
#            wgrad_impl refuses only the four-wave f32 kernel).  The labeled pass is evaluated first, so it is
#            differentiated last and takes along what the unlabeled pass parked: the c4 row keeps that order; the c2
#            row keeps the order its parity case has always run (the plan sees the sum only).
WORKLOADS = {
    "c2": dict(hw=224, batches=(16, 32), dtype=torch.bfloat16, layers=None, pair=(16, 32)),
    "c4": dict(hw=256, batches=(16, 32), dtype=torch.float16, layers=None, pair=(32, 16)),
    "c5": dict(hw=224, batches=(512,), dtype=torch.bfloat16, layers=ENCODER, pair=None),
}
DTYPE_TAGS = {torch.bfloat16: "DF16b", torch.float16: "DF16_", torch.float32: "f"}
MAX_CHANNEL = 512


def workload_layers(workload: str):
    row = WORKLOADS[workload]
    return [l for l in unet_layers(row["hw"], MAX_CHANNEL) if row["layers"] is None or l[0] in row["layers"]]


def workload_cases(workload: str):
    """every (layer, N) launch of a workload"""
    return [(l, n) for l in workload_layers(workload) for n in WORKLOADS[workload]["batches"]]


def workload_pair_layers(workload: str):
    """the layers whose weight gradient the workload's step computes for both passes in one launch"""
    return [l for l in workload_layers(workload) if l[0] in ENCODER] if WORKLOADS[workload]["pair"] else []


def layer_plans(layer, N: int, dtype) -> dict:
    """the launch plans of one layer at N images: forward, data gradient (`dgrad`; for a concat layer also
    `dgrad_split`, the two-tensor form the step runs) and weight gradient"""
    from cyhip import ops
    name, H, C1, C2, Cout, mode, pro = layer
    plans = {"fwd": ops.conv3x3_plan(N, H, H, C1, C2, Cout, dtype, mode, bool(pro)),
             "dgrad": ops.conv3x3_plan(N, H, H, Cout, 0, C1 + C2, dtype, 0, False),
             "wgrad": ops.conv3x3_wgrad_plan(N, H, H, C1, C2, Cout, dtype, mode, bool(pro))}
    if C2:
        plans["dgrad_split"] = ops.conv3x3_plan(N, H, H, Cout, 0, C1 + C2, dtype, 0, False, split=C1)
    return plans


def pair_plan(layer, n_a: int, n_b: int, dtype) -> dict:
    from cyhip import ops
    name, H, C1, C2, Cout, mode, pro = layer
    return ops.conv3x3_wgrad_plan(n_a, H, H, C1, C2, Cout, dtype, mode, bool(pro), n_b=n_b)


def conv_tuple(plan: dict, dtype, geom=()):
    return ("conv", plan["kernel"], plan["th"], plan["tw"], plan["bn"], plan["ksplit"], plan["one_per_cu"],
            str(dtype)) + tuple(geom)


def wgrad_tuple(plan: dict, dtype, geom=()):
    return ("wgrad", plan["twelve"], plan["wco"], plan["wci"], plan["wk"], plan["th"], plan["tw"], plan["dma"],
            plan["blk_order"], str(dtype)) + tuple(geom)


def case_tuples(cases, pair_layers, pair, dtype) -> dict:
    """plan tuple -> the (layer name, N, direction) launches that produce it, for a list of (layer, N) cases and a list
    of layers whose weight gradient runs paired (`pair` = (n_a, n_b)).  A tuple is the plan's fields, the storage type
    and the image geometry the plan is applied to (H, input channels, output channels of that launch): the same tile on
    another image size is another case (32-row tiles on 14-row images cross image boundaries, on 56-row images not)."""
    out = {}
    for layer, N in cases:
        name, H, C1, C2, Cout, mode, pro = layer
        for k, p in layer_plans(layer, N, dtype).items():
            if k == "wgrad":
                t = wgrad_tuple(p, dtype, (H, C1 + C2, Cout))
            else:
                t = conv_tuple(p, dtype, (H, C1 + C2, Cout) if k == "fwd" else (H, Cout, C1 + C2))
            out.setdefault(t, []).append((name, N, k))
    for layer in pair_layers:
        name, H, C1, C2, Cout, mode, pro = layer
        # (its own entry point, cy_conv3x3_wgrad_pair: never the same case as a single launch with an equal plan)
        t = wgrad_tuple(pair_plan(layer, pair[0], pair[1], dtype), dtype, (H, C1 + C2, Cout, "pair"))
        out.setdefault(t, []).append((name, tuple(pair), "wgrad_pair"))
    return out


def workload_plan_tuples(workload: str) -> dict:
    """every plan tuple the workload's launches get from today's planner -> where it comes from"""
    row = WORKLOADS[workload]
    return case_tuples(workload_cases(workload), workload_pair_layers(workload), row["pair"], row["dtype"])


def kernel_names(cases, pair_layers, pair, dtype) -> set:
    """the instantiation names (profile spelling) of the same launches"""
    tag = DTYPE_TAGS[dtype]
    names = set()
    for layer, N in cases:
        name, H, C1, C2, Cout, mode, pro = layer
        p = layer_plans(layer, N, dtype)
        names.add(conv_kernel_name(p["fwd"], tag, cin=C1 + C2, stats=True, pro=bool(pro)))
        names.add(conv_kernel_name(p["dgrad"], tag, cin=Cout))
        if "dgrad_split" in p:
            names.add(conv_kernel_name(p["dgrad_split"], tag, cin=Cout))
        names.add(wgrad_kernel_name(p["wgrad"], tag))
    for layer in pair_layers:
        names.add(wgrad_kernel_name(pair_plan(layer, pair[0], pair[1], dtype), tag))
    return names
