"""The conv / weight-gradient launch plans of all three benchmark workloads (tests/c2_layers.py WORKLOADS: c2, c4, c5)
are reached by parity cases of tests/test_gpu_c2_geometry.py.  The launch plan is a pure host-side function of the layer
geometry, the batch and the storage type (cy_conv3x3_plan / cy_conv3x3_wgrad_plan), so the coverage claim is checked
here, on the CPU, twice: against the kernel instantiations the newest benchmark profile of each workload names, and --
independent of any profile -- against the plans today's planner gives every (layer, N, direction) of the workload table.
The GPU cases take their plans from the same queries and assert per case what a launch lets them observe of it.
Also here: the 2 GiB rule of the planners (32-bit buffer offsets below it, the 64-bit-offset kernels above)."""
import pytest
import torch

from tests import c2_layers as cl


def _gpu_case_lists(workload):
    """the parameter lists tests/test_gpu_c2_geometry.py hands to pytest.mark.parametrize for a workload:
    ((layer, N) cases, paired weight-gradient layers)"""
    from tests import test_gpu_c2_geometry as geo
    layers, batches, pair_layers = geo.GEOMETRY_CASES[workload]
    return [(l, n) for l in layers for n in batches], pair_layers


@pytest.mark.parametrize("workload", sorted(cl.WORKLOADS))
def test_every_profiled_conv_instantiation_has_a_parity_case(workload):
    path = cl.latest_profile(workload)
    assert path is not None, f"no kernel summary of the {workload} benchmark under profiles/"
    prof = cl.profiled_conv_kernels(path)
    assert prof, "no conv kernels found in the profile summary"
    row = cl.WORKLOADS[workload]
    cases, pair_layers = _gpu_case_lists(workload)
    tested = cl.kernel_names(cases, pair_layers, row["pair"], row["dtype"])
    missing = sorted(prof - tested)
    assert not missing, f"{path.name} names kernel instantiations no {workload}-geometry parity case reaches: {missing}"


@pytest.mark.parametrize("workload", sorted(cl.WORKLOADS))
def test_every_plan_of_a_workload_has_a_parity_case(workload):
    """no workload row, layer, N or direction is filtered out of the GPU parametrisation: the plan tuples of the
    workload table (left) against those of the lists the GPU cases are parametrised with (right)"""
    row = cl.WORKLOADS[workload]
    want = cl.workload_plan_tuples(workload)
    cases, pair_layers = _gpu_case_lists(workload)
    have = cl.case_tuples(cases, pair_layers, row["pair"], row["dtype"])
    assert want, workload
    missing = {t: want[t] for t in want if t not in have}
    assert not missing, (f"{len(missing)} launch plans of the {workload} benchmark have no parity case "
                         f"(plan tuple: launches that get it): {missing}")


def _largest_below_2gib(H, C, esz=2):
    """largest N for which an N x H x H x C tensor of esz-byte elements is addressable with 32-bit byte offsets"""
    return (2 ** 31 - 1) // (H * H * C * esz)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_two_gib_rule_streaming_layer(dtype):
    """224 x 224, 32 -> 32 channels (Conv1b): the last N below 2 GiB keeps the streaming kernel and the LDS-DMA weight
    gradient, the next one falls back to the 64-bit-offset plane kernel and wgrad12_kernel"""
    from cyhip import ops
    n = _largest_below_2gib(224, 32)
    assert n * 224 * 224 * 32 * 2 <= 2 ** 31 - 1 < (n + 1) * 224 * 224 * 32 * 2
    for pro in (0, 1):
        below = ops.conv3x3_plan(n, 224, 224, 32, 0, 32, dtype, 0, pro)
        above = ops.conv3x3_plan(n + 1, 224, 224, 32, 0, 32, dtype, 0, pro)
        assert below["kernel"] == "conv3x3_stream_kernel", below
        assert above["kernel"] == "conv3x3_plane_kernel", above
        wb = ops.conv3x3_wgrad_plan(n, 224, 224, 32, 0, 32, dtype, 0, pro)
        wa = ops.conv3x3_wgrad_plan(n + 1, 224, 224, 32, 0, 32, dtype, 0, pro)
        assert wb["twelve"] == 2 and wb["dma"] == 1, wb
        assert wa["twelve"] == 1 and wa["dma"] == 0 and wa["blk_order"] == 0, wa


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_two_gib_rule_flow_layer(dtype):
    """56 x 56, 128 -> 128 channels (Conv3b): the limit falls at another N; below it the flow kernel and the LDS-DMA
    weight gradient, above it the plane kernel and register-staging loaders (64 x 64 blocks keep wgrad12s_kernel)"""
    from cyhip import ops
    n = _largest_below_2gib(56, 128)
    assert n != _largest_below_2gib(224, 32)
    below = ops.conv3x3_plan(n, 56, 56, 128, 0, 128, dtype, 0, 1)
    above = ops.conv3x3_plan(n + 1, 56, 56, 128, 0, 128, dtype, 0, 1)
    assert below["kernel"] == "conv3x3_flow_kernel", below
    assert above["kernel"] == "conv3x3_plane_kernel", above
    wb = ops.conv3x3_wgrad_plan(n, 56, 56, 128, 0, 128, dtype, 0, 1)
    wa = ops.conv3x3_wgrad_plan(n + 1, 56, 56, 128, 0, 128, dtype, 0, 1)
    assert wb["twelve"] == 2 and wb["dma"] == 1, wb
    assert wa["dma"] == 0 and wa["blk_order"] == 0, wa
    # the paired launch is planned from the total batch
    wp = ops.conv3x3_wgrad_plan(n - 15, 56, 56, 128, 0, 128, dtype, 0, 1, n_b=16)
    assert wp["dma"] == 0, wp


def test_plan_query_matches_partials_and_split():
    from cyhip import ops
    p = ops.conv3x3_plan(16, 28, 28, 256, 0, 256, torch.bfloat16, 0, 1)  # Conv4b at N=16: four-wave 16 x 64 tiles
    assert p["kernel"] == "conv3x3_flow_kernel" and p["bn"] == 64 and p["th"] == 16 and p["ksplit"] == 1
    assert p["workgroups"] == 224
    pd = ops.conv3x3_plan(16, 14, 14, 512, 0, 256, torch.bfloat16, 0, 0)  # Conv5a data gradient at N=16: 56 such
    assert pd["kernel"] == "conv3x3_flow_kernel" and pd["bn"] == 128 and pd["ksplit"] == 8  # tiles: split-K stays
    p5 = ops.conv3x3_plan(16, 14, 14, 512, 0, 512, torch.bfloat16, 0, 1)  # Conv5b at N=16: split-K over 8-chunk ranges
    assert p5["kernel"] == "conv3x3_flow_kernel" and p5["ksplit"] == 4 and p5["workgroups"] == 224
    q = ops.conv3x3_plan(16, 28, 28, 128, 0, 256, torch.bfloat16, 1, 0)  # Conv4a: 2x2 max on load stays on the plane kernel
    assert q["kernel"] == "conv3x3_plane_kernel" and q["bn"] == 128
    w = ops.conv3x3_wgrad_plan(16, 14, 14, 512, 0, 512, torch.bfloat16, 0, 1)
    assert w["splits"] >= 1 and w["workgroups"] >= 64


FLOW_TILINGS = {(16, 128), (32, 128), (64, 64), (32, 64), (16, 64)}  # (th, bn): the list in csrc/cy_conv_flow.h
IGEMM_TILES = {(8, 32), (16, 16), (32, 8)}


def _plan_violations(d, p, q):
    """the invariants (a) .. (i) that tie a plan to what the dispatcher can launch and the other queries report;
    d: descriptor, p: cy_conv_plan, q: the other queries' answers.  Returns the letters of the broken ones."""
    IGEMM, PLANE, STREAM, FLOW = 0, 1, 4, 5  # CY_CONV_KERNEL_*
    Cin, bits16, tile = d.C1 + d.C2, d.in_dtype != 0, (p.th, p.tw, p.bn)
    bad = []
    if q["ws_bytes"] != (p.ksplit * d.N * d.H * d.W * d.Cout * 4 if p.ksplit > 1 else 0):
        bad.append("a")
    if q["num_partials"] != p.partials:
        bad.append("b")
    if p.kernel == STREAM:
        if not (bits16 and tile == (16, 14, d.Cout) and p.ksplit == 1 and Cin in (32, 64) and d.Cout in (32, 64)
                and p.partials == 4 * q["stat_workgroups"]):
            bad.append("c")
    elif q["stat_workgroups"] != p.partials:
        bad.append("c")
    if p.kernel == FLOW and not (bits16 and (p.th, p.bn) in FLOW_TILINGS and p.tw in (14, 16) and d.W % p.tw == 0
                                 and d.Cout % p.bn == 0 and d.mode1 != 1):
        bad.append("d")
    if p.kernel == PLANE and not ((p.th, p.tw) == (16, 14) and d.W % 14 == 0 and p.bn in (32, 64, 128)):
        bad.append("e")
    if p.kernel == IGEMM and not (((p.th, p.tw) in IGEMM_TILES and p.bn in (32, 64, 128))
                                  or tile in ((8, 28, 128), (16, 14, 128))):
        bad.append("f")
    if p.kernel not in (IGEMM, PLANE, STREAM, FLOW):
        bad.append("kernel")
    if p.one_per_cu and not (p.kernel == PLANE and p.bn == 128):
        bad.append("g")
    if q["dgrad_bn_ok"] and not (p.kernel == FLOW and d.prologue == 2):
        bad.append("h")
    if q["dgrad_dz_ok"] and not (p.kernel == FLOW and p.ksplit == 1 and p.th == 16):
        bad.append("i")
    return bad


def test_every_plan_is_one_the_dispatcher_can_launch():
    """Every valid descriptor of the reduced grid of tools/plan_dump.py (unit leading dimensions, N in 1, 3, 16, 32,
    512; invalid combinations are those cy_conv3x3_plan itself refuses) gets a plan that dispatch_conv has a kernel
    instantiation for, and the partial / workspace / fused-data-gradient queries agree with it.  A tiling added to the
    planner and not to the dispatcher shows up here instead of as CY_ERR_SHAPE on some layer at run time."""
    from cyhip import _lib
    from tools import plan_dump
    lib = plan_dump.load(_lib.LIB_PATH)
    d, p = _lib.ConvDesc(), _lib.ConvPlan()
    names = [n for n, _ in _lib.ConvDesc._fields_]
    valid, broken = 0, []
    for fields in plan_dump.descriptors(reduced=True):
        for n, v in zip(names, fields):
            setattr(d, n, v)
        if lib.cy_conv3x3_plan(d, p) != 0:
            continue
        valid += 1
        q = {"ws_bytes": lib.cy_conv3x3_fwd_ws_bytes(d), "num_partials": lib.cy_conv3x3_num_partials(d),
             "stat_workgroups": lib.cy_conv3x3_stat_workgroups(d), "dgrad_bn_ok": lib.cy_conv3x3_dgrad_bn_ok(d),
             "dgrad_dz_ok": lib.cy_conv3x3_dgrad_dz_ok(d, 0, d.Cout)}
        bad = _plan_violations(d, p, q)
        if bad:
            broken.append((bad, fields, {f: getattr(p, f) for f, _ in p._fields_}, q))
    assert valid > 150000, valid  # (270 480 of the 518 400 combinations pass cy_conv3x3_plan's own checks today)
    assert not broken, f"{len(broken)} of {valid} plans break an invariant; the first: {broken[:3]}"
