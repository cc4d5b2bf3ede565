"""The weight gradient's slab sums as one batched launch (cy_wgrad_reduce_batched, cyhip.ops.DEFER_WGRAD_REDUCE).

A deferred weight gradient enqueues its MFMA (first layer: VALU) kernel only; the slab sums of many layers then run in
one launch in which every output keeps the summation tree of its own reduce launch (wgrad_reduce_kernel,
first_wgrad_reduce_kernel).  So everything here is bitwise: torch.equal against the immediate entry points, and whole
training steps with deferral on against deferral off.

The CPU test restates in Python the rules that decide the tree -- plan_wgrad's split count S and wgrad_impl's slab
group count SG (csrc/cy_wgrad.hip), the first layer's partial count -- and checks the host-side entry query against
them for every weight-gradient launch of bench.py's three workloads, so that the tree cannot drift unnoticed."""
import ctypes as C
import random
import sys
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

from tests import c2_layers as cl  # noqa: E402

# ---- the rules of today's immediate reduce, restated -----------------------------------------------------------------


def _roundup(a, b):
    return (a + b - 1) // b * b


def _conv_s_sg(N, H, W, Cin, Cout, dtype):
    """plan_wgrad's S and wgrad_impl's SG for a layer at N images (the total batch of a paired launch)"""
    twelve = dtype != torch.float32
    if not twelve:
        wco, wci = 1, 1
    elif Cout > 32 and Cin > 32:
        wco, wci = 2, 2
    elif Cout > 32:
        wco, wci = 2, 1
    elif Cin > 32:
        wco, wci = 1, 2
    else:
        wco, wci = 1, 1
    co_pad, ci_pad = _roundup(Cout, 32 * wco), _roundup(Cin, 32 * wci)
    TW = W if W <= 32 else (32 if W % 32 == 0 else (28 if W % 28 == 0 else 16))
    TH = max(th for th in range(1, 9) if th <= H and th * TW <= 256 and H % th == 0)
    ntiles = (N * H // TH) * ((W + TW - 1) // TW)
    out_tiles = (co_pad // (32 * wco)) * (ci_pad // (32 * wci))
    S = (256 if twelve else 512) // out_tiles
    S = min(S, (48 << 20) // (9 * co_pad * ci_pad * 4))
    S = min(max(S, 1), ntiles)
    total = Cout * (Cin // 4)
    SG = 1
    while SG < 32 and SG * 2 <= S and (total * SG) // 256 < 1024:
        SG *= 2
    return S, SG


def _first_s(N, Cin, H, W, Cout, dtype):
    """partials of the first layer's weight gradient (first_wgrad_mfma_blocks, else first_wgrad_blocks)"""
    if Cin == 1 and Cout == 32 and dtype in (torch.bfloat16, torch.float16) and H % 8 == 0 and W % 16 == 0 \
            and W <= 2048:
        return min(N * H // 8, 1024)
    npix = N * H * W
    b = min(max((npix + 1023) // 1024, 1), 1024)
    rows_max = (96 * 1024 // 4) // (W + 2) - 4
    return max(b, (npix + rows_max * W - 1) // (rows_max * W))


def _workload_wgrad_launches(workload):
    """(layer, N, n_b) of every conv weight-gradient launch of a workload (n_b > 0: paired) and its first-layer
    launches (None, N, 0)"""
    row = cl.WORKLOADS[workload]
    out = [(layer, N, 0) for layer, N in cl.workload_cases(workload)]
    out += [(layer, row["pair"][0], row["pair"][1]) for layer in cl.workload_pair_layers(workload)]
    out += [(None, N, 0) for N in row["batches"]]
    return out


@pytest.mark.parametrize("workload", sorted(cl.WORKLOADS))
def test_reduce_entries_keep_the_summation_tree(workload):
    from cyhip import ops
    row = cl.WORKLOADS[workload]
    dt = row["dtype"]
    n = 0
    for layer, N, n_b in _workload_wgrad_launches(workload):
        if layer is None:
            hw, cout = row["hw"], cl.MAX_CHANNEL // 16
            e = ops.first_wgrad_reduce_entry(N, 1, hw, hw, cout, dt)
            assert e["kind"] == 1 and (e["S"], e["SG"]) == (_first_s(N, 1, hw, hw, cout, dt), 64), (N, e)
            assert e["blocks"] == (cout * 9 + 3) // 4
        else:
            name, H, C1, C2, Cout, mode, pro = layer
            e = ops.wgrad_reduce_entry(N, H, H, C1, C2, Cout, dt, mode, bool(pro), n_b=n_b)
            want = _conv_s_sg(N + n_b, H, H, C1 + C2, Cout, dt)
            assert e["kind"] == 0 and (e["S"], e["SG"]) == want, (name, N, n_b, e, want)
            assert e["S"] == ops.conv3x3_wgrad_plan(N, H, H, C1, C2, Cout, dt, mode, bool(pro), n_b=n_b)["splits"]
            opb = 256 // e["SG"]
            assert e["blocks"] == (Cout * ((C1 + C2) // 4) + opb - 1) // opb
        n += 1
    assert n == len(_workload_wgrad_launches(workload)) and n > 0


# ---- GPU: the batched launch against the immediate entry points --------------------------------------------------------


def _wgrad_tuple_cases():
    """one (workload, layer, N, n_b) per weight-gradient plan tuple of the three workloads (single and paired)"""
    cases, seen = [], set()
    for wl in sorted(cl.WORKLOADS):
        layers = {l[0]: l for l in cl.workload_layers(wl)}
        for t, where in sorted(cl.workload_plan_tuples(wl).items(), key=lambda kv: repr(kv[0])):
            if t[0] != "wgrad" or (wl, t) in seen:
                continue
            seen.add((wl, t))
            name, N, kind = next(w for w in where if w[2] in ("wgrad", "wgrad_pair"))
            if kind == "wgrad_pair":
                cases.append(pytest.param(wl, layers[name], N[0], N[1], id=f"{wl}-{name}-pair{N[0]}+{N[1]}"))
            else:
                cases.append(pytest.param(wl, layers[name], N, 0, id=f"{wl}-{name}-N{N}"))
    return cases


def _nhwc(N, C, H, W, dt, g, scale=1.0):
    from cyhip import ops
    t = ops.empty_nhwc(N, C, H, W, dt, "cuda")
    t.copy_((torch.randn(N, C, H, W, device="cuda", generator=g) * scale).to(dt))
    return t


def _layer_operands(layer, N, dt, g):
    name, H, C1, C2, Cout, mode, pro = layer
    from cyhip import ops
    Hs = 2 * H if mode == ops.CY_SRC_POOL2 else (H // 2 if mode == ops.CY_SRC_UP2 else H)
    src1 = _nhwc(N, C1, Hs, Hs, dt, g)
    src2 = _nhwc(N, C2, H, H, dt, g) if C2 else None
    dy = _nhwc(N, Cout, H, H, dt, g, 0.01)
    scale = shift = None
    if pro:
        scale = torch.rand(C1, device="cuda", generator=g) + 0.5
        shift = torch.randn(C1, device="cuda", generator=g) * 0.1
    return src1, src2, dy, scale, shift


def _p(t):
    return None if t is None else t.data_ptr()


def _deferred_conv(layer, a, b, dw, accumulate):
    """the MFMA launch of cy_conv3x3_wgrad(_pair)_deferred into a fresh slab buffer: (entry, slab buffer)"""
    from cyhip import _lib, ops
    name, H, C1, C2, Cout, mode, pro = layer
    src1, src2, dy, scale, shift = a
    N = src1.shape[0]
    d = ops._desc(N, H, H, C1, C2, Cout, mode, 1 if pro else 0, ops.dtype_code(src1.dtype), C1, C2, Cout)
    e = _lib.WgradReduceEntry()
    if b is None:
        nbytes = _lib.load().cy_conv3x3_wgrad_ws_bytes(d.ref)
        ws = ops._ws(nbytes, "cuda")
        _lib.call("cy_conv3x3_wgrad_deferred", d.ref, src1.data_ptr(), _p(src2), _p(scale), _p(shift), dy.data_ptr(),
                  dw.data_ptr(), accumulate, ws.data_ptr(), nbytes, C.byref(e), ops._stream())
    else:
        s1b, s2b, dyb, scb, shb = b
        nbytes = _lib.load().cy_conv3x3_wgrad_pair_ws_bytes(d.ref, s1b.shape[0])
        ws = ops._ws(nbytes, "cuda")
        _lib.call("cy_conv3x3_wgrad_pair_deferred", d.ref, src1.data_ptr(), _p(src2), _p(scale), _p(shift),
                  dy.data_ptr(), s1b.shape[0], s1b.data_ptr(), _p(s2b), _p(scb), _p(shb), dyb.data_ptr(),
                  dw.data_ptr(), accumulate, ws.data_ptr(), nbytes, C.byref(e), ops._stream())
    return e, ws


def _immediate_conv(layer, a, b, dw, accumulate):
    from cyhip import _lib, ops
    name, H, C1, C2, Cout, mode, pro = layer
    src1, src2, dy, scale, shift = a
    N = src1.shape[0]
    d = ops._desc(N, H, H, C1, C2, Cout, mode, 1 if pro else 0, ops.dtype_code(src1.dtype), C1, C2, Cout)
    if b is None:
        nbytes = _lib.load().cy_conv3x3_wgrad_ws_bytes(d.ref)
        ws = ops._ws(nbytes, "cuda")
        _lib.call("cy_conv3x3_wgrad", d.ref, src1.data_ptr(), _p(src2), _p(scale), _p(shift), dy.data_ptr(),
                  dw.data_ptr(), accumulate, ws.data_ptr(), nbytes, ops._stream())
    else:
        s1b, s2b, dyb, scb, shb = b
        nbytes = _lib.load().cy_conv3x3_wgrad_pair_ws_bytes(d.ref, s1b.shape[0])
        ws = ops._ws(nbytes, "cuda")
        _lib.call("cy_conv3x3_wgrad_pair", d.ref, src1.data_ptr(), _p(src2), _p(scale), _p(shift), dy.data_ptr(),
                  s1b.shape[0], s1b.data_ptr(), _p(s2b), _p(scb), _p(shb), dyb.data_ptr(), dw.data_ptr(), accumulate,
                  ws.data_ptr(), nbytes, ops._stream())
    torch.cuda.synchronize()


def _batched(entries):
    from cyhip import _lib, ops
    arr = (_lib.WgradReduceEntry * len(entries))(*entries)
    _lib.call("cy_wgrad_reduce_batched", arr, len(entries), ops._stream())
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("workload,layer,N,n_b", _wgrad_tuple_cases())
def test_batched_reduce_is_bit_equal_per_plan(workload, layer, N, n_b):
    """accumulate 0 and 1 of one layer as two entries of one batched launch = the two immediate calls"""
    dt = cl.WORKLOADS[workload]["dtype"]
    g = torch.Generator(device="cuda").manual_seed(11)
    a = _layer_operands(layer, N, dt, g)
    b = _layer_operands(layer, n_b, dt, g) if n_b else None
    Cout, Cin = layer[4], layer[2] + layer[3]
    base = torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g)
    ref0, ref1 = torch.full_like(base, float("nan")), base.clone()
    _immediate_conv(layer, a, b, ref0, 0)
    _immediate_conv(layer, a, b, ref1, 1)
    out0, out1 = torch.full_like(base, float("nan")), base.clone()
    e0, ws0 = _deferred_conv(layer, a, b, out0, 0)
    e1, ws1 = _deferred_conv(layer, a, b, out1, 1)
    _batched([e0, e1])
    assert torch.equal(out0, ref0), (workload, layer[0], N, n_b, (out0 - ref0).abs().max().item())
    assert torch.equal(out1, ref1), (workload, layer[0], N, n_b, (out1 - ref1).abs().max().item())


@pytest.mark.gpu
def test_mixed_table_equals_the_launches_one_by_one():
    """conv, paired and first-layer entries in one table, two of them (first layer) and two others (a conv layer,
    single then paired) on one dW each: the updates of one dW take effect in table order"""
    from cyhip import _lib, ops
    dt = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(5)
    conv = ("c", 28, 64, 0, 128, 0, 1)
    cat = ("u", 56, 32, 32, 32, 0, 0)
    a, b = _layer_operands(conv, 4, dt, g), _layer_operands(conv, 6, dt, g)
    c = _layer_operands(cat, 3, dt, g)
    x = torch.randn(5, 1, 64, 64, device="cuda", generator=g)
    dyf = [_nhwc(5, 32, 64, 64, dt, g, 0.01) for _ in range(2)]
    w_conv = torch.randn(128, 64, 3, 3, device="cuda", generator=g)
    w_cat = torch.randn(32, 64, 3, 3, device="cuda", generator=g)
    w_first = torch.randn(32, 1, 3, 3, device="cuda", generator=g)

    def first(dw, dy, deferred):
        nbytes = _lib.load().cy_conv3x3_first_wgrad_ws_bytes(5, 1, 64, 64, 32)
        ws = ops._ws(nbytes, "cuda")
        if not deferred:
            _lib.call("cy_conv3x3_first_wgrad", x.data_ptr(), dy.data_ptr(), dw.data_ptr(), 1, 5, 1, 64, 64, 32,
                      ops.CY_BF16, ws.data_ptr(), nbytes, ops._stream())
            torch.cuda.synchronize()
            return None
        e = _lib.WgradReduceEntry()
        _lib.call("cy_conv3x3_first_wgrad_deferred", x.data_ptr(), dy.data_ptr(), dw.data_ptr(), 1, 5, 1, 64, 64, 32,
                  ops.CY_BF16, ws.data_ptr(), nbytes, C.byref(e), ops._stream())
        return e, ws

    ref = [w_conv.clone(), w_cat.clone(), w_first.clone()]
    _immediate_conv(conv, a, None, ref[0], 1)
    first(ref[2], dyf[0], False)
    _immediate_conv(cat, c, None, ref[1], 1)
    _immediate_conv(conv, a, b, ref[0], 1)
    first(ref[2], dyf[1], False)
    out = [w_conv.clone(), w_cat.clone(), w_first.clone()]
    keep = [_deferred_conv(conv, a, None, out[0], 1), first(out[2], dyf[0], True), _deferred_conv(cat, c, None, out[1], 1),
            _deferred_conv(conv, a, b, out[0], 1), first(out[2], dyf[1], True)]
    _batched([k[0] for k in keep])
    for o, r in zip(out, ref):
        assert torch.equal(o, r), (o - r).abs().max().item()


def _run_steps(steps: int, bf16: bool, defer: bool, flush_bytes=None):
    import bench
    from cyhip import ops
    dev = torch.device("cuda:0")
    was = ops.DEFER_WGRAD_REDUCE, ops.WGRAD_FLUSH_BYTES
    ops.DEFER_WGRAD_REDUCE, ops.WGRAD_FLUSH_BYTES = defer, flush_bytes
    try:
        random.seed(5)
        torch.manual_seed(3)
        ctx = bench.build_step(dev, 0, 4, 4, 64, 128, bf16=bf16)
        for e in range(steps):  # (step 0 eager, later ones replay the captured graphs)
            bench.run_epoch(ctx, dev, 1, e)
        torch.cuda.synchronize()
    finally:
        ops.DEFER_WGRAD_REDUCE, ops.WGRAD_FLUSH_BYTES = was
    state = {k: v.detach().clone() for k, v in ctx["model"].state_dict().items()}
    state.update({f"grad.{n}": p.grad.detach().clone() for n, p in ctx["model"].named_parameters()
                  if p.grad is not None})
    state.update({f"hook.{i}": v.detach().clone() for i, v in enumerate(ctx["hook"].parameters())})
    return state


@pytest.mark.gpu
@pytest.mark.parametrize("flush_bytes", [None, 1, 1 << 16], ids=["at-end", "every-layer", "64KiB-groups"])
@pytest.mark.parametrize("bf16", [True, False])
def test_training_steps_bit_equal_with_and_without_deferral(bf16, flush_bytes):
    """two-stage steps (both passes; eager, then graph replays) with ASYNC_WGRAD / TWO_STREAM at their defaults; the
    batched launches at the end of the backward pass only, or also inside it (ops.WGRAD_FLUSH_BYTES: after every layer,
    in groups)"""
    from cyhip import ops
    assert ops.ASYNC_WGRAD and ops.TWO_STREAM
    s_off = _run_steps(4, bf16, False)
    s_on = _run_steps(4, bf16, True, flush_bytes)
    assert s_off.keys() == s_on.keys()
    bad = [k for k in s_off if not torch.equal(s_off[k], s_on[k])]
    assert not bad, f"{len(bad)} of {len(s_off)} tensors differ with the slab sums deferred, e.g. {bad[:5]}"
