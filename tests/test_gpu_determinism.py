"""Run-to-run bit equality of the hot path.

The structural rule behind it ("Reproducibility"): every reduction of the path has a fixed order
-- per-workgroup partials summed by a second kernel in workgroup order (weight-gradient slabs, head / projector
gradients, loss means), or integer fixed-point sums whose adds commute (the BatchNorm accumulators, cy_bn_acc.h) -- and
no kernel accumulates floating point with atomics.  So two runs of the same step on the same inputs must agree in
every bit, whatever the streams, the graph replays and the arrival order of workgroups do; a kernel variant that
breaks the rule (round 2's dW1 / db1 form with coefficient loads carried across an MFMA block is the one known case,
never shipped, cause not identified) fails here rather than in a tolerance.
"""
import random
import sys
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

pytestmark = pytest.mark.gpu


def _run_steps(steps: int, dtype_bf16: bool):
    import bench

    dev = torch.device("cuda:0")
    random.seed(5)
    torch.manual_seed(3)
    ctx = bench.build_step(dev, 0, 4, 4, 64, 128, bf16=dtype_bf16)
    losses = []
    for e in range(steps):  # (one step per epocher run: step 0 eager, later ones replay the captured graphs)
        ep = bench.run_epoch(ctx, dev, 1, e)
        m = ep.get_metric()
        losses.append(repr(sorted((k, repr(v)) for k, v in m.items())))
    torch.cuda.synchronize()
    state = {k: v.detach().clone() for k, v in ctx["model"].state_dict().items()}
    state.update({f"hook.{i}": v.detach().clone() for i, v in enumerate(ctx["hook"].parameters())})
    return losses, state


@pytest.mark.parametrize("bf16", [True, False])
def test_training_steps_are_bit_reproducible(bf16):
    l0, s0 = _run_steps(4, bf16)
    l1, s1 = _run_steps(4, bf16)
    assert l0 == l1
    assert s0.keys() == s1.keys()
    bad = [k for k in s0 if not torch.equal(s0[k], s1[k])]
    assert not bad, f"{len(bad)} of {len(s0)} tensors differ between two identical runs, e.g. {bad[:5]}"


@pytest.mark.parametrize("geom", [(4, 64, 64, 56), (3, 128, 256, 28), (2, 512, 512, 14), (2, 32, 32, 112), (2, 64, 32, 112)])
def test_conv_family_is_bit_reproducible(geom):
    """forward (with statistics), data gradient and weight gradient of one 3x3 layer, four launches each"""
    from cyhip import ops

    N, Cin, Cout, H = geom
    dev, dt = "cuda", torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(1)
    x = ops.to_nhwc(torch.randn(N, Cin, H, H, generator=g).to(dev).to(dt))
    dy = ops.to_nhwc(torch.randn(N, Cout, H, H, generator=g).to(dev).to(dt))
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05).to(dev)
    wf, wd = ops.pack_weights(w, dt)
    ref = None
    for _ in range(4):
        y, part = ops.conv3x3_fwd(x, None, wf, Cout, want_stats=True)
        dx, _ = ops.conv3x3_fwd(dy, None, wd, Cin, want_stats=False)
        dw = ops.conv3x3_wgrad(x, None, dy)
        torch.cuda.synchronize()
        cur = (y.clone(), part.clone(), dx.clone(), dw.clone())
        if ref is None:
            ref = cur
        else:
            for a, b in zip(ref, cur):
                assert torch.equal(a, b)


def test_pinned_uploads_survive_a_host_running_ahead():
    """per-step host parameters (augmentation theta / gamma, labels, sampled rows) go up through cyhip.ops.pinned without
    a host sync; with the stream held by a spin kernel, four rings' worth of uploads of one shape must each arrive with
    the values handed in -- a refilled slot must not change what an earlier, still queued copy delivers"""
    from cyhip import _lib, ops

    dev = torch.device("cuda:0")
    n = 4 * 16
    _lib.call("cy_debug_spin", 20000, ops._stream())  # 20 ms: the uploads below are all enqueued behind it
    outs = [ops.pinned.upload(torch.full((16, 6), float(i)), dev) for i in range(n)]
    torch.cuda.synchronize()
    bad = [i for i, o in enumerate(outs) if not torch.equal(o.cpu(), torch.full((16, 6), float(i)))]
    assert not bad, f"{len(bad)} of {n} uploads delivered another upload's values, e.g. {bad[:5]}"
