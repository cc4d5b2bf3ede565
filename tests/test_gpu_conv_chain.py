"""One ConvChainFn block against torch.nn on the CPU in f64, across what its forward dispatches in one place: training
and eval-mode BatchNorms (per layer), the pooled second output, and the accumulator path against the finalize path
(ops.BN_ACC).  A backward through an eval-mode block, and through a block that mixes the two modes, runs nowhere else.

The block: [Conv2d(3 x 3, bias=False) -> BatchNorm2d -> ReLU] x 2 [-> MaxPool2d(2)], channels 8 -> 16 -> 16,
on N = 2, 16 x 16, f32 compute.  Bounds are the f32 ones of tests/test_gpu_unet.py: 1e-4 relative (to the largest
reference magnitude) on forward values, 2e-3 on gradients, 1e-5 on buffers.

Gradients through ReLU and max-pool are discontinuous where a pre-activation is zero or a window's two largest values
tie.  The inputs are continuous random data, and the seeds (SEED) were picked so that, in the f64 reference of every
mode, no BatchNorm output lies within MARGIN of zero and no pool window's two largest values within MARGIN of each
other -- ten times what f32 rounding moves them by; `_reference` asserts it.  A seed that lands on a routing flip is
replaced, the bound is not loosened."""
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, HW, CH = 2, 16, (8, 16, 16)
SEED = 11
MARGIN = 1e-5
MODES = [("train", "train"), ("eval", "eval"), ("train", "eval")]
MOMENTUM = 0.1


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _layers(chans, seed):
    """[(conv, bn)] in f64 on the CPU with non-trivial affine parameters and running statistics"""
    g = torch.Generator().manual_seed(seed)
    layers = []
    for cin, cout in zip(chans[:-1], chans[1:]):
        conv = nn.Conv2d(cin, cout, 3, padding=1, bias=False).double()
        bn = nn.BatchNorm2d(cout, momentum=MOMENTUM).double()
        with torch.no_grad():
            conv.weight.copy_(torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * (2.0 / (9 * cin)) ** 0.5)
            bn.weight.copy_(torch.rand(cout, generator=g, dtype=torch.float64) + 0.5)
            bn.bias.copy_(torch.rand(cout, generator=g, dtype=torch.float64) - 0.5)
            bn.running_mean.copy_(torch.randn(cout, generator=g, dtype=torch.float64) * 0.1)
            bn.running_var.copy_(torch.rand(cout, generator=g, dtype=torch.float64) + 0.5)
        layers.append((conv, bn))
    return layers


def _set_modes(layers, modes):
    for (_, bn), m in zip(layers, modes):
        bn.train(m == "train")


def _clear_of_zero(t):
    assert t.abs().min().item() > MARGIN, "a pre-activation within MARGIN of zero: pick another SEED"


def _ref_chain(layers, x):
    for conv, bn in layers:
        z = bn(conv(x))
        _clear_of_zero(z)
        x = torch.relu(z)
    return x


def _pool_clear_of_ties(out):
    top = torch.nn.functional.unfold(out.flatten(0, 1).unsqueeze(1), 2, stride=2).topk(2, dim=1).values
    gap = top[:, 0] - top[:, 1]
    gap = gap[top[:, 0] > 0]  # (a window of zeros only has no gradient to route)
    assert gap.min().item() > MARGIN, "a max-pool window with a near-tie: pick another SEED"


_REFS = {}


def _reference(modes, pool_out, shape=(N, HW, CH), seed=None):
    """the block in f64 on the CPU: inputs, loss weights, outputs, buffers after the pass and gradients.  Computed once
    per case and left unchanged."""
    seed = SEED if seed is None else seed
    key = (modes, pool_out, shape, seed)
    if key not in _REFS:
        n, hw, ch = shape
        g = torch.Generator().manual_seed(seed + 100)
        x = torch.randn(n, ch[0], hw, hw, generator=g, dtype=torch.float64).requires_grad_(True)
        r_out = torch.randn(n, ch[-1], hw, hw, generator=g, dtype=torch.float64)
        r_pool = torch.randn(n, ch[-1], hw // 2, hw // 2, generator=g, dtype=torch.float64)
        layers = _layers(ch, seed)
        _set_modes(layers, modes)
        out = _ref_chain(layers, x)
        loss = (out * r_out).sum()
        pooled = None
        if pool_out:
            _pool_clear_of_ties(out.detach())
            pooled = nn.MaxPool2d(2)(out)
            loss = loss + (pooled * r_pool).sum()
        loss.backward()
        _REFS[key] = dict(x=x, r_out=r_out, r_pool=r_pool, layers=layers, out=out.detach(),
                          pooled=None if pooled is None else pooled.detach())
    return _REFS[key]


def _device_layers(chans, seed, modes):
    """the same layers as f32 modules on the GPU, in their state before the pass"""
    layers = [(c.float().to(DEV), b.float().to(DEV)) for c, b in _layers(chans, seed)]
    _set_modes(layers, modes)
    return layers


def _chain_params(layers):
    return [p for conv, bn in layers for p in (conv.weight, bn.weight, bn.bias)]


def _check_layers(layers, ref_layers):
    for i, ((conv, bn), (rconv, rbn)) in enumerate(zip(layers, ref_layers)):
        assert rel_err(bn.running_mean, rbn.running_mean) < 1e-5, i
        assert rel_err(bn.running_var, rbn.running_var) < 1e-5, i
        assert bn.num_batches_tracked.item() == rbn.num_batches_tracked.item(), i
        for name, p, rp in (("weight", conv.weight, rconv.weight), ("gamma", bn.weight, rbn.weight),
                            ("beta", bn.bias, rbn.bias)):
            assert p.grad is not None, (i, name)
            assert rel_err(p.grad, rp.grad) < 2e-3, (i, name, rel_err(p.grad, rp.grad))


def _check_block(modes, pool_out, bn_acc, shape=(N, HW, CH), seed=None):
    from cyhip import ops
    from cyhip.functions import ChainCfg, ConvChainFn
    seed = SEED if seed is None else seed
    ref = _reference(modes, pool_out, shape, seed)
    ops.BN_ACC = bn_acc
    try:
        layers = _device_layers(shape[2], seed, modes)
        cfg = ChainCfg([bn for _, bn in layers], ops.CY_SRC_DIRECT, False, pool_out)
        cfg.dtype = torch.float32
        x = ref["x"].detach().float().to(DEV).requires_grad_(True)
        res = ConvChainFn.apply(cfg, x, None, *_chain_params(layers))
        out, pooled = res if pool_out else (res, None)
        loss = (out * ref["r_out"].float().to(DEV)).sum()
        if pool_out:
            loss = loss + (pooled * ref["r_pool"].float().to(DEV)).sum()
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.BN_ACC = True
    assert rel_err(out, ref["out"]) < 1e-4
    if pool_out:
        assert rel_err(pooled, ref["pooled"]) < 1e-4
    assert rel_err(x.grad, ref["x"].grad) < 2e-3, rel_err(x.grad, ref["x"].grad)
    _check_layers(layers, ref["layers"])


@pytest.mark.parametrize("bn_acc", [True, False], ids=["acc", "finalize"])
@pytest.mark.parametrize("pool_out", [False, True], ids=["plain", "pooled"])
@pytest.mark.parametrize("modes", MODES, ids=["-".join(m) for m in MODES])
def test_block_matches_torch_nn(modes, pool_out, bn_acc):
    _check_block(modes, pool_out, bn_acc)


WIDE = (1, 4, (16, 1040, 16))
WIDE_SEED = 1


def test_block_with_a_layer_wider_than_the_accumulator_path():
    """more than 1024 channels: that layer takes the finalize launch although ops.BN_ACC is on, and the whole block's
    backward runs on partial rows -- for the narrow second layer, from the first four rows of the coefficient block its
    accumulator-path forward left.  The smallest geometry the conv planner takes: N = 1, 4 x 4, 16 -> 1040 -> 16."""
    from cyhip import ops
    n, hw, ch = WIDE
    assert ops.conv3x3_plan(n, hw, hw, ch[0], 0, ch[1], torch.float32)["workgroups"] > 0
    _check_block(("train", "train"), True, True, WIDE, WIDE_SEED)


# ---- a block's output read by an _UpConv-style chain: the `_cy_tail` hand-off ----------------------------------------
UP_CH = (16, 8)
_UP_REFS = {}


def _up_reference(modes):
    """block (BatchNorm modes as given, no pooled output) -> Upsample(2) -> Conv2d(16, 8, 3) -> BatchNorm2d (the mode
    of the block's first) -> ReLU, in f64 on the CPU"""
    if modes not in _UP_REFS:
        g = torch.Generator().manual_seed(SEED + 200)
        x = torch.randn(N, CH[0], HW, HW, generator=g, dtype=torch.float64).requires_grad_(True)
        r_up = torch.randn(N, UP_CH[-1], 2 * HW, 2 * HW, generator=g, dtype=torch.float64)
        layers, up = _layers(CH, SEED), _layers(UP_CH, SEED + 1)
        _set_modes(layers, modes)
        _set_modes(up, modes[:1])
        out = _ref_chain(up, nn.Upsample(scale_factor=2)(_ref_chain(layers, x)))
        (out * r_up).sum().backward()
        _UP_REFS[modes] = dict(x=x, r_up=r_up, layers=layers, up=up, out=out.detach())
    return _UP_REFS[modes]


@pytest.mark.parametrize("bn_acc", [True, False], ids=["acc", "finalize"])
@pytest.mark.parametrize("modes", MODES, ids=["-".join(m) for m in MODES])
def test_upconv_chain_reading_a_block_matches_torch_nn(modes, bn_acc):
    """the upsample backward of the second chain writes the dA of the block's last BatchNorm and may add its backward
    sums on the way; inside one network pass (defer_batch_counters): the running statistics and the batch counters of
    all three layers are updated when the pass ends"""
    from cyhip import ops
    from cyhip.functions import ChainCfg, ConvChainFn, defer_batch_counters
    ref = _up_reference(modes)
    ops.BN_ACC = bn_acc
    try:
        layers, up = _device_layers(CH, SEED, modes), _device_layers(UP_CH, SEED + 1, modes[:1])
        cfg = ChainCfg([bn for _, bn in layers], ops.CY_SRC_DIRECT, False)
        up_cfg = ChainCfg([bn for _, bn in up], ops.CY_SRC_UP2, False)
        cfg.dtype = up_cfg.dtype = torch.float32
        x = ref["x"].detach().float().to(DEV).requires_grad_(True)
        with defer_batch_counters(x.device):
            mid = ConvChainFn.apply(cfg, x, None, *_chain_params(layers))
            out = ConvChainFn.apply(up_cfg, mid, None, *_chain_params(up))
        (out * ref["r_up"].float().to(DEV)).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.BN_ACC = True
    assert rel_err(out, ref["out"]) < 1e-4
    assert rel_err(x.grad, ref["x"].grad) < 2e-3, rel_err(x.grad, ref["x"].grad)
    _check_layers(layers, ref["layers"])
    _check_layers(up, ref["up"])
