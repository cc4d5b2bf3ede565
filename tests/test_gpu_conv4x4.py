"""`cyhip.glue.Conv4x4Fn` (csrc/cy_conv4x4.hip) on the GPU against `F.conv2d` and its autograd in f64 on the CPU.

Exact cases: inputs, weights and output gradients on the 1/8 grid in [-1, 1].  Every product is a multiple of 1/64 of
magnitude <= 1 and every partial sum of up to 2^18 terms is exactly representable in f32, so any summation order gives
the f64 result: y, dx and dW must be `torch.equal` to it, no tolerance.  The longest sums here: 16 * 512 = 8 192 terms
forward, 1 568 output positions in a weight gradient.

Random cases: normal inputs, weights * 0.02; relative 2-norm and max-norm distance to f64 within
max(4 * e_ref, 1e-6), e_ref the larger of torch's CPU f32 distance and `Conv2dFn`'s distance on the GPU on the same
inputs -- never anything measured from the kernels under test.

Then: equal bits of two runs, `needs_input_grad`, the peak memory of a forward + backward against the size of the patch
matrix it no longer writes, and the discriminator through both settings of `Discriminator.conv` against an f64 replica
of torch's layers."""
import functools

import pytest
import torch
import torch.nn.functional as F

from torch import nn

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR, FACTOR = 1e-6, 4.0

# (stride, pad, (N, Cin, H, W, Cout)): the smallest shapes that reach each path
EXACT = [
    (2, 1, (1, 3, 4, 4, 6)),         # minimum: 2 x 2 outputs, Cin < 4
    (2, 1, (3, 5, 9, 11, 3)),        # odd H and W, 4-byte loads, a tile that spans images
    (2, 1, (2, 64, 18, 14, 64)),     # 16-byte loads, several reduction stages
    (2, 1, (2, 130, 10, 12, 70)),    # channel tails on both sides
    (2, 1, (5, 12, 34, 30, 24)),     # 1 275 rows: several row tiles and weight-gradient splits, a ragged last one
    (2, 1, (2, 64, 56, 56, 128)),    # the benchmark's second layer at N = 2
    (1, 0, (3, 24, 4, 4, 1)),        # a 1 x 1 output
    (1, 0, (2, 512, 6, 5, 1)),       # Cout = 1 form
    (1, 0, (2, 512, 14, 14, 1)),     # the benchmark's last layer, K = 8 192
    (1, 0, (2, 8, 7, 6, 40)),        # the MFMA form at stride 1 (forward, weight gradient)
    (1, 0, (2, 36, 7, 6, 40)),       # and its data gradient, which needs Cin >= 32 as well
    (2, 1, (1, 5, 20, 18, 64)),      # the first layer's form: MFMA forward, 16 lanes per pixel in the data gradient
    (2, 1, (2, 7, 9, 8, 40)),        # the same with idle lanes (Cout < 64), odd H, Cin = 7
    (2, 1, (1, 128, 6, 6, 32)),      # the 128 x 128 data-gradient tile with 16-byte loads (Cin > 64)
]
RANDOM = [(2, 1, (2, 64, 18, 14, 64)), (2, 1, (2, 130, 10, 12, 70)), (1, 0, (2, 512, 6, 5, 1))]


def out_hw(H, W, stride, pad):
    return (H + 2 * pad - 4) // stride + 1, (W + 2 * pad - 4) // stride + 1


@functools.lru_cache(maxsize=None)
def case(stride, pad, shape, kind):
    """-> (x, w, gy) f32 on the CPU and (y, dx, dw) of F.conv2d in f64; computed once, shared, never written to"""
    N, Cin, H, W, Cout = shape
    gen = torch.Generator().manual_seed(1000 * stride + sum(shape))
    Ho, Wo = out_hw(H, W, stride, pad)
    if kind == "grid":
        draw = lambda *s: torch.randint(-8, 9, s, generator=gen).float() / 8  # noqa: E731
        x, w, gy = draw(N, Cin, H, W), draw(Cout, Cin, 4, 4), draw(N, Cout, Ho, Wo)
    else:
        x, w = torch.randn(N, Cin, H, W, generator=gen), 0.02 * torch.randn(Cout, Cin, 4, 4, generator=gen)
        gy = torch.randn(N, Cout, Ho, Wo, generator=gen)
    return (x, w, gy), conv_ref(x, w, gy, stride, pad, torch.float64)


def conv_ref(x, w, gy, stride, pad, dtype):
    xs, ws = x.to(dtype).requires_grad_(True), w.to(dtype).requires_grad_(True)
    y = F.conv2d(xs, ws, None, stride, pad)
    y.backward(gy.to(dtype))
    return y.detach(), xs.grad, ws.grad


def nhwc_at_offset(t, floats):
    """t [N, C, H, W] on the GPU as an NHWC-dense tensor whose storage starts `floats` floats into an allocation"""
    N, Cc, H, W = t.shape
    flat = torch.empty(t.numel() + floats, dtype=torch.float32, device=DEV)
    view = flat[floats:].view(N, H, W, Cc).permute(0, 3, 1, 2)
    view.copy_(t)
    return view


def run(fn, x, w, gy, stride, pad, x_grad=True, w_grad=True):
    """x, w, gy already on the GPU -> (y, dx, dw) of `fn(x, w, stride, pad)`"""
    xs, ws = x.detach().requires_grad_(x_grad), w.detach().requires_grad_(w_grad)
    y = fn(xs, ws, stride, pad)
    y.backward(gy)
    return y.detach(), xs.grad, ws.grad


def conv4(x, w, stride, pad):
    from cyhip.glue import Conv4x4Fn
    return Conv4x4Fn.apply(x, w, stride, pad)


def conv2(x, w, stride, pad):
    from cyhip.glue import Conv2dFn
    return Conv2dFn.apply(x, w, None, stride, pad)


def assert_exact(got, want, tag):
    for name, g, r in zip(("y", "dx", "dw"), got, want):
        g = g.detach().double().cpu()
        assert g.shape == r.shape, (tag, name, g.shape, r.shape)
        bad = int((g != r).sum())
        assert torch.equal(g, r), f"{tag} {name}: {bad} of {r.numel()} elements differ, max {float((g - r).abs().max())}"


@pytest.mark.parametrize("stride,pad,shape", EXACT, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_exact_on_the_eighth_grid(stride, pad, shape):
    (x, w, gy), want = case(stride, pad, shape, "grid")
    got = run(conv4, x.to(DEV), w.to(DEV), gy.to(DEV), stride, pad)
    assert_exact(got, want, f"{shape} s{stride}p{pad}")
    assert got[0].permute(0, 2, 3, 1).is_contiguous()  # NCHW-shaped over NHWC memory


def test_exact_on_a_non_contiguous_view():
    stride, pad, shape = 2, 1, (2, 64, 18, 14, 64)
    (x, w, gy), want = case(stride, pad, shape, "grid")
    wide = torch.zeros(2, 64, 18, 30, device=DEV)
    wide[..., 1:29:2] = x.to(DEV)
    view = wide[..., 1:29:2]
    assert not view.is_contiguous() and not view.permute(0, 2, 3, 1).is_contiguous()
    wt = w.to(DEV).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)  # a weight that is no dense OIHW block either
    assert not wt.is_contiguous()
    assert_exact(run(conv4, view, wt, gy.to(DEV), stride, pad), want, "non-contiguous x")


@pytest.mark.parametrize("stride,pad,shape", [(2, 1, (2, 64, 18, 14, 64)), (1, 0, (2, 8, 7, 6, 40)),
                                              (1, 0, (2, 512, 6, 5, 1))])
def test_exact_four_bytes_into_an_allocation(stride, pad, shape):
    """channel counts that take the 16-byte loads, on bases that are 4 bytes off: the launcher must take the 4-byte
    loads (a misaligned 16-byte load would be the bug)"""
    (x, w, gy), want = case(stride, pad, shape, "grid")
    xo, gyo = nhwc_at_offset(x.to(DEV), 1), nhwc_at_offset(gy.to(DEV), 1)
    assert xo.data_ptr() % 16 == 4 and gyo.data_ptr() % 16 == 4
    assert_exact(run(conv4, xo, w.to(DEV), gyo, stride, pad), want, f"offset {shape}")
    assert_exact(run(conv4, xo, w.to(DEV), gy.to(DEV), stride, pad), want, f"offset x only {shape}")
    assert_exact(run(conv4, x.to(DEV), w.to(DEV), gyo, stride, pad), want, f"offset dy only {shape}")


def dist(got, want):
    got, want = got.detach().double().cpu(), want.double()
    assert got.shape == want.shape and torch.isfinite(got).all()
    d = got - want
    return float(d.norm() / want.norm()), float(d.abs().max() / want.abs().max())


def bound(e_ref):
    return max(FACTOR * e_ref, FLOOR)


@pytest.mark.parametrize("stride,pad,shape", RANDOM, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_random_inputs_within_the_reference_distance(stride, pad, shape):
    (x, w, gy), want = case(stride, pad, shape, "normal")
    cpu32 = conv_ref(x, w, gy, stride, pad, torch.float32)
    dev = (x.to(DEV), w.to(DEV), gy.to(DEV))
    old, new = run(conv2, *dev, stride, pad), run(conv4, *dev, stride, pad)
    fails = []
    for name, r64, r32, o, n in zip(("y", "dx", "dw"), want, cpu32, old, new):
        e_cpu, e_old, e_new = dist(r32, r64), dist(o, r64), dist(n, r64)
        for norm, i in (("e_2", 0), ("e_max", 1)):
            e_ref = max(e_cpu[i], e_old[i])
            print(f"{shape} s{stride} {name} {norm}: Conv4x4Fn {e_new[i]:.2e}  (torch f32 CPU {e_cpu[i]:.2e}, Conv2dFn "
                  f"{e_old[i]:.2e}, bound {bound(e_ref):.2e})")
            if e_new[i] > bound(e_ref):
                fails.append(f"{name} {norm} {e_new[i]:.2e} > {bound(e_ref):.2e}")
    assert not fails, fails


def test_two_runs_give_the_same_bits():
    stride, pad, shape = 2, 1, (5, 12, 34, 30, 24)
    (x, w, gy), _ = case(stride, pad, shape, "normal")
    dev = (x.to(DEV), w.to(DEV), gy.to(DEV))
    a, b = run(conv4, *dev, stride, pad), run(conv4, *dev, stride, pad)
    for name, p, q in zip(("y", "dx", "dw"), a, b):
        assert torch.equal(p, q), name
    # and the MFMA form, whose weight gradient is split over several ranges of output positions
    stride, pad, shape = 2, 1, (2, 64, 56, 56, 128)
    (x, w, gy), _ = case(stride, pad, shape, "grid")
    g = torch.Generator().manual_seed(5)
    dev = (torch.randn(x.shape, generator=g).to(DEV), w.to(DEV), torch.randn(gy.shape, generator=g).to(DEV))
    a, b = run(conv4, *dev, stride, pad), run(conv4, *dev, stride, pad)
    for name, p, q in zip(("y", "dx", "dw"), a, b):
        assert torch.equal(p, q), name


@pytest.mark.parametrize("stride,pad,shape", [(2, 1, (2, 64, 18, 14, 64)), (1, 0, (2, 512, 6, 5, 1))])
def test_gradients_that_are_not_needed_are_not_computed(monkeypatch, stride, pad, shape):
    from cyhip import ops
    (x, w, gy), _ = case(stride, pad, shape, "normal")
    dev = (x.to(DEV), w.to(DEV), gy.to(DEV))
    calls = {"wgrad": 0, "dgrad": 0}
    for name in calls:
        real = getattr(ops, f"conv4x4_{name}")

        def counted(*a, _real=real, _name=name, **k):
            calls[_name] += 1
            return _real(*a, **k)

        monkeypatch.setattr(ops, f"conv4x4_{name}", counted)
    _, dx_full, dw_full = run(conv4, *dev, stride, pad)
    assert calls == {"wgrad": 1, "dgrad": 1} and dw_full is not None
    _, dx, dw = run(conv4, *dev, stride, pad, w_grad=False)  # a detached weight: no weight-gradient launch
    assert dw is None and calls == {"wgrad": 1, "dgrad": 2}
    assert torch.equal(dx, dx_full)
    _, dx, dw = run(conv4, *dev, stride, pad, x_grad=False)  # an input without gradient: no data-gradient launch
    assert dx is None and calls == {"wgrad": 2, "dgrad": 2}
    assert torch.equal(dw, dw_full)


def test_peak_memory_stays_below_the_patch_matrix():
    """x [8, 64, 56, 56] -> 128 channels: the patch matrix alone would be 8 * 28 * 28 * 1024 * 4 bytes"""
    N, Cin, H, Cout = 8, 64, 56, 128
    patch_bytes = N * (H // 2) * (H // 2) * 16 * Cin * 4
    assert patch_bytes == 25_690_112
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, H, H, Cin, generator=g).to(DEV).permute(0, 3, 1, 2).requires_grad_(True)
    w = (0.02 * torch.randn(Cout, Cin, 4, 4, generator=g)).to(DEV).requires_grad_(True)
    gy = torch.randn(N, H // 2, H // 2, Cout, generator=g).to(DEV).permute(0, 3, 1, 2)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    y = conv4(x, w, 2, 1)
    y.backward(gy)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"peak {peak / 1e6:.1f} MB above the inputs; patch matrix {patch_bytes / 1e6:.1f} MB")
    assert x.grad is not None and w.grad is not None
    assert peak < patch_bytes


# ---------------------------------------------------------------------------------------------- the discriminator
HIDDEN, KCLS = 16, 4


def replica(sd, dtype):
    """torch's own layers in the discriminator's order at hidden_dim = HIDDEN under the state dict `sd`, on the CPU
    (`tests/adversarial_fixture.py: replica` is the same construction, fixed at that fixture's hidden_dim)"""
    cin, h = 1 + KCLS, HIDDEN
    main = nn.Sequential(
        nn.Conv2d(cin, h, 4, 2, 1, bias=False), nn.LeakyReLU(0.2),
        nn.Conv2d(h, 2 * h, 4, 2, 1, bias=False), nn.BatchNorm2d(2 * h), nn.LeakyReLU(0.2),
        nn.Conv2d(2 * h, 4 * h, 4, 2, 1, bias=False), nn.BatchNorm2d(4 * h), nn.LeakyReLU(0.2),
        nn.Conv2d(4 * h, 8 * h, 4, 2, 1, bias=False), nn.BatchNorm2d(8 * h), nn.LeakyReLU(0.2),
        nn.Conv2d(8 * h, 1, 4, 1, 0, bias=False), nn.Sigmoid())
    main.load_state_dict({k[len("_main."):]: v for k, v in sd.items()}, strict=True)
    return main.to(dtype)


def replica_pass(sd, image, logits, dtype):
    """scores (in front of the sigmoid), their sum's gradient on the logits and on every parameter, torch's layers"""
    main = replica(sd, dtype).train()
    z = logits.to(dtype).clone().requires_grad_(True)
    s = main[:-1](torch.cat([image.to(dtype), z.softmax(1)], 1))
    s.sum().backward()
    return s.detach(), z.grad, {f"_main.{k}": p.grad for k, p in main.named_parameters()}


@pytest.fixture(scope="module")
def disc_case():
    from contrastyou.arch.discriminator import Discriminator
    torch.manual_seed(21)
    sd = {k: v.clone() for k, v in Discriminator(1 + KCLS, HIDDEN).state_dict().items()}
    g = torch.Generator().manual_seed(22)
    image, logits = torch.rand(2, 1, 64, 64, generator=g), 2 * torch.randn(2, KCLS, 64, 64, generator=g)
    r64 = replica_pass(sd, image, logits, torch.float64)
    r32 = replica_pass(sd, image, logits, torch.float32)
    e_s, e_z = dist(r32[0], r64[0]), dist(r32[1], r64[1])
    e_p = [dist(r32[2][k], r64[2][k]) for k in r64[2]]
    e_p = (max(e[0] for e in e_p), max(e[1] for e in e_p))  # the largest over the tensors of the kind
    return sd, image, logits, r64, {"scores": e_s, "dlogits": e_z, "params": e_p}


@pytest.mark.parametrize("path", ["conv_implicit", "conv_im2col"])
def test_discriminator_through_both_convolutions(disc_case, path):
    from contrastyou.arch import discriminator as D
    sd, image, logits, (s64, dz64, dp64), e_ref = disc_case
    assert D.Discriminator.conv is D.conv_implicit
    D.Discriminator.conv = staticmethod(getattr(D, path))
    try:
        dis = D.Discriminator(1 + KCLS, HIDDEN).to(DEV).train()
        dis.load_state_dict(sd, strict=True)
        z = logits.to(DEV).requires_grad_(True)
        s = dis.scores_from_logits(image.to(DEV), z)
        s.sum().backward()
    finally:
        D.Discriminator.conv = staticmethod(D.conv_implicit)
    fails = []

    def check(what, got, want, kind):
        e = dist(got, want)
        b = (bound(e_ref[kind][0]), bound(e_ref[kind][1]))
        print(f"{path} {what}: e_2 {e[0]:.2e} (bound {b[0]:.2e})  e_max {e[1]:.2e} (bound {b[1]:.2e})")
        if e[0] > b[0] or e[1] > b[1]:
            fails.append((what, e, b))

    check("scores", s, s64, "scores")
    check("d sum / d logits", z.grad, dz64, "dlogits")
    grads = dict(dis.named_parameters())
    assert set(grads) == set(dp64)
    for k, want in dp64.items():
        check(f"d sum / d {k}", grads[k].grad, want, "params")
    assert not fails, fails
