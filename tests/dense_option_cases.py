"""The cases tests/test_gpu_dense_options.py is parametrised with, their seeded inputs, the float64 reference, and the
CPU emulation of the 16-bit kernels' rounding points; tests/test_dense_options_host.py checks on the CPU what the cases
reach (read from the host-side plan query, cyhip.ops.pixel_mlp_plan).  A plain module: no GPU, no library call at
import.

A case is (M rows computed, C, ldx, hid, out, normalize, idx, dtype name).  `idx`: the rows are a shuffled subset of
R = M + 37 rows of x; otherwise x has exactly M rows.  hid == 0 is the linear head.

The row counts: 1 (a one-row problem), 63 and 126 = 2 * 7 * 9 (partial last tiles of 64- and 32-row tiles), and one
row past `forward workgroup cap x rows per tile` (1024 x 64 for 16-bit rows, 1024 x 32 for f32 rows): the forward
kernel makes its second trip there and the backward kernel (256 workgroups) its fifth.  Those cases keep C, hid and
out small, so a float64 reference of 65 537 rows costs a fraction of a second.
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

DenseCase = namedtuple("DenseCase", "M C ldx hid out normalize idx dtype")

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SLOPE = 0.01
PAST_CAP = {"f32": 1024 * 32 + 1, "bf16": 1024 * 64 + 1, "f16": 1024 * 64 + 1}

CASES = [
    DenseCase(1, 8, 8, 64, 5, True, False, "f32"),
    DenseCase(63, 32, 40, 256, 32, False, False, "f32"),          # pixel stride > C
    DenseCase(126, 256, 256, 0, 256, True, True, "f32"),          # linear head, row list
    DenseCase(126, 256, 256, 256, 256, True, False, "f32"),       # every size at its maximum: the largest LDS tiles
    DenseCase(PAST_CAP["f32"], 8, 8, 64, 5, True, False, "f32"),
    DenseCase(1, 32, 32, 0, 5, False, True, "bf16"),
    DenseCase(63, 8, 8, 64, 32, True, False, "bf16"),
    DenseCase(126, 256, 256, 256, 256, True, True, "bf16"),
    DenseCase(PAST_CAP["bf16"], 8, 8, 64, 5, True, False, "bf16"),
    DenseCase(126, 32, 48, 64, 32, True, False, "f16"),           # pixel stride > C
    DenseCase(63, 256, 256, 0, 256, False, True, "f16"),
    DenseCase(PAST_CAP["f16"], 32, 32, 0, 5, True, False, "f16"),
]


def case_id(c):
    return (f"M{c.M}-C{c.C}" + (f"ld{c.ldx}" if c.ldx != c.C else "") + f"-h{c.hid}-o{c.out}-{c.dtype}"
            + ("-norm" if c.normalize else "") + ("-idx" if c.idx else ""))


def plan(c):
    from cyhip import ops
    return ops.pixel_mlp_plan(c.M, c.C, c.hid, c.out, DTYPES[c.dtype])


@functools.lru_cache(maxsize=None)
def inputs(c):
    """seeded CPU tensors: x [R, ldx] in the storage type (the kernel reads x[:, :C]), idx int32 [M] or None, f32
    weights and biases, dy f32 [M, out]"""
    g = torch.Generator().manual_seed(7000 + CASES.index(c))
    R = c.M + 37 if c.idx else c.M
    x = torch.randn(R, c.ldx, generator=g).to(DTYPES[c.dtype])
    idx = torch.randperm(R, generator=g)[:c.M].to(torch.int32) if c.idx else None
    j1 = c.hid if c.hid else c.out
    w1 = torch.randn(j1, c.C, generator=g) / c.C ** 0.5
    b1 = torch.randn(j1, generator=g) * 0.5
    w2 = b2 = None
    if c.hid:
        w2 = torch.randn(c.out, c.hid, generator=g) / c.hid ** 0.5
        b2 = torch.randn(c.out, generator=g) * 0.5
    if c.hid:
        # LeakyReLU's derivative jumps at 0: a pre-activation that the kernel's f32 sums and the float64 reference put
        # on different sides of it moves one element of dH by its own size, which is no error of either.  Rows with a
        # pre-activation (on the operands the kernel multiplies: W1 in the storage type) closer to 0 than 1e-4, a
        # hundred times the f32 summation error of 256 terms, are drawn again.
        w1t = w1.to(DTYPES[c.dtype]).double()
        for _ in range(20):
            pre = x[:, :c.C].double() @ w1t.t() + b1.double()
            bad = (pre.abs() < 1e-4).any(dim=1)
            if not bad.any():
                break
            x[bad] = torch.randn(int(bad.sum()), c.ldx, generator=g).to(DTYPES[c.dtype])
        assert not bad.any()
    dy = torch.randn(c.M, c.out, generator=g)
    return dict(x=x, idx=idx, w1=w1, b1=b1, w2=w2, b2=b2, dy=dy)


def _rows(c, t):
    x = t["x"][:, :c.C].double()
    return x if t["idx"] is None else x[t["idx"].long()]


def _scatter_dx(c, t, dxr):
    """gradient of the selected rows -> [R, ldx] like x: zero at the other rows and at the padding columns"""
    dx = torch.zeros(t["x"].shape, dtype=torch.float64)
    sel = torch.arange(c.M) if t["idx"] is None else t["idx"].long()
    dx[sel, :c.C] = dxr
    return dx


@functools.lru_cache(maxsize=None)
def reference(c):
    """float64 torch on the CPU: F.conv2d 1x1 -> leaky_relu -> F.conv2d 1x1 -> F.normalize, and autograd"""
    t = inputs(c)
    leaf = lambda v: None if v is None else v.double().requires_grad_(True)  # noqa: E731
    xr = _rows(c, t).requires_grad_(True)
    w1, b1, w2, b2 = leaf(t["w1"]), leaf(t["b1"]), leaf(t["w2"]), leaf(t["b2"])
    fmap = xr.t().reshape(1, c.C, c.M, 1)
    y = F.conv2d(fmap, w1[:, :, None, None], b1)
    if c.hid:
        y = F.conv2d(F.leaky_relu(y, SLOPE), w2[:, :, None, None], b2)
    if c.normalize:
        y = F.normalize(y, p=2, dim=1)
    y = y.reshape(c.out, c.M).t()
    (y * t["dy"].double()).sum().backward()
    res = dict(y=y.detach(), dx=_scatter_dx(c, t, xr.grad), dw1=w1.grad, db1=b1.grad)
    if c.hid:
        res.update(dw2=w2.grad, db2=b2.grad)
    return res


def emulate(c):
    """The 16-bit kernels' arithmetic on the CPU, float64 sums between the same rounding points: W1 and W2 rounded to
    the storage type; bias and LeakyReLU unrounded; the hidden tile rounded once; backward: dY (formed from dy, the
    normalised y and inv) and dH rounded for their products and for the bias sums; dx rounded on its store."""
    t = inputs(c)
    T = DTYPES[c.dtype]
    rnd = lambda v: v.to(torch.float32).to(T).double()  # noqa: E731
    x = _rows(c, t)
    w1, b1, dy = rnd(t["w1"]), t["b1"].double(), t["dy"].double()
    pre = x @ w1.t() + b1
    if c.hid:
        w2, b2 = rnd(t["w2"]), t["b2"].double()
        h = rnd(torch.where(pre > 0, pre, SLOPE * pre))
        y = h @ w2.t() + b2
    else:
        y = pre
    if c.normalize:
        inv = 1.0 / y.norm(dim=1, keepdim=True).clamp_min(1e-12)
        y = y * inv
        dY = inv * (dy - y * (dy * y).sum(dim=1, keepdim=True))
    else:
        dY = dy
    g = rnd(dY)
    res = dict(y=y)
    if c.hid:
        res.update(dw2=g.t() @ h, db2=g.sum(0))
        g = rnd((g @ w2) * torch.where(pre > 0, 1.0, SLOPE))
    res.update(dw1=g.t() @ x, db1=g.sum(0), dx=_scatter_dx(c, t, rnd(g @ w1)))
    return res


def rel_err(got, want):
    """largest element-wise difference, relative to the reference tensor's largest magnitude"""
    return float((got.double() - want).abs().max() / want.abs().max())


def emulation_error(dtype):
    """(forward, gradient): the largest rel_err of emulate() against reference() over the cases of `dtype`"""
    fwd = grad = 0.0
    for c in CASES:
        if c.dtype != dtype:
            continue
        ref, emu = reference(c), emulate(c)
        fwd = max(fwd, rel_err(emu["y"], ref["y"]))
        grad = max([grad] + [rel_err(emu[k], ref[k]) for k in ref if k != "y"])
    return fwd, grad
