"""The cases of tests/test_gpu_dense_dispatch.py: every form of the dense projector (csrc/cy_dense.hip VALU,
csrc/cy_dense_mfma.h register-resident, csrc/cy_dense_wide.h streamed) on non-square maps and past every launch cap,
and the adaptive pools and the row gather next to it.  Seeded CPU inputs, the float64 reference, and the helpers that
state what each case claims; tests/test_dense_proj_coverage.py checks those claims without a GPU.  A plain module: no
GPU, no library call at import.

Reference: torch on the CPU in float64 -- F.conv2d 1x1 -> F.leaky_relu(., slope) -> F.adaptive_avg_pool2d(., (sh, sw)),
autograd under a seeded upstream gradient for dx, dW1 and db1; with a bin list, the listed rows of the pooled map.
x and W1 are representable in the storage type; a pixel with a pre-activation (float64, on those operands) within
MARGIN of zero is drawn again (the rule of tests/dense_option_cases.inputs), so kernel and reference take the same side
of LeakyReLU and NO element is excluded from any comparison.
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SLOPE = 0.01
MARGIN = 1e-4

# ------------------------------------------------------------------------------------------------ geometries
Geom = namedtuple("Geom", "N H W sh sw listed")

GEOMS = {
    "nonsquare_a": Geom(2, 23, 38, 5, 9, False),   # H != W, sh != sw, ragged bins, different ratios per axis
    "nonsquare_b": Geom(2, 38, 23, 7, 4, False),   # the transposed sense
    "one_bin": Geom(1, 19, 21, 1, 1, False),       # one job of 399 pixels = 13 blocks of 32, the last partial
    "pixel_bins": Geom(2, 9, 12, 9, 12, False),    # every bin one pixel, every odd cell segment empty
    "big_bins": Geom(2, 40, 56, 2, 3, False),      # bins of 20 x 19 pixels and more
    "past_cap": Geom(3, 33, 33, 32, 32, False),    # 3 072 bins, 11 907 cells
    "long_list": Geom(3, 33, 33, 32, 32, True),    # a shuffled list of every bin with (i + j) % 5 != 0
}

Inst = namedtuple("Inst", "form C hid dtype slope")

VALU = [Inst("valu", C, hid, dt, SLOPE) for dt in ("f32", "bf16", "f16") for C in (8, 40, 96) for hid in (64, 256)] + \
       [Inst("valu", 32, 128, dt, 1.5) for dt in ("bf16", "f16")]   # slope > 1 keeps a matrix-core shape on the VALU form
REG = [Inst("reg", C, hid, dt, SLOPE) for dt in ("bf16", "f16") for C in (32, 64, 128) for hid in (128, 256)]
STREAM = [Inst("stream", C, hid, dt, SLOPE) for dt in ("bf16", "f16") for C in (256, 512) for hid in (128, 256)]
INSTANCES = VALU + REG + STREAM

# the geometries that do not run on every instantiation: once per form and storage type
ROTATION = [Inst("valu", 40, 64, "f32", SLOPE), Inst("valu", 40, 64, "bf16", SLOPE), Inst("valu", 96, 256, "f16", SLOPE),
            Inst("reg", 64, 256, "bf16", SLOPE), Inst("reg", 128, 128, "f16", SLOPE),
            Inst("stream", 256, 128, "bf16", SLOPE), Inst("stream", 512, 256, "f16", SLOPE)]
# the option cases (null outputs, accumulate, ldx > C): nonsquare_a, one instantiation of every form
OPTION_INSTANCES = [Inst("valu", 40, 64, "f32", SLOPE), Inst("valu", 40, 64, "bf16", SLOPE),
                    Inst("reg", 64, 256, "bf16", SLOPE), Inst("reg", 32, 128, "f16", SLOPE),
                    Inst("stream", 256, 128, "f16", SLOPE), Inst("stream", 512, 256, "bf16", SLOPE)]
LDX_PAD = 16

Case = namedtuple("Case", "geom inst")

CASES = [Case(g, i) for i in INSTANCES for g in ("nonsquare_a", "past_cap")] + \
        [Case(g, i) for g in ("nonsquare_b", "one_bin", "pixel_bins", "big_bins", "long_list") for i in ROTATION]
OPTION_CASES = [Case("nonsquare_a", i) for i in OPTION_INSTANCES]
TWICE = ("past_cap", "long_list")  # run twice and compared bit for bit


def case_id(c):
    i = c.inst
    return f"{c.geom}-{i.form}-C{i.C}-h{i.hid}-{i.dtype}" + ("" if i.slope == SLOPE else f"-slope{i.slope}")


def form_of(inst):
    """the form the dispatch (dp_plan) gives this instantiation: 'valu', 'reg' or 'stream'"""
    from cyhip import _lib, ops
    p = ops.dense_proj_plan(inst.C, inst.hid, DTYPES[inst.dtype], inst.slope)
    return {_lib.CY_DENSE_PROJ_VALU: "valu", _lib.CY_DENSE_PROJ_MFMA_REG: "reg",
            _lib.CY_DENSE_PROJ_MFMA_STREAM: "stream"}[p["form"]]


# ------------------------------------------------------------------------------------------------ bins
def bin_range(i, L, s):
    """torch's adaptive pooling: [floor(i L / s), ceil((i + 1) L / s))"""
    return (i * L) // s, -((-(i + 1) * L) // s)


def bin_rect(g, i, j):
    r0, r1 = bin_range(i, g.H, g.sh)
    c0, c1 = bin_range(j, g.W, g.sw)
    return r0, r1, c0, c1


@functools.lru_cache(maxsize=None)
def bin_list(name):
    """int32 [nb, 3] = (image, bin row, bin col), or None (all bins in row-major order)"""
    g = GEOMS[name]
    if not g.listed:
        return None
    rows = [(n, i, j) for n in range(g.N) for i in range(g.sh) for j in range(g.sw) if (i + j) % 5 != 0]
    perm = torch.randperm(len(rows), generator=torch.Generator().manual_seed(99))
    return torch.tensor(rows, dtype=torch.int32)[perm].contiguous()


def num_bins(name):
    g = GEOMS[name]
    b = bin_list(name)
    return g.N * g.sh * g.sw if b is None else int(b.shape[0])


def flat_bins(name):
    """rows of the all-bins pooled map [N * sh * sw, .] that the case computes, int64"""
    g = GEOMS[name]
    b = bin_list(name)
    if b is None:
        return torch.arange(g.N * g.sh * g.sw)
    b = b.long()
    return (b[:, 0] * g.sh + b[:, 1]) * g.sw + b[:, 2]


def colour_of(i, j):
    return (i & 1) | ((j & 1) << 1)


@functools.lru_cache(maxsize=None)
def cover(name):
    """int64 [N, H, W]: the number of the case's bins that contain each pixel (all bins: 1, 2 or 4)"""
    g = GEOMS[name]
    b = bin_list(name)
    bins = [(n, i, j) for n in range(g.N) for i in range(g.sh) for j in range(g.sw)] if b is None else b.tolist()
    cnt = torch.zeros(g.N, g.H, g.W, dtype=torch.int64)
    for n, i, j in bins:
        r0, r1, c0, c1 = bin_rect(g, i, j)
        cnt[n, r0:r1, c0:c1] += 1
    return cnt


def num_cells(g):
    """jobs of the all-bins backward of the matrix-core forms: the cells cut out by the bin boundaries"""
    return g.N * (2 * g.sh - 1) * (2 * g.sw - 1)


# ------------------------------------------------------------------------------------------------ inputs and reference
def _seed(c, ldx_pad):
    return 5000 + 7 * (CASES + OPTION_CASES).index(c) + (1 if ldx_pad else 0)


@functools.lru_cache(maxsize=None)
def inputs(c, ldx_pad=0):
    """x [N, H, W, C + ldx_pad] in the storage type (NaN in the padding columns), w1 f32 [hid, C] representable in the
    storage type, b1 f32 [hid], dh f32 [nb, hid] (the upstream gradient of hpool), pre_dw / pre_db (the pre-fill of
    the accumulate option)"""
    g, i = GEOMS[c.geom], c.inst
    T = DTYPES[i.dtype]
    gen = torch.Generator().manual_seed(_seed(c, ldx_pad))
    x = torch.randn(g.N, g.H, g.W, i.C, generator=gen).to(T)
    w1 = (torch.randn(i.hid, i.C, generator=gen) / i.C ** 0.5).to(T).float()
    b1 = torch.randn(i.hid, generator=gen) * 0.5
    for _ in range(40):
        bad = (pre_activation(x, w1, b1).abs() < MARGIN).any(dim=-1)
        if not bad.any():
            break
        x[bad] = torch.randn(int(bad.sum()), i.C, generator=gen).to(T)
    assert not bad.any()
    dh = torch.randn(num_bins(c.geom), i.hid, generator=gen)
    pre_dw = torch.randn(i.hid, i.C, generator=gen)
    pre_db = torch.randn(i.hid, generator=gen)
    if ldx_pad:
        x = torch.cat([x, torch.full((g.N, g.H, g.W, ldx_pad), float("nan"), dtype=T)], dim=-1)
    return dict(x=x, w1=w1, b1=b1, dh=dh, pre_dw=pre_dw, pre_db=pre_db)


def pre_activation(x, w1, b1):
    """float64 [N, H, W, hid] on the operands the kernels multiply"""
    return x[..., :w1.shape[1]].double() @ w1.double().t() + b1.double()


@functools.lru_cache(maxsize=None)
def reference(c, ldx_pad=0):
    """float64: hpool [nb, hid], dx [N, H, W, C], dw1 [hid, C], db1 [hid]"""
    g, i = GEOMS[c.geom], c.inst
    t = inputs(c, ldx_pad)
    x = t["x"][..., :i.C].double().permute(0, 3, 1, 2).requires_grad_(True)
    w1 = t["w1"].double().requires_grad_(True)
    b1 = t["b1"].double().requires_grad_(True)
    a = F.leaky_relu(F.conv2d(x, w1[:, :, None, None], b1), i.slope)
    pooled = F.adaptive_avg_pool2d(a, (g.sh, g.sw))
    rows = pooled.permute(0, 2, 3, 1).reshape(-1, i.hid)[flat_bins(c.geom)]
    (rows * t["dh"].double()).sum().backward()
    return dict(hpool=rows.detach(), dx=x.grad.permute(0, 2, 3, 1).contiguous(), dw1=w1.grad, db1=b1.grad)


def bounds(dtype):
    """the project's bounds against float64, relative to the reference tensor's largest magnitude.  16-bit forms
    (tests/test_gpu_dense_wide.py): exact products and f32 sums forward; the pooled gradient is rounded to 16 bits
    before the dx product and dx is stored in 16 bits.  f32: F32_BAR of tests/test_gpu_dense_options.py."""
    if dtype == "f32":
        return dict(hpool=1e-4, dx=2e-4, dw1=2e-4, db1=2e-4)
    return dict(hpool=1e-4, dx=1e-2, dw1=3e-3, db1=3e-3)


def rel_err(got, want):
    """largest element-wise difference, relative to the reference tensor's largest magnitude"""
    return float((got.double() - want).abs().max() / want.abs().max())


def class_errors(name, got_dx, want_dx):
    """{bins per pixel: rel_err over the pixels that many of the case's bins contain}, for every count >= 1 that
    occurs: a wrong weight at shared pixels cannot hide behind the interior pixels' larger maximum"""
    cnt = cover(name)
    return {int(k): rel_err(got_dx[cnt == k], want_dx[cnt == k]) for k in cnt.unique().tolist() if k >= 1}


# ------------------------------------------------------------------------------------------------ the model with faults
def model(c, fault=None):
    """The same operation written out over bins in float64 (no autograd), so that ONE thing can be made wrong:
      'swap'       sh and sw exchanged in the bin arithmetic (clamped to the map)
      'drop_bin'   pixels shared by four bins get the gradient of three
      'wrong_inv'  at shared pixels every bin's gradient is divided by a neighbour's size
      'drop_tail'  the last partial block of 32 pixels of every bin is left out of the forward sum
    -> hpool, dx as reference().  fault=None reproduces reference() (tests/test_dense_proj_coverage.py checks that)."""
    g, i = GEOMS[c.geom], c.inst
    t = inputs(c)
    pre = pre_activation(t["x"], t["w1"], t["b1"])
    act = torch.where(pre > 0, pre, i.slope * pre)
    der = torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, i.slope))
    dh = t["dh"].double()
    b = bin_list(c.geom)
    bins = [(n, a, j) for n in range(g.N) for a in range(g.sh) for j in range(g.sw)] if b is None else b.tolist()
    sh, sw = (g.sw, g.sh) if fault == "swap" else (g.sh, g.sw)

    def rect(a, j):
        r0, r1 = bin_range(a, g.H, sh)
        c0, c1 = bin_range(j, g.W, sw)
        r0, c0 = min(r0, g.H - 1), min(c0, g.W - 1)
        return r0, max(min(r1, g.H), r0 + 1), c0, max(min(c1, g.W), c0 + 1)

    cnt = cover(c.geom)
    hpool = torch.zeros(len(bins), i.hid, dtype=torch.float64)
    coef = torch.zeros(g.N, g.H, g.W, i.hid, dtype=torch.float64)
    for k, (n, a, j) in enumerate(bins):
        r0, r1, c0, c1 = rect(a, j)
        npx = (r1 - r0) * (c1 - c0)
        px = act[n, r0:r1, c0:c1].reshape(npx, i.hid)
        keep = npx - npx % 32 if fault == "drop_tail" and npx % 32 else npx
        hpool[k] = px[:keep].sum(0) / npx
        w = torch.full((r1 - r0, c1 - c0, 1), 1.0 / npx, dtype=torch.float64)
        if fault == "wrong_inv":  # the size of the bin one step along the shorter axis ratio (a different size: ragged)
            q0, q1, p0, p1 = rect(a + 1 if a + 1 < g.sh else a - 1, j) if g.sh > 1 else rect(a, j)
            shared = (cnt[n, r0:r1, c0:c1] > 1)[..., None]
            w = torch.where(shared, torch.full_like(w, 1.0 / ((q1 - q0) * (p1 - p0))), w)
        if fault == "drop_bin" and colour_of(a, j) == 3:
            w = torch.where((cnt[n, r0:r1, c0:c1] == 4)[..., None], torch.zeros_like(w), w)
        coef[n, r0:r1, c0:c1] += w * dh[k]
    dx = (coef * der) @ t["w1"].double()
    return dict(hpool=hpool, dx=dx)


# ------------------------------------------------------------------------------------------------ pools and gather
PoolCase = namedtuple("PoolCase", "N H W C sh sw dtype listed")

PAST_CAP_MAP = (2, 64, 65, 256)  # 2 129 920 elements: one trip past 8192 blocks x 256 threads


def _pool(name, C, dtype, listed=False):
    g = GEOMS[name]
    return PoolCase(g.N, g.H, g.W, C, g.sh, g.sw, dtype, listed)


AVG_FWD = [_pool(n, C, dt, lst) for dt in ("f32", "bf16", "f16") for n in ("nonsquare_a", "one_bin", "pixel_bins")
           for C, lst in ((8, False), (260, True))] + [_pool("nonsquare_a", 260, "f32"), _pool("nonsquare_a", 8, "bf16", True)]
AVG_BWD = [PoolCase(*PAST_CAP_MAP[:3], PAST_CAP_MAP[3], 7, 9, "bf16", False)] + \
          [_pool(n, 8, dt) for dt in ("f32", "bf16", "f16") for n in ("nonsquare_a", "one_bin", "pixel_bins")]
MAX_CASES = [_pool(n, C, dt) for dt in ("f32", "bf16", "f16") for n, C in (("nonsquare_a", 260), ("pixel_bins", 8))] + \
            [PoolCase(*PAST_CAP_MAP[:3], PAST_CAP_MAP[3], 7, 9, "bf16", False)]
GATHER = [(8200, 257), (300, 1), (1, 257)]  # M, D: 2 107 400 elements (past the cap), one column, one row
GATHER_SPARE = 37                            # rows of the source that are not listed

STORAGE_FORMAT = {"f32": (23, -126), "bf16": (7, -126), "f16": (10, -14)}  # stored mantissa bits, smallest normal exponent


def half_ulp(v, dtype, slack=0.0):
    """half a unit in the last place of the storage type at |v| + slack (float64 tensors): 2^(e - p - 1) with
    e = floor(log2 |v|), not below the smallest normal exponent -- the subnormal range has that one's spacing"""
    p, emin = STORAGE_FORMAT[dtype]
    e = torch.floor(torch.log2((v.abs() + slack).clamp_min(2.0 ** emin)))
    return 2.0 ** (e - p - 1)


def pool_id(p):
    return f"N{p.N}-{p.H}x{p.W}-C{p.C}-s{p.sh}x{p.sw}-{p.dtype}" + ("-list" if p.listed else "")


def pool_bins(p):
    """a seeded list of about half the bins, shuffled; int32 [nb, 3]"""
    rows = [(n, i, j) for n in range(p.N) for i in range(p.sh) for j in range(p.sw)]
    gen = torch.Generator().manual_seed(p.H * 131 + p.C)
    perm = torch.randperm(len(rows), generator=gen)[:max(1, len(rows) // 2)]
    return torch.tensor(rows, dtype=torch.int32)[perm].contiguous()


@functools.lru_cache(maxsize=None)
def avg_inputs(p):
    gen = torch.Generator().manual_seed(p.H * 1000 + p.W * 10 + p.C)
    x = torch.randn(p.N, p.H, p.W, p.C, generator=gen).to(DTYPES[p.dtype])
    dpool = torch.randn(p.N * p.sh * p.sw, p.C, generator=gen)
    return x, dpool


@functools.lru_cache(maxsize=None)
def avg_fwd_reference(p):
    """(rows float64 [nb, C], bound float64 [nb, C]).  The kernel adds a bin's npx values one after the other in f32
    and divides once: |fl(sum) - sum| <= (npx - 1) u sum|x| to first order (u = 2^-24), the division adds u |result|
    <= u mean|x|, so the error of the mean is at most npx u mean|x|; (npx + 1) covers the higher-order terms."""
    x, _ = avg_inputs(p)
    xd = x.double().permute(0, 3, 1, 2)
    rows = F.adaptive_avg_pool2d(xd, (p.sh, p.sw)).permute(0, 2, 3, 1).reshape(-1, p.C)
    mean_abs = F.adaptive_avg_pool2d(xd.abs(), (p.sh, p.sw)).permute(0, 2, 3, 1).reshape(-1, p.C)
    npx = torch.tensor([(bin_range(i, p.H, p.sh)[1] - bin_range(i, p.H, p.sh)[0])
                        * (bin_range(j, p.W, p.sw)[1] - bin_range(j, p.W, p.sw)[0])
                        for _ in range(p.N) for i in range(p.sh) for j in range(p.sw)], dtype=torch.float64)
    bound = (npx[:, None] + 1) * 2.0 ** -24 * mean_abs
    if p.listed:
        b = pool_bins(p).long()
        flat = (b[:, 0] * p.sh + b[:, 1]) * p.sw + b[:, 2]
        rows, bound = rows[flat], bound[flat]
    return rows, bound


@functools.lru_cache(maxsize=None)
def avg_bwd_reference(p):
    """(dx float64 [N, H, W, C], bound).  An element is the f32 sum of at most four terms dpool / |bin|: one rounding
    per division and at most three additions, 4 u sum|terms|, and the store rounds to the storage type (half a unit in
    the last place of the storage type, `half_ulp`)."""
    _, dpool = avg_inputs(p)
    d = dpool.double().reshape(p.N, p.sh, p.sw, p.C).permute(0, 3, 1, 2)

    def back(v):
        x = torch.zeros(p.N, p.C, p.H, p.W, dtype=torch.float64, requires_grad=True)
        (F.adaptive_avg_pool2d(x, (p.sh, p.sw)) * v).sum().backward()
        return x.grad.permute(0, 2, 3, 1).contiguous()

    dx, terms = back(d), back(d.abs())
    f32_sum = 4 * 2.0 ** -24 * terms  # (the unit is taken where the f32 sum may lie: it can cross into the next binade)
    return dx, f32_sum + half_ulp(dx, p.dtype, f32_sum)


MAX_LEVELS = (-1.0, -0.5, 0.0, 0.5, 1.0)


@functools.lru_cache(maxsize=None)
def max_inputs(p):
    """x with five distinct values (nearly every bin has ties), the upstream gradient small integers over 8: every sum
    of up to four of them is exact in f32, bf16 and f16"""
    gen = torch.Generator().manual_seed(p.H * 77 + p.C)
    x = torch.tensor(MAX_LEVELS)[torch.randint(0, 5, (p.N, p.H, p.W, p.C), generator=gen)].to(DTYPES[p.dtype])
    dpool = torch.randint(-4, 5, (p.N * p.sh * p.sw, p.C), generator=gen).float() / 8
    return x, dpool


@functools.lru_cache(maxsize=None)
def max_reference(p, last=False):
    """F.adaptive_max_pool2d(return_indices=True) on the stored values: rows f32 [nb, C], arg int32 [nb, C] (pixel
    h * W + w inside the image, the FIRST maximum in row-major order), dx f32 [N, H, W, C] by autograd.
    last=True is the faulty model of the sensitivity check: the LAST maximum on ties."""
    x, dpool = max_inputs(p)
    xd = x.double().permute(0, 3, 1, 2)
    if last:
        xd = xd.flip(2, 3)
    xd = xd.contiguous().requires_grad_(True)
    out, idx = F.adaptive_max_pool2d(xd, (p.sh, p.sw), return_indices=True)
    if last:  # bins mirror onto bins (floor and ceil exchange), so flipping the pooled map back gives the same values
        out, idx = out.flip(2, 3), (p.H * p.W - 1 - idx).flip(2, 3)
    d = dpool.double().reshape(p.N, p.sh, p.sw, p.C).permute(0, 3, 1, 2)
    (out * d).sum().backward()
    dx = xd.grad.flip(2, 3) if last else xd.grad
    rows = out.detach().permute(0, 2, 3, 1).reshape(-1, p.C).float()
    arg = idx.permute(0, 2, 3, 1).reshape(-1, p.C).to(torch.int32)
    return rows, arg, dx.permute(0, 2, 3, 1).contiguous().float()


@functools.lru_cache(maxsize=None)
def gather_inputs(M, D):
    gen = torch.Generator().manual_seed(M * 3 + D)
    R = M + GATHER_SPARE
    src = torch.randn(R, D, generator=gen)
    idx = torch.randperm(R, generator=gen)[:M].to(torch.int32)
    dout = torch.randn(M, D, generator=gen)
    return src, idx, dout


# ------------------------------------------------------------------------------------------------ head level
HEAD_MAPS = [(32, "bf16"), (256, "bf16"), (16, "f32")]
HEAD_POOLS = ("adaptive_avg", "adaptive_max", "identical", "none", None)
HEAD_TYPES = ("mlp", "linear")
HEAD_HIDDEN, HEAD_OUT = 128, 24
