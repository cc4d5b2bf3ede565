"""Case tables of tests/test_gpu_pica_stream.py: the streaming and finishing kernels of csrc/cy_pica.hip (PUILoss,
PUISegLoss, JSD_div, EntropyPrior) past every launch cap, at their maxima and on every branch that the goldens of
tests/test_gpu_patch_losses.py do not reach.  Each case carries a note saying what it reaches;
tests/test_pica_stream_coverage.py checks the notes' claims on the CPU.

The sizes are too large for an npz, so the inputs come from a seeded `torch.Generator` and the references are the f64
formulas of tests/patch_losses_cases.py (`pui64`, `puiseg64`, `jsd64`, `prior64`).

Tolerance (the rule of tests/patch_losses_fixture.py): the bound of a kind is max(4 * e_ref, 1e-6), e_ref the larger of
the fixture's stored e_ref of that kind and the case's own distance between the f64 formula and the same formula run in
f32 on the CPU (`own_distances`): the reference's error on the case, never the kernel's.
"""
import zlib
from collections import namedtuple

import numpy as np
import torch

import patch_losses_cases as pc
import patch_losses_fixture as fx

# ---------------------------------------------------------------------------------------------- the launch rule
STREAM_GRID_CAP = 1024           # csrc/cy_pica.hip
PK_KMAX, JSD_MMAX = 64, 8
ONE_TRIP = STREAM_GRID_CAP * 256  # positions one trip of a capped grid covers
SIDE = 513                        # 513 * 513 = one trip + four full blocks + one item
PAST_CAP = SIDE * SIDE
EPS = fx.EPS
PUI_LAMDA = fx.PUI_LAMDA


def cy_blocks(items, per_block, cap):
    """csrc/cy_common.h: blocks of `per_block` items for `items`, at least 1, at most `cap`"""
    return max(1, min(cap, -(-items // per_block)))


def trips(items, cap=STREAM_GRID_CAP):
    """how often the grid-stride loop of a kernel launched by cy_blocks(items, 256, cap) goes round"""
    return -(-items // (cy_blocks(items, 256, cap) * 256))


def last_owner(items, cap=STREAM_GRID_CAP):
    """(trip, block, thread) of the last item"""
    span = cy_blocks(items, 256, cap) * 256
    e = items - 1
    return e // span, (e % span) // 256, e % 256


def gen_of(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def simplex(shape, g, scale=2.0):
    return torch.softmax(torch.randn(*shape, generator=g) * scale, 1)


# ---------------------------------------------------------------------------------------------- JSD_div
# needs: the maps a gradient is requested on (None: all); kind: how the maps are drawn
Jsd = namedtuple("Jsd", "name m shape fmt reduction needs kind note")
ZERO_CLASS, ZERO_BOTH, ZERO_ONE = 1, slice(0, 100), slice(100, 150)  # image rows of the exact zeros

JSD_CASES = (
    Jsd("cap_nchw_none", 3, (1, 4, SIDE, SIDE), "nchw", "none", None, "simplex",
        "past cap, S > 1: out_map and the per-position upstream gradient across the second trip"),
    Jsd("cap_nhwc_mean", 2, (1, 4, SIDE, SIDE), "nhwc", "mean", None, "simplex",
        "past cap, channels_last (S = 1), block partials of two trips, 1 / R"),
    Jsd("cap_rows_sum", 2, (PAST_CAP, 3), "rows", "sum", None, "simplex", "past cap on [R,C] rows, reduction sum"),
    Jsd("cap_zeros", 2, (1, 4, SIDE, SIDE), "nchw", "sum", None, "zeros",
        "past cap; class 1 exactly 0 in both maps on image rows 0..99 (the mean is exactly 0), and in map 0 only on "
        "rows 100..149"),
    Jsd("m8_none", 8, (2, 64, 5, 7), "nchw", "none", (0, 5), "simplex",
        "m = JSD_MMAX, C = PK_KMAX; gradients on maps 0 and 5 only: skipped maps between the two and after them"),
    Jsd("m8_sum", 8, (2, 64, 5, 7), "nhwc", "sum", (0, 5), "simplex", "the same maps channels_last, reduction sum"),
    Jsd("c1", 2, (2, 1, 9, 7), "nchw", "mean", None, "positive",
        "C = 1; positive maps in [0.05, 1], not a simplex (a one-class simplex has JSD 0)"),
    Jsd("rows_1", 2, (1, 5), "rows", "none", None, "simplex", "R = 1: one live thread"),
    Jsd("rows_255", 2, (255, 5), "rows", "mean", None, "simplex", "R = 255: one block, its last thread idle"),
    Jsd("rows_256", 2, (256, 5), "rows", "sum", None, "simplex", "R = 256: exactly one block"),
    Jsd("rows_257", 2, (257, 5), "rows", "none", None, "simplex", "R = 257: a second block of one position"),
)


def jsd_positions(c):
    return c.shape[0] * int(np.prod(c.shape[2:]))


def jsd_inputs(c):
    g = gen_of("jsd_" + c.name)
    if c.kind == "positive":
        return [0.05 + 0.95 * torch.rand(*c.shape, generator=g) for _ in range(c.m)]
    xs = [simplex(c.shape, g) for _ in range(c.m)]
    if c.kind == "zeros":
        for x in xs:
            x[:, ZERO_CLASS, ZERO_BOTH] = 0.0
        xs[0][:, ZERO_CLASS, ZERO_ONE] = 0.0
    return xs


def jsd_formula(c):
    return lambda xs: pc.jsd64(xs, c.reduction, EPS)


# ---------------------------------------------------------------------------------------------- EntropyPrior
Prior = namedtuple("Prior", "name shape given kind note")
PRIOR_CASES = (
    Prior("cap_given", (PAST_CAP, 2), True, "simplex",
          "forward (R) and backward (R * C) both past the cap; given prior"),
    Prior("bwd_cap_k64", (4100, 64), False, "simplex",
          "forward 17 blocks; backward 262 400 elements = one trip + 256: past the cap; C = PK_KMAX, uniform prior"),
    Prior("c1", (300, 1), False, "positive", "C = 1 on positive rows"),
    Prior("r1", (1, 5), True, "simplex", "R = 1"),
)


def prior_inputs(c):
    """-> (x [R,C], prior [1,C] or None)"""
    g = gen_of("prior_" + c.name)
    x = 0.05 + 0.95 * torch.rand(*c.shape, generator=g) if c.kind == "positive" else simplex(c.shape, g)
    prior = simplex((1, c.shape[1]), g, 1.0) if c.given else None
    return x, prior


def prior_formula(prior):
    return lambda xs: pc.prior64(xs[0], None if prior is None else prior.to(xs[0].dtype), EPS)


# ---------------------------------------------------------------------------------------------- PUILoss
# rows are softmax times a per-row factor from [0.5, 1.5]: the port drops the reference's simplex assertion
Pui = namedtuple("Pui", "name N K column note")
CLAMPED_COLUMN = 2
PUI_CASES = (
    Pui("4100x64", 4100, 64, None,
        "rows_axpb_kernel past its cap (N * K = one trip + 256), with b (dx) and without (dy); K = PK_KMAX"),
    Pui("5x33", 5, 33, None, "nsl = 7 slices, 231 live threads of pui_stats_kernel"),
    Pui("3x2", 3, 2, None, "N smaller than the number of slices (128)"),
    Pui("clamped_300x6", 300, 6, 0.0, "y[:, 2] = 0: the column norm is clamped at 1e-12, gb = 0"),
    Pui("tiny_300x6", 300, 6, 1e-14,
        "y[:, 2] = 1e-14: the norm 1.7e-13 is clamped too, but the column's joint is not 0, so that a gb computed "
        "through the clamp would differ"),
)


def pui_inputs(c):
    g = gen_of("pui_" + c.name)
    x, y = (simplex((c.N, c.K), g) * (0.5 + torch.rand(c.N, 1, generator=g)) for _ in range(2))
    if c.column is not None:
        y[:, CLAMPED_COLUMN] = c.column
    return [x, y]


def pui_formula(xs):
    return pc.pui64(xs[0], xs[1], PUI_LAMDA)


# ---------------------------------------------------------------------------------------------- PUISegLoss
# runs: (memory format, (gradient on x1, gradient on x2)) of the GPU test
BOTH, X1_ONLY, X2_ONLY = (True, True), (True, False), (False, True)
Seg = namedtuple("Seg", "name shape pad lamda runs note")
SMALL_RUNS = (("nchw", BOTH), ("nhwc", BOTH))
SEG_CASES = (
    Seg("cap", (1, 2, SIDE, SIDE), 1, 2.0, (("nchw", BOTH),), "pixmean_entropy_fwd/bwd_kernel past the cap"),
    Seg("tt289", (1, 2, 20, 20), 8, 2.0, SMALL_RUNS, "T*T = 289 > 256: the displacement loop's second pass"),
    Seg("k64", (1, 64, 6, 5), 1, 2.0, SMALL_RUNS, "k = PK_KMAX: all diag[] and dP[] entries live, k*k = 4096"),
    Seg("lam0", (2, 5, 13, 11), 2, 0.0, SMALL_RUNS, "lamda = 0: value and dx1 are the ce term alone"),
    Seg("lam2", (2, 5, 13, 11), 2, 2.0, SMALL_RUNS + (("nchw", X1_ONLY), ("nchw", X2_ONLY)),
        "the input of lam0 with lamda = 2: value and dx1 dominated by the balance term; one-sided gradients"),
)
SEG_INPUT_OF = {"lam2": "lam0"}  # the two share their input


def seg_inputs(c):
    """softmax times a per-pixel factor from [0.5, 1.5], both ends present: the per-pixel class mean is factor / k"""
    g = gen_of("seg_" + SEG_INPUT_OF.get(c.name, c.name))
    n, k, H, W = c.shape
    out = []
    for _ in range(2):
        f = 0.5 + torch.rand(n, 1, H, W, generator=g)
        f.view(-1)[0], f.view(-1)[-1] = 0.5, 1.5
        out.append(simplex(c.shape, g) * f)
    return out


def seg_formula(c, lamda=None):
    lam = c.lamda if lamda is None else lamda
    return lambda xs: pc.puiseg64(xs[0], xs[1], lam, c.pad)


def pixel_mean_spread(x):
    """max / min of the per-pixel class mean of a [n,k,H,W] map"""
    pm = x.double().mean(1)
    return float(pm.max() / pm.min())


# one past-cap case of each loss for "two runs give the same bits"
SAME_BITS = {"jsd": "cap_nchw_none", "prior": "cap_given", "pui": "4100x64", "seg": "cap"}


def by_name(cases, name):
    hit = [c for c in cases if c.name == name]
    assert len(hit) == 1, (name, [c.name for c in cases])
    return hit[0]


# ---------------------------------------------------------------------------------------------- references, tolerances
def reference32(fn, ps):
    """pc.reference with f32 leaves: the same formula at the precision of the reference's own f32 run"""
    xs = [p.float().clone().requires_grad_(True) for p in ps]
    v = fn(xs)
    (v if v.dim() == 0 else (v * fx.none_weights(v)).sum()).backward()
    return v.detach(), [x.grad for x in xs]


def own_distances(ref32, ref64):
    """-> (value distance, [[2-norm, max-norm] per gradient]) of the f32 formula from the f64 one"""
    return fx.rel_vec(ref32[0], ref64[0]), [fx.rel_grad(a, b) for a, b in zip(ref32[1], ref64[1])]


def fixture_e_ref(npz):
    """kind -> the largest stored e_ref of tests/golden/patch_losses.npz (what fx.tolerances multiplies by 4)"""
    worst = np.max(np.stack([v for k, v in npz.items() if k.endswith("_e_ref")]), axis=0)
    return dict(zip(fx.KINDS, (float(w) for w in worst)))


def bound(stored, own):
    return max(4.0 * max(stored, own), 1e-6)


def tolerances(stored, own_value, own_grad):
    """the tolerance dict of pc.check_value / pc.check_grad for one gradient of a case"""
    return {"scalar": bound(stored["scalar"], own_value), "grad2": bound(stored["grad2"], own_grad[0]),
            "gradmax": bound(stored["gradmax"], own_grad[1])}
