"""The cases tests/test_gpu_norm_act_dispatch.py is parametrised with, and what tests/test_norm_act_plan_coverage.py
requires of them: the BatchNorm, pool and upsample kernels of csrc/cy_norm_act.hip (with cy_bn_acc.h).  A plain module
(no GPU, no library call at import): the GPU tests and the CPU guard read the launch plan of a case through the same
host-side query, cyhip.ops.norm_act_plan.

Every shape is the smallest that reaches its branch; none is a shape of the benchmark.  Types are named by strings
("bf16", "f16", "f32") so that nothing here needs torch."""
from collections import namedtuple

TYPES = ("bf16", "f16", "f32")

# ---------------------------------------------------------------- backward reduce: pixels x channels
# cy_bn_relu_bwd_reduce and _reduce_acc over `npix` pixels of C channels
ReduceCase = namedtuple("ReduceCase", "npix C dtype note")

ONE_WG = 31            # one workgroup
LAST_32 = 16352        # last count on 32-pixel workgroups (511 of them)
FIRST_511 = 16353      # first count on the 511-workgroup plateau: 33 pixels each, 15 workgroups empty
LAST_511 = 65408       # last count on 511 workgroups (128 pixels each): the last deep launch
FIRST_SHALLOW = 65409  # first non-deep count: 512 workgroups of 128 pixels
LAST_UNCAPPED = 131072 # last count under the cap: 1024 workgroups of 128 pixels
PAST_CAP = 131073      # past the cap: 129 pixels each, 7 workgroups empty
REDUCE_PIXELS = (ONE_WG, LAST_32, FIRST_511, LAST_511, FIRST_SHALLOW, LAST_UNCAPPED, PAST_CAP)
# C: 8 = 256 pixel rows (more rows than pixels per workgroup); 40 = five groups, thread 255 idle; 64 = eight groups;
# 512 = four rows; 2048 = one row, 256 groups per page; 2056 = two pages, the second with one group
REDUCE_CHANNELS = (8, 40, 64, 512, 2048, 2056)

REDUCE_CASES = (
    # every channel count on one workgroup (the products with the large pixel counts stay at C <= 64)
    [ReduceCase(ONE_WG, C, "bf16", "one workgroup") for C in REDUCE_CHANNELS]
    + [ReduceCase(ONE_WG, 40, "f16", "one workgroup"), ReduceCase(ONE_WG, 512, "f32", "one workgroup, 4-pixel round"),
       ReduceCase(ONE_WG, 2056, "f32", "two pages"),
       # a few workgroups: rows of 4 and of 1 pixel walk the 4-pixel round, then the tail; the last workgroup is short
       ReduceCase(1000, 512, "f16", "deep, 32 workgroups, round and tail"),
       ReduceCase(333, 2056, "bf16", "deep, 11 workgroups, two pages")]
    # both sides of the three boundaries, at the smallest C
    + [ReduceCase(n, 8, "bf16", "boundary") for n in REDUCE_PIXELS[1:]]
    + [ReduceCase(FIRST_511, 8, "f32", "15 empty workgroups"), ReduceCase(FIRST_511, 40, "bf16", "15 empty, idle thread"),
       ReduceCase(FIRST_511, 8, "f16", "15 empty workgroups"),
       ReduceCase(FIRST_SHALLOW, 8, "f16", "first non-deep"), ReduceCase(FIRST_SHALLOW, 64, "bf16", "non-deep, 8 groups"),
       ReduceCase(PAST_CAP, 8, "f32", "7 empty workgroups"), ReduceCase(PAST_CAP, 64, "bf16", "past the cap, 8 groups")])

# ---------------------------------------------------------------- elementwise kernels, small geometry
# One case runs every elementwise launch on [N, H, W, C] (H, W even; the pooled / low-resolution map is H/2 x W/2):
# the applies (plain, pooled, both on coefficients and on an accumulator), the backward applies, the pool and upsample
# backward and their fused-sum forms.  `mixed`: also the apply that reads `dtype` and writes f32.
EwCase = namedtuple("EwCase", "N H W C dtype mixed")
SMALL = (3, 6, 10)  # N = 3; H != W; pooled 3 x 5, both odd
EW_CASES = (
    [EwCase(*SMALL, C, dt, False) for C in (8, 40, 1024) for dt in TYPES]
    + [EwCase(*SMALL, 24, "bf16", True), EwCase(*SMALL, 24, "f16", True), EwCase(*SMALL, 24, "f32", False)])
# C/8 of 3 and 5 do not divide 256: the fused pool / upsample forms must say so, and the unfused kernel runs
FUSED_REFUSED_C = (24, 40)

# ---------------------------------------------------------------- capped grid-stride loops (bf16 only)
# (N, H, W) are in the unit of the kinds: pixels for apply / bwd_apply, pooled dims for the pool kinds, low-resolution
# dims for the upsample kinds.  Each is within 5 % above the smallest count that gives a second trip
# (plan["one_trip_items"] + 1 items of 8 channels).
BigCase = namedtuple("BigCase", "name kinds N H W C fold")
BIG_CASES = (
    BigCase("plain-c512", ("apply", "bwd_apply", "pool_bwd", "up_bwd"), 1, 181, 182, 512, 0),
    BigCase("plain-c40-not-pow2", ("bwd_apply",), 1, 648, 648, 40, 0),
    BigCase("fold-c1024", ("apply", "bwd_apply"), 1, 45, 46, 1024, 2),
    BigCase("fold-c8", ("apply", "bwd_apply"), 1, 512, 513, 8, 32),
    BigCase("pooled-apply-c512", ("apply_pool",), 1, 181, 182, 512, 0),
    BigCase("pooled-apply-fold-c1024", ("apply_pool",), 1, 45, 46, 1024, 2),
    BigCase("fused-sums-c512", ("pool_bwd_bn", "up_bwd_bn"), 1, 64, 65, 512, 4),
)

# ---------------------------------------------------------------- accumulator consumers on their own
# replica counts: direct gathers 1, 2, 4, 8; wide direct 16, 32 (elementwise kernels; LDS atomics in bn_fold_kernel);
# LDS atomics 64
FOLD_RS = (1, 2, 4, 8, 16, 32, 64)
FOLD_KINDS = ("fold_coef", "apply", "apply_pool", "bwd_apply")
FOLD_GEOM = (3, 10, 14, 40)  # N, H, W, C: 2100 items, three workgroups of 1024 threads (leader and two others)

# ---------------------------------------------------------------- finalize
FINALIZE_P = (1, 256, 257)          # bn_finalize_kernel strides 256 partial rows
BWD_FINALIZE_P = (1, 64, 65, 1024)  # bn_bwd_finalize_kernel strides 64
FINALIZE_C = 10       # three workgroups of four channels, the last half empty
BWD_FINALIZE_C = 24
RUNNING_LAYERS, RUNNING_C = 33, 264  # two launches (32 + 1 layers), two trips over the channels


def ew_kinds(c):
    """(kind, N, H, W, fold) of every launch an EwCase makes (fold = the replica count the test uses)"""
    N, H, W = c.N, c.H, c.W
    h, w = H // 2, W // 2
    return [("apply", N, H, W, 0), ("apply", N, H, W, 2), ("apply_pool", N, h, w, 0), ("apply_pool", N, h, w, 2),
            ("bwd_reduce", N, H, W, 0), ("bwd_apply", N, H, W, 0), ("bwd_apply", N, H, W, 2),
            ("pool_bwd", N, h, w, 0), ("pool_bwd_bn", N, h, w, 1), ("up_bwd", N, h, w, 0), ("up_bwd_bn", N, h, w, 1)]


def case_id(c):
    if isinstance(c, ReduceCase):
        return f"{c.npix}px-c{c.C}-{c.dtype}"
    if isinstance(c, EwCase):
        return f"{c.N}x{c.H}x{c.W}-c{c.C}-{c.dtype}" + ("-mixed" if c.mixed else "")
    return c.name


def torch_dtype(name):
    import torch
    return {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[name]


def plan(kind, N, H, W, C, dtype="bf16", fold=0, out_dtype=None):
    from cyhip import ops
    return ops.norm_act_plan(kind, N, H, W, C, torch_dtype(dtype), fold,
                             None if out_dtype is None else torch_dtype(out_dtype))


def reduce_plan(c, fold=0):
    return plan("bwd_reduce", 1, 1, c.npix, c.C, c.dtype, fold)
