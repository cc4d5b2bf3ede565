"""The cases tests/test_gpu_unet2_dispatch.py is parametrised with, and what tests/test_unet2_plan_coverage.py requires of
them: the kernels of the second backbone, csrc/cy_groupnorm.hip (GroupNorm + SiLU, modulation, bilinear resize) and
csrc/cy_unet2.hip (strided GEMM, im2col / col2im, column sums, channel LayerNorm, softmaxes, activations, embedding).
A plain module: no GPU, no torch and no library call at import.

Every shape is the smallest that reaches its branch.  Slice counts are never restated here: the coverage file reads
them from the library's workspace queries.  What the library does not export (the GroupNorm reduction geometry, the
three block caps, the GEMM loader choice) is restated below FOR COVERAGE ONLY, next to a pointer at its source line;
no expected value of the GPU file comes from it.

Long reductions carry their tolerance in the table: `yardstick` is the error (relative to max|ref|) of torch's own f32
CPU operator against the float64 reference on the same input, measured once with the `yardstick_*` functions of the
GPU file; `bound` = max(4 * yardstick, the project's small-size number).  4x covers another, equally valid summation
order without hiding a dropped slice (1/512 of a column sum, 1/256 of a softmax denominator, 1/64 of a split-K sum)."""
from collections import namedtuple

TYPES = ("f32", "bf16", "f16")
# 16-bit outputs: the unit roundoff of the storage type bounds one rounding relative to the value, so relative to
# max|ref|; the f32 bound of the kernel is added to it
ROUND = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}

# the project's small-size numbers (tests/test_gpu_unet2_glue.py, tests/test_gpu_next_rows.py, test_gpu_round4_rows.py)
TOL_GEMM_FWD, TOL_GEMM_GRAD = 2e-5, 3e-5
TOL_LN = 5e-5
TOL_SOFTMAX, TOL_ATTN_GRAD = 3e-5, 1e-4
TOL_GN = 2e-4
TOL_ACT = 1e-5

# ---------------------------------------------------------------- restated launch geometry (coverage only)
GN_SPLIT = 32          # cy_groupnorm.hip: constexpr int GN_SPLIT
GN_GRID_CAP = 8192     # cy_groupnorm.hip: `constexpr int GRID_CAP = 8192;`, cy_blocks(items, 256, GRID_CAP)
U2_GRID_CAP = 16384    # cy_unet2.hip: `constexpr int GRID_CAP = 16384;`, cy_blocks(items, 256, GRID_CAP)
ACT_GRID_CAP = 4096    # cy_unet2.hip: cy_act_fwd / cy_act_bwd, `b > 4096 ? 4096 : b`
SLICE_CAP = 512        # cy_unet2.hip: slices_for(); only used to NAME the cap, the count comes from *_ws_bytes
COL_SLICE_CAP = 256    # cy_unet2.hip: col_slices(); likewise
GEMM_KSTEP = 16        # cy_unet2.hip: cy_gemm_strided rounds the K chunk of a split up to the LDS stage of 16


def gn_geometry(C, HW):
    """cy_groupnorm.hip, channel_reduce(): gpp 8-channel groups x `rows` pixel lanes per workgroup, GN_SPLIT pixel splits
    per image of `per` pixels; a lane walks its split 4 pixels per round (`q + 3 * rows < q1`), then one at a time."""
    gpp = min(C // 8, 256)
    rows = 256 // gpp
    per = -(-HW // GN_SPLIT)
    round_any = tail_any = both_any = False
    empty = 0
    for s in range(GN_SPLIT):
        q0, q1 = s * per, min(HW, s * per + per)
        if q1 <= q0:
            empty += 1
            continue
        for prow in range(rows):
            q, rounds = q0 + prow, 0
            while q + 3 * rows < q1:
                q, rounds = q + 4 * rows, rounds + 1
            tail = q < q1
            round_any |= rounds > 0
            tail_any |= tail
            both_any |= rounds > 0 and tail
    return {"gpp": gpp, "rows": rows, "idle_threads": 256 - gpp * rows, "per": per, "empty_splits": empty,
            "round": round_any, "tail": tail_any, "both": both_any}


def gemm_loader(la, lb):
    """cy_unet2.hip, cy_gemm_strided(): `am = la->rs == 1 && la->cs != 1, bn = lb->cs == 1` -> <A_MFAST, B_NFAST>"""
    return (la[0] == 1 and la[1] != 1, lb[1] == 1)


def gemm_kranges(K, ksplit):
    """cy_unet2.hip, cy_gemm_strided(): kchunk = ceil(K / ksplit) rounded up to 16; split s covers [s*kchunk, +kchunk) & K"""
    kchunk = -(-(-(-K // ksplit)) // GEMM_KSTEP) * GEMM_KSTEP
    return [(min(K, s * kchunk), min(K, s * kchunk + kchunk)) for s in range(ksplit)]


# ---------------------------------------------------------------- GroupNorm + SiLU
# `fill`: "randn" or "const" (every value 1.5 with a bias of 0.25: u = 1.75 and u*u are exact, the variance is exactly 0)
GnShape = namedtuple("GnShape", "name N HW C G fill")
GN_SHAPES = (
    GnShape("one-channel-per-group", 2, 5, 8, 8, "randn"),     # rows = 256, HW below rows and below GN_SPLIT: 27 empty splits
    GnShape("zero-variance", 1, 1, 8, 1, "const"),
    GnShape("three-groups-idle-thread", 2, 169, 24, 3, "randn"),  # gpp = 3, rows = 85, thread 255 idle
    GnShape("round-then-tail", 2, 81 * 81, 40, 8, "randn"),    # rows = 51, split length 206: one 4-pixel round, then a tail
    GnShape("host-limits", 1, 150, 2048, 8, "randn"),          # C = 2048 and C / G = 256, rows = 1, round and tail
    GnShape("round-only", 3, 4096, 64, 8, "randn"),            # rows = 32, split length 128 = one round of 4 x 32, no tail
    GnShape("tail-only", 3, 128, 64, 8, "randn"),              # rows = 32, split length 4: the round never runs
)
GN_STRIDED = GnShape("strided-rows", 2, 169, 24, 3, "randn")   # ldy = C + 8, ldo = C + 16, ldd = C + 24, ldu = C + 8
GN_STRIDES = {"ldy": 8, "ldo": 16, "ldd": 24, "ldu": 8}
GN_GRADS = GnShape("gradient-outputs", 3, 37, 16, 2, "randn")  # accumulate, null outputs, per-image modulation (N = 3)
# which of (dgamma, dbeta, dbias) are passed; every set runs plain and modulated, the modulated one also with
# dmod_scale / dmod_shift null
GN_NULL_SETS = ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0))
# past the apply grid cap: N * HW * C / 8 = 2 101 248 items of 8 channels > 8192 * 256 and no multiple of it
GN_CAP = GnShape("past-apply-cap", 1, 513 * 512, 64, 8, "randn")
# per-channel mean 30 standard deviations from zero through the conv bias (bias = 30 + 0.5 randn): the variance is
# E[u^2] - mean^2.  yardstick: F.group_norm + F.silu in f32 on the CPU (out, du); measured 1.1e-6 / 1.4e-6
GN_OFFSET = GnShape("offset-30-sigma", 2, 1000, 32, 4, "randn")
GN_OFFSET_YARDSTICK = {"out": 1.1e-6, "du": 1.4e-6}
GN_OFFSET_BOUND = {"out": TOL_GN, "du": TOL_GN}  # 4 x yardstick is under the small-size number, which holds

# ---------------------------------------------------------------- strided GEMM
# variant name -> (A_MFAST, B_NFAST).  "N" = row-major as the product reads it, "T" = stored transposed.  A transposed
# A is stored with a leading dimension of M + 3 so that M = 1 still has cs != 1 (the loader choice looks at the strides)
GEMM_VARIANTS = {"AmBn": (True, True), "AmBk": (True, False), "AkBn": (False, True), "AkBk": (False, False)}
GEMM_SIZES = ((65, 63, 17), (64, 64, 16), (1, 1, 3))
# K >= 2048 and 2 tiles: _auto_ksplit gives 4.  yardstick: torch f32 CPU matmul; measured 4.2e-7
GEMM_LONG = (65, 63, 2051)
GEMM_LONG_YARDSTICK = 4.2e-7
GEMM_LONG_BOUND = TOL_GEMM_FWD
GemmSplit = namedtuple("GemmSplit", "name M N K ksplit variant")
GEMM_SPLITS = (
    GemmSplit("last-split-one-element", 65, 63, 33, 3, "AkBn"),
    GemmSplit("last-split-empty", 65, 63, 32, 3, "AmBk"),
)
# bias + alpha + accumulate + 3 x 2 batches + split-K, A and C column slices of wider matrices
GEMM_COMBINED = {"nb1": 3, "nb2": 2, "M": 50, "N": 8, "K": 40, "ksplit": 3, "alpha": 0.5, "a_off": 16, "a_pad": 16,
                 "c_off": 4, "ldc": 40}


def gemm_layouts(variant, M, N, K):
    """(la, lb, A storage shape, B storage shape): la / lb = (rs, cs, 0, 0)"""
    am, bn = GEMM_VARIANTS[variant]
    la, sa = ((1, M + 3, 0, 0), (K, M + 3)) if am else ((K, 1, 0, 0), (M, K))
    lb, sb = ((N, 1, 0, 0), (K, N)) if bn else ((1, K, 0, 0), (N, K))
    return la, lb, sa, sb


# ---------------------------------------------------------------- im2col / col2im
ConvGeom = namedtuple("ConvGeom", "name N H W C Cout K stride pad")
# (H + 2 pad - K) % stride != 0.  The first leaves the bottom / right PADDING unused; the second leaves the last input
# row and column outside every window: their dx is exactly 0
CONV_RAGGED = (
    ConvGeom("h10-k3-s2-p1", 2, 10, 12, 5, 7, 3, 2, 1),
    ConvGeom("h12-w9-k3-s3-p1", 2, 12, 9, 5, 7, 3, 3, 1),
)
# the patch matrix has 242 * 241 * 9 * 8 = 4 199 184 elements > 16384 * 256
IM2COL_CAP = ConvGeom("im2col-past-cap", 1, 242, 241, 8, 4, 3, 1, 1)
# the col2im output has 648 * 648 * 10 = 4 199 040 elements > 16384 * 256 (patch matrix 324 * 324 * 90, 38 MB)
COL2IM_CAP = ConvGeom("col2im-past-cap", 1, 648, 648, 10, 0, 3, 2, 1)
CONVT_CASES = (ConvGeom("convT-4x4-s2", 2, 5, 7, 6, 10, 4, 2, 1),)


def conv_out(g):
    return (g.H + 2 * g.pad - g.K) // g.stride + 1, (g.W + 2 * g.pad - g.K) // g.stride + 1


# ---------------------------------------------------------------- column sums and channel LayerNorm
RowsCase = namedtuple("RowsCase", "M N")
ROWS_CASES = (RowsCase(1, 1), RowsCase(1, 257), RowsCase(256, 8), RowsCase(257, 257), RowsCase(131072, 8),
              RowsCase(131073, 1), RowsCase(131073, 8))
ROWS_M = (1, 256, 257, 131072, 131073)
ROWS_N = (1, 8, 257)
LONG_M = 131073
# yardsticks on M = 131073 (N = 8): torch f32 CPU sum(0) 4.2e-8; F.layer_norm and its autograd y 1.6e-7, dx 1.9e-7, dg 2.2e-6,
# db 3.7e-6
COLSUM_LONG_YARDSTICK = 4.2e-8
COLSUM_LONG_BOUND = TOL_GEMM_GRAD
LN_LONG_YARDSTICK = {"y": 1.6e-7, "dx": 1.9e-7, "dg": 2.2e-6, "db": 3.7e-6}
LN_LONG_BOUND = TOL_LN

# ---------------------------------------------------------------- softmaxes
HeadCase = namedtuple("HeadCase", "name M heads dh ld off")
HEAD_CASES = (
    HeadCase("past-cap", 1048601, 4, 2, 8, 0),     # M * heads = 4 194 404 > 16384 * 256; runs first
    HeadCase("offset-padded", 300, 3, 5, 24, 4),   # off > 0, ld > off + heads * dh
    HeadCase("dh-1", 70, 4, 1, 8, 2),
)
ColCase = namedtuple("ColCase", "name B n Ch ld off")
COL_CASES = (
    ColCase("past-cap-n32769", 1, 32769, 129, 129, 0),   # B * n * Ch = 4 227 201 > 16384 * 256; 256 slices, the last empty
    ColCase("n32768", 2, 32768, 8, 16, 5),
    ColCase("n1", 3, 1, 257, 260, 3),
    ColCase("n128", 3, 128, 8, 8, 0),
    ColCase("n129-ch257", 3, 129, 257, 264, 7),
)
COL_N = (1, 128, 129, 32768, 32769)
# yardstick on n = 32769: torch f32 CPU softmax over the positions; measured 4.5e-6
COL_LONG_YARDSTICK = 4.5e-6
COL_LONG_BOUND = TOL_SOFTMAX
ROW_N = (1, 255, 256, 257, 784, 1000)
ROW_ROWS = 5
# module level.  LinearAttentionFn: one image of 182 x 181 = 32 942 positions (257 column-softmax slices capped to 256;
# the context GEMM has K = 32 942 and one tile per batch: _auto_ksplit gives 64).  yardstick: the same expressions in
# f32 on the CPU; measured fwd 4.0e-7, dqkv 5.8e-7
LINATTN_LONG = {"N": 1, "H": 182, "W": 181, "heads": 1, "dh": 8}
LINATTN_LONG_YARDSTICK = {"out": 4.0e-7, "dqkv": 5.8e-7}
LINATTN_LONG_BOUND = {"out": TOL_SOFTMAX, "dqkv": TOL_ATTN_GRAD}
ATTN_784 = {"N": 1, "H": 28, "W": 28, "heads": 2, "dh": 8}

# ---------------------------------------------------------------- activations, embedding, bilinear
ACT_KINDS = (0, 1)  # SiLU, exact GELU
ACT_N = ACT_GRID_CAP * 256 + 37
EmbCase = namedtuple("EmbCase", "B dim")
EMB_CASES = (EmbCase(300, 4), EmbCase(300, 6), EmbCase(5, 128))
EMB_T_MAX = 1000.0
BilinearCase = namedtuple("BilinearCase", "name N H W C h w")
BILINEAR_CASES = (
    BilinearCase("past-cap", 1, 300, 301, 3, 837, 836),   # 837 * 836 * 3 = 2 099 196 outputs > 8192 * 256; runs first
    BilinearCase("up-non-integer", 2, 7, 9, 3, 17, 20),
    BilinearCase("down-non-integer", 2, 17, 20, 3, 7, 9),
    BilinearCase("mixed", 1, 11, 5, 2, 6, 13),
)
BILINEAR_BIG_TYPES = ("bf16",)  # the cap case runs in one type; the small ones in all three

# ---------------------------------------------------------------- rejections: (what, expected status)
ERR_ARG, ERR_SHAPE, ERR_DTYPE, ERR_LAUNCH, ERR_WORKSPACE = -1, -2, -3, -4, -5
# GroupNorm: keyword overrides of a valid call (N = 1, HW = 4, C = 16, G = 2, every ld = C, full workspace)
GN_REJECTS = (
    ("C % 8", {"C": 12, "G": 2}, ERR_SHAPE),
    ("C % G", {"C": 16, "G": 3}, ERR_SHAPE),
    ("C / G = 512", {"C": 512, "G": 1}, ERR_SHAPE),
    ("C = 2056", {"C": 2056, "G": 257}, ERR_SHAPE),
    ("ld % 8", {"ld": 20}, ERR_SHAPE),
    ("ld < C", {"ld": 8}, ERR_SHAPE),
    ("short workspace", {"ws_short": 1}, ERR_WORKSPACE),
    ("one modulation pointer null", {"mod_null": 1}, ERR_ARG),
)
OTHER_REJECTS = ("gemm nbatch*ksplit > 65535", "gemm split-K null workspace", "gemm split-K short workspace",
                 "col_softmax B > 65535", "act kind 2", "sinusoidal dim 2", "sinusoidal dim 5", "colsum short workspace",
                 "layernorm bwd short workspace", "col_softmax short workspace")


def ident(c):
    return c if isinstance(c, str) else c.name if hasattr(c, "name") else "-".join(str(v) for v in c)
