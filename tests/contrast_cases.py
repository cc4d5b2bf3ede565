"""The cases tests/test_gpu_contrast_dispatch.py is parametrised with, and what tests/test_contrast_plan_coverage.py
requires of them: the kernels of csrc/cy_contrast.hip -- the f32 MFMA GEMM, the InfoNCE / SupCon loss on its three paths
(materialised similarity matrix, fused, exclude_other_pos) -- and of csrc/cy_proj_head.hip -- the projection head,
piecewise and in one launch.
A plain module: no GPU, no torch and no library call at import.

Every shape is the smallest that reaches its branch.  The column-split count of the fused kernels is never restated
here: the coverage file reads it from cy_supcon_fused_ws_bytes.  What the library does not export (tile sizes, the block
cap, the pooling slices of the one-launch head) is restated below FOR COVERAGE ONLY, next to a pointer at its source
line; no expected value of the GPU file comes from it.

Tolerances are the ones the project already applies to these kernels (tests/test_gpu_kernels.py,
tests/test_gpu_round4_rows.py), on max|got - ref| <= tol * max|ref| over the whole tensor, no element left out."""
from collections import namedtuple

TYPES = ("f32", "bf16", "f16")
T = 0.07        # temperature of every SupCon case
GSCALE = 0.7    # upstream gradient of every backward: never 1

TOL_LOSS = 1e-5           # relative
TOL_GRAD = 1e-4           # f32 gradients and matrices against float64
TOL_Z, TOL_SIM = 2e-5, 1e-5   # forward outputs of the head (pooled, y1, y2, norms, z); sim_logits / sim_exp
TOL_PATHS = 1e-5          # fused against materialised
TOL_SGEMM = 1e-6
TOL_POOL = 1e-6           # avgpool forward: at most 7 additions and one division in f32
TOL_16 = {"f32": TOL_GRAD, "bf16": 1.2e-2, "f16": 2e-3}   # dfeat / dx in the storage type

# ---------------------------------------------------------------- restated launch geometry (coverage only)
SC_TM = 64          # cy_contrast.hip: constexpr int SC_TM, rows / columns of a fused tile
SC_SPLIT_BUDGET = 256   # cy_contrast.hip: sc_nsplit(), `ns = 256 / rb`, at most rb, at least 1
GRID_CAP = 8192     # cy_contrast.hip and cy_proj_head.hip: `constexpr int GRID_CAP = 8192;`, cy_blocks(items, 256, GRID_CAP)
SGEMM_KSTAGE = 16   # cy_contrast.hip: sgemm_kernel stages K 16 at a time
DP_TILE = 32        # cy_contrast.hip: sc_bwd_sweep, `nct = (D + 31) / 32` column tiles of dP, 8 at most
PH_NT, PH_NW = 1024, 16   # cy_proj_head.hip: threads and waves of the one-launch head
EPC = {"f32": 4, "bf16": 8, "f16": 8}   # cy_common.h: ElemTr<T>::EPC, elements per 16-byte chunk


def row_blocks(R):
    return -(-R // SC_TM)


def split_blocks(R, ns):
    """cy_contrast.hip, sc_block(): split y takes column blocks [ncb * y / ns, ncb * (y + 1) / ns)"""
    ncb = row_blocks(R)
    return [ncb * (y + 1) // ns - ncb * y // ns for y in range(ns)]


def pool_slices(C, dtype):
    """cy_proj_head.hip, proj_head_fwd_kernel: `nsl = PH_NT / G < PH_NW ? PH_NT / G : PH_NW`, G = C / EPC"""
    return min(PH_NT // (C // EPC[dtype]), PH_NW)


# ---------------------------------------------------------------- SupCon: the golden masks
PATHS = ("materialised", "fused", "exclude_other_pos")
GOLDEN_FILE = "supcon_masks.npz"    # tests/golden/gen_goldens_supcon.py
GOLDEN_N, GOLDEN_D = 70, 16
# name -> (holds pairs that are neither, symmetric)
GOLDEN_MASKS = {"a": (False, True), "b": (False, False), "c": (True, True), "d": (True, False), "z": (False, False)}

# ---------------------------------------------------------------- SupCon: column splits of the fused kernels
# positives: "simclr" = labels 0..n-1 (only the other view), "mod3" = labels i % 3; `paths`: which of PATHS run
SplitCase = namedtuple("SplitCase", "name n D positives paths row_blocks splits twins")
SPLIT_CASES = (
    SplitCase("one-pair", 1, 16, "simclr", PATHS, 1, 1, True),                   # R = 2: the smallest problem there is
    SplitCase("one-full-tile", 32, 8, "mod3", PATHS, 1, 1, False),               # R = 64
    SplitCase("two-row-second-tile", 33, 8, "mod3", PATHS, 2, 2, False),         # R = 66
    SplitCase("splits-of-one-and-two-blocks", 520, 8, "mod3", PATHS, 17, 15, False),   # R = 1040
    SplitCase("129-row-blocks", 4100, 8, "mod3", ("fused",), 129, 1, False),     # R = 8200: 256 / 129 = 1
    SplitCase("past-the-split-budget", 8200, 8, "mod3", ("fused",), 257, 1, False),    # R = 16400: 256 / 257 = 0 -> 1
)
# One pair: each row's only other column is its positive, so loss_i = log(1 + 1e-16 / e_ij) and every gradient term
# carries the same 1e-16 -- zero to f32 whatever the input, a relative bound has nothing to hold on to.  The case
# therefore makes the arithmetic exact: both views are the same row of entries +-1/4, D = 16 (`twin_rows`), so every
# product and partial sum is exact in any order, S_ij = S_ii = M and e_ij = 1.  The float64 reference gives exactly 0
# for loss and gradient (it rounds 1 + 1e-16 to 1; the true values are 1e-16 and at most gs / (R t) * 1e-16 * 2 |P| =
# 2.5e-16).  Bound, absolute: 1e-15, the reference's own error.  A wrong positive count, a diagonal or a column past
# R in the denominator (each adds at least exp(-1 / t) = 6e-7) is far outside it.
ONE_PAIR_ABS = 1e-15


def twin_rows(n, D):
    """n rows of D entries +-1/4 (unit norm for D = 16), signs from a fixed pattern"""
    return [[0.25 if (3 * i + k * k) % 5 < 3 else -0.25 for k in range(D)] for i in range(n)]


# R = 4096 (64 row blocks, 4 splits) runs in tests/test_gpu_kernels.py already; the coverage file checks the citation
SPLIT_CITED = {"R": 4096, "row_blocks": 64, "splits": 4, "file": "test_gpu_kernels.py",
               "test": "test_supcon_fused_against_oracle_and_unfused", "param": "(2048, 256)"}
CHUNK_ROWS = 512      # the float64 reference of the fused-only cases is formed in row chunks of at most this many rows
CHUNKED_FROM = 8200   # ... from this R on: the similarity matrix is never formed whole

# ---------------------------------------------------------------- SupCon: embedding widths
WIDTH_N = 35   # R = 70: two row blocks, two column splits, a six-row second tile
# fused: 1, 2, 3, 5, 8 (ragged: 248 = 7 * 32 + 24) and 8 (full) column tiles of the second product
FUSED_WIDTHS = (8, 40, 96, 136, 248, 256)
# materialised: K below, across and past the 16-wide stage of the GEMM; 257 and 264 are the widths the fused path
# refuses (above 256; 257 is no multiple of 8 either), 1 and 17 are no multiples of 8
MATERIALISED_WIDTHS = (1, 17, 257, 264)

# ---------------------------------------------------------------- SupCon: past the block cap GRID_CAP
CAP_N, CAP_D = 725, 8   # R = 1450: R * R = 2 102 500 > 8192 * 256, through cy_supcon_bwd, _excl_bwd and _matrices
MASK_D_VALUES = (0, 1, -1, 2)   # a mask "of kind (d)": asymmetric, these values, all-ones diagonal


def kind_d_mask(n, seed):
    """an [n][n] int8 mask of kind (d) -- asymmetric, values {0, 1, -1, 2}, all-ones diagonal -- as a torch tensor"""
    import torch
    g = torch.Generator().manual_seed(seed)
    eye = torch.eye(n, dtype=torch.bool)
    m = ((torch.rand(n, n, generator=g) < 0.2) | eye).to(torch.int8)
    m[(torch.rand(n, n, generator=g) < 0.12) & ~eye] = -1
    m[(torch.rand(n, n, generator=g) < 0.10) & ~eye] = 2
    return m


# ---------------------------------------------------------------- cy_sgemm
SGEMM_SIZES = ((1, 1, 1), (64, 64, 16), (65, 63, 17), (130, 5, 2), (3, 200, 45))   # (M, N, K)
SGEMM_ALPHA = 0.75

# ---------------------------------------------------------------- projector pieces
POOL_HW = (1, 3, 4, 7)       # the four-way unroll of avgpool_fwd_kernel: tail only, tail only, one round, round + tail
POOL_C = (8, 256, 264)       # 264: a second channel block of 256 threads, 8 of them busy
POOL_N = 2
POOL_CAP = (2, 4097, 256)    # (N, HW, C) of the backward: 2 097 664 elements, just above 8192 * 256 = 2 097 152

LINEAR_I = (1, 63, 64, 65)   # below, at and past one trip of the 64 lanes
LINEAR_O = (1, 3, 4, 5)      # the four-chain loop of linear_bwd_dx_kernel: tail only, one round, round + tail
LINEAR_M = 5
LINEAR_ACTS = (0, 1)         # none, LeakyReLU
LINEAR_SLOPE = 0.01
# (dx, dw, db) requested: every combination (none at all launches nothing and must leave the buffers alone)
LINEAR_WANTS = tuple((a, b, c) for a in (1, 0) for b in (1, 0) for c in (1, 0))
LINEAR_WANTS_AT = (65, 5)    # (I, O) the combinations run at

L2_D = (1, 63, 64, 65, 300)
L2_M = (1, 4, 5)             # one wave per row, four rows per block: one block part full, full, and a second block
L2_ZERO_ROW = 0              # this row of every case with M > 1 is exactly zero: nrm <= eps, dx = dz / eps
L2_EPS = 1e-12

# ---------------------------------------------------------------- the one-launch projection head
HEAD_SHAPES = ((8, 4, 1), (512, 512, 512), (264, 260, 3), (128, 256, 256))   # (C, hid, out)
HEAD_HW = (1, 5, 16, 17, 196)   # fewer positions than pooling slices, equal (16 slices), one more, the hook's 14 x 14
HEAD_B = (1, 3)
# (8, 4, 1): with one output the normalised vector is +-1 and its gradient dz / nrm - y2 (y2 . dz) / nrm^3 cancels to
# zero exactly; so does every gradient behind it, and the float64 reference holds rounding residue of 1e-15 and less.
# A bound relative to that has nothing to hold on to.  By the project's rule for such cases: the same case in float32
# on the CPU with the kernels' operations -- 1 / nrm, then dz * iv - y2 * (dot * iv * iv * iv) -- in torch's summation
# order (test_gpu_contrast_dispatch.yardstick_head_out1: largest error against float64 over the case's HW x B x
# storage types), and twice that, absolute, added to the relative bound.  (torch's own F.normalize backward rounds
# fewer times: 4.9e-9 on dfeat where this formula leaves 1.3e-8 -- the residue is the formula's, on any device.)
HEAD_OUT1_YARDSTICK = {"dfeat": 1.3e-08, "dw1": 8.9e-08, "db1": 3.8e-07, "dw2": 3.4e-07, "db2": 9.5e-07}
HEAD_OUT1_BOUND = {k: 2 * v for k, v in HEAD_OUT1_YARDSTICK.items()}
HEAD_SLOPE, HEAD_EPS = 0.01, 1e-12
HEAD_ZERO = {"shape": (128, 256, 256), "HW": 5, "B": 3, "sample": 1}   # that sample all zero, both biases zero
# ProjectionHead.forward: (name, C, hid, out, one launch?)
MODULE_CASES = (("one-launch", 128, 256, 256, True), ("wide-input", 520, 256, 256, False), ("odd-hidden", 128, 6, 256, False))

# ---------------------------------------------------------------- rejections (CPU file)
ERR_ARG, ERR_SHAPE, ERR_DTYPE, ERR_LAUNCH, ERR_WORKSPACE = -1, -2, -3, -4, -5
SUPCON_ENTRIES = ("cy_supcon_fwd", "cy_supcon_bwd", "cy_supcon_excl_fwd", "cy_supcon_excl_bwd", "cy_supcon_fused_fwd",
                  "cy_supcon_fused_bwd")
# (what, overrides of n / D / t / nulls, expected status, the entries it applies to)
SUPCON_REJECTS = (
    ("P null", {"null": "P"}, ERR_ARG, SUPCON_ENTRIES),
    ("neither labels nor mask", {"null": "labels+mask"}, ERR_ARG, SUPCON_ENTRIES),
    ("an output null", {"null": "out"}, ERR_ARG, SUPCON_ENTRIES),
    ("n = 0", {"n": 0}, ERR_SHAPE, SUPCON_ENTRIES),
    ("n < 0", {"n": -3}, ERR_SHAPE, SUPCON_ENTRIES),
    ("D = 0", {"D": 0}, ERR_SHAPE, SUPCON_ENTRIES),
    ("D < 0", {"D": -8}, ERR_SHAPE, SUPCON_ENTRIES),
    ("t = 0", {"t": 0.0}, ERR_SHAPE, SUPCON_ENTRIES),
    ("t < 0", {"t": -0.07}, ERR_SHAPE, SUPCON_ENTRIES),
    ("fused D = 257", {"D": 257}, ERR_SHAPE, SUPCON_ENTRIES[4:]),
    ("fused D = 12", {"D": 12}, ERR_SHAPE, SUPCON_ENTRIES[4:]),
    ("fused workspace one byte short", {"ws_short": 1}, ERR_WORKSPACE, SUPCON_ENTRIES[4:]),
    ("fused workspace null", {"null": "ws"}, ERR_ARG, SUPCON_ENTRIES[4:]),
)
HEAD_REJECTS = (
    ("C = 520", {"C": 520}, ERR_SHAPE),
    ("C = 12", {"C": 12}, ERR_SHAPE),
    ("hid = 6", {"hid": 6}, ERR_SHAPE),
    ("hid = 516", {"hid": 516}, ERR_SHAPE),
    ("out = 513", {"out": 513}, ERR_SHAPE),
    ("unknown dtype code", {"dtype": 7}, ERR_DTYPE),
    ("short workspace", {"ws_short": 1}, ERR_WORKSPACE),
    ("feat / dz null", {"null": 1}, ERR_ARG),
)
