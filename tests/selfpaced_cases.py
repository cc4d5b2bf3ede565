"""The cases of tests/test_gpu_selfpaced.py and tests/test_selfpaced_host.py: SelfPacedSupConLoss on the fused kernels
of csrc/cy_contrast.hip (supcon_sp_fwd_kernel, supcon_sp_finalize_kernel, supcon_sp_bwd_kernel).  Tables at import: no
GPU, no torch and no library call; the functions below import torch when they are called.

The geometry (tile size, column splits, widths of the second product) is that of tests/contrast_cases.py, whose
constants are used as they are.  The hard weight [l_ij <= gamma] is a threshold: every hard case must leave a gap of
HARD_MARGIN between gamma and the float64 loss of every positive pair, so that float32 cannot come down on the other
side.  That is a condition on the inputs (tests/test_selfpaced_host.py asserts it for every problem below), not a
measurement.  gamma is never restated here: it is derived from the problem's own float64 losses by its rule."""
from collections import namedtuple

from tests.contrast_cases import (GSCALE, ONE_PAIR_ABS, T, TOL_GRAD, TOL_LOSS, TOL_PATHS, WIDTH_N, kind_d_mask,  # noqa: F401
                                  row_blocks, split_blocks, twin_rows)

MODES = ("hard", "soft")
HARD_MARGIN = 1e-3     # min |l_ij - gamma| over every positive pair, float64
RATIO_FLOOR = 1e-6     # the ratio's tolerance is 4 x the reference's own f32-f64 distance, at least this

# ---------------------------------------------------------------- problems
# positives: "simclr" labels 0..n-1, "mod3" labels i % 3, "maskd" kind_d_mask(n, MASK_SEED)
# rows: "twin" twin_rows (both views the same +-1/4 row), "camp" two camps of opposite sign, "rand" random unit rows
# gamma rule (hard, soft): camp -> the midpoint of the largest gap of the sorted positive-pair losses, both modes;
#                          rand -> hard: midpoint of the widest gap between the 25th and 75th percentile, soft: the median
Problem = namedtuple("Problem", "name n D positives rows seed")
MASK_SEED = 61
CAMP_SEED, RAND_SEED = 11, 23

ONE_PAIR = Problem("one-pair", 1, 16, "simclr", "twin", 0)
# (name, n, D, row blocks, column splits)
SIZES = (("one-full-tile", 32, 8, 1, 1), ("two-row-second-tile", 33, 8, 2, 2), ("uneven-splits", 520, 8, 17, 15))
RAND_MAX_N = 70   # random rows leave a margin of a few 1e-3 only at small sizes
SIZE_PROBLEMS = tuple(Problem(f"{name}/camp", n, D, "mod3", "camp", CAMP_SEED) for name, n, D, _, _ in SIZES) + \
    tuple(Problem(f"{name}/rand", n, D, "mod3", "rand", RAND_SEED) for name, n, D, _, _ in SIZES if n <= RAND_MAX_N)
# widths at n = 35 (R = 70): 1 tile, 2 tiles, a ragged eighth tile and a full eighth tile of the second product
WIDTHS = (8, 40, 248, 256)
WIDTH_PROBLEMS = tuple(Problem(f"width-{D}", WIDTH_N, D, "mod3", "rand", RAND_SEED) for D in WIDTHS)
# the fused path refuses these (above 256; no multiple of 8): the composition runs and still matches
FALLBACK_WIDTHS = (264, 17)
FALLBACK_PROBLEMS = tuple(Problem(f"fallback-{D}", WIDTH_N, D, "mod3", "rand", RAND_SEED) for D in FALLBACK_WIDTHS)
MASK_PROBLEM = Problem("mask-d", WIDTH_N, 16, "maskd", "rand", RAND_SEED)
BIG = Problem("uneven-splits/camp", 520, 8, "mod3", "camp", CAMP_SEED)   # R = 1040: the two bit-equal runs
# fused against the kept composition, TOL_PATHS on loss and gradients: the general mask, and labels over two and over
# fifteen column splits (every one of them is in ALL_PROBLEMS, so its hard margin is asserted)
PATH_PROBLEMS = (MASK_PROBLEM, Problem("two-row-second-tile/camp", 33, 8, "mod3", "camp", CAMP_SEED),
                 Problem("two-row-second-tile/rand", 33, 8, "mod3", "rand", RAND_SEED), BIG)
ALL_PROBLEMS = (ONE_PAIR,) + SIZE_PROBLEMS + WIDTH_PROBLEMS + FALLBACK_PROBLEMS + (MASK_PROBLEM,)

# ---------------------------------------------------------------- golden (tests/golden/gen_goldens_selfpaced.py)
GOLDEN_FILE = "selfpaced.npz"
GOLDEN_INPUTS = "supcon_masks.npz"    # z1, z2 (70 x 16 random unit rows), b_mask, d_mask
GOLDEN_N, GOLDEN_D = 70, 16
GOLDEN_POSITIVES = ("mod3", "b", "d")   # labels i % 3; the asymmetric masks, d with pairs that are neither
GOLDEN_TAGS = tuple(f"{p}_{m}_c{c}" for p in GOLDEN_POSITIVES for m in MODES for c in (0, 1))
# |ratio(f32) - ratio(f64)| of the REFERENCE on each golden case, as the generator printed it; the test allows
# max(4 x this, RATIO_FLOOR).  The hard ratio is a count over a count: the same in both precisions.
RATIO_F32_F64 = {
    "mod3_hard_c0": 0.0e+00,   # gamma 7.565548  loss 1.419299  ratio 0.274859
    "mod3_hard_c1": 0.0e+00,   # gamma 7.565548  loss 5.163730  ratio 0.274859
    "mod3_soft_c0": 1.3e-08,   # gamma 9.936621  loss 0.800364  ratio 0.157497
    "mod3_soft_c1": 1.3e-08,   # gamma 9.936621  loss 5.081758  ratio 0.157497
    "b_hard_c0": 0.0e+00,   # gamma 10.264114  loss 3.594654  ratio 0.522295
    "b_hard_c1": 0.0e+00,   # gamma 10.264114  loss 6.882427  ratio 0.522295
    "b_soft_c0": 7.1e-09,   # gamma 10.044763  loss 0.791010  ratio 0.160387
    "b_soft_c1": 7.1e-09,   # gamma 10.044763  loss 4.931886  ratio 0.160387
    "d_hard_c0": 0.0e+00,   # gamma 12.159835  loss 5.647486  ratio 0.722429
    "d_hard_c1": 0.0e+00,   # gamma 12.159835  loss 7.817361  ratio 0.722429
    "d_soft_c0": 2.5e-09,   # gamma 9.800202  loss 0.777663  ratio 0.168340
    "d_soft_c1": 2.5e-09,   # gamma 9.800202  loss 4.619605  ratio 0.168340
}


def ratio_tol(tag):
    return max(4 * RATIO_F32_F64[tag], RATIO_FLOOR)

# ---------------------------------------------------------------- behaviour
GAMMA_INF = 1e10           # every weight 1: the loss is SupConLoss1's
NOMAT_N, NOMAT_D = 2048, 256   # R = 4096: one R x R f32 matrix is 64 MiB, the fused step must stay below that
HOOK = {"channels": 128, "hw": 32, "n": 4, "K": 4}   # test_self_paced_infonce_hook_gamma_schedule_and_loss's setup

ERR_ARG, ERR_SHAPE, ERR_WORKSPACE = -1, -2, -5
SP_ENTRIES = ("cy_supcon_sp_fwd", "cy_supcon_sp_bwd")
# (what, overrides, expected status)
SP_REJECTS = (
    ("P null", {"null": "P"}, ERR_ARG),
    ("neither labels nor mask", {"null": "labels+mask"}, ERR_ARG),
    ("an output null", {"null": "out"}, ERR_ARG),
    ("row_stats null", {"null": "stats"}, ERR_ARG),
    ("workspace null", {"null": "ws"}, ERR_ARG),
    ("n = 0", {"n": 0}, ERR_SHAPE),
    ("n < 0", {"n": -3}, ERR_SHAPE),
    ("D = 0", {"D": 0}, ERR_SHAPE),
    ("D < 0", {"D": -8}, ERR_SHAPE),
    ("D = 264", {"D": 264}, ERR_SHAPE),
    ("D = 12", {"D": 12}, ERR_SHAPE),
    ("t = 0", {"t": 0.0}, ERR_SHAPE),
    ("t < 0", {"t": -0.07}, ERR_SHAPE),
    ("t NaN", {"t": float("nan")}, ERR_SHAPE),
    ("gamma = 0", {"gamma": 0.0}, ERR_SHAPE),
    ("gamma < 0", {"gamma": -1.0}, ERR_SHAPE),
    ("gamma NaN", {"gamma": float("nan")}, ERR_SHAPE),
    ("workspace one byte short", {"ws_short": 1}, ERR_WORKSPACE),
)


# ---------------------------------------------------------------- inputs (torch from here on)
def camp_rows(n, D, seed):
    """two views of n unit rows in two camps of opposite sign around three class centres: a positive pair lies either
    in one camp (cosine near 1) or across them (near -1), which leaves a gap of some 25 between the two groups of
    losses at t = 0.07.  Drawn in float64 in the order centres, z1 noise, z2 noise; returned as float32"""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    c = F.normalize(torch.randn(3, D, generator=g, dtype=torch.float64), dim=1)
    noise = [torch.randn(n, D, generator=g, dtype=torch.float64) for _ in range(2)]
    idx = torch.arange(n)
    sign = torch.where((idx // 3) % 2 == 0, 1.0, -1.0).to(torch.float64)[:, None]
    return tuple(F.normalize(sign * c[idx % 3] + 0.05 * e, dim=1).float() for e in noise)


def rand_rows(n, D, seed):
    """two views of n random unit rows, float64 draws, returned as float32"""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    z1 = F.normalize(torch.randn(n, D, generator=g, dtype=torch.float64), dim=1)
    z2 = F.normalize(z1 + 0.4 * torch.randn(n, D, generator=g, dtype=torch.float64), dim=1)
    return z1.float(), z2.float()


def tensors(p):
    """(z1, z2, target list or None, mask or None) of a problem, on the CPU"""
    import torch
    if p.rows == "twin":
        z1 = torch.tensor(twin_rows(p.n, p.D), dtype=torch.float32)
        z1, z2 = z1, z1.clone()
    else:
        z1, z2 = (camp_rows if p.rows == "camp" else rand_rows)(p.n, p.D, p.seed)
    if p.positives == "maskd":
        return z1, z2, None, kind_d_mask(p.n, MASK_SEED)
    return z1, z2, (list(range(p.n)) if p.positives == "simclr" else [i % 3 for i in range(p.n)]), None


def positive_losses(z1, z2, target=None, mask=None, t=T):
    """l_ij = log D_i - (s_ij - M) of every positive pair in float64, sorted (contrastive.py:160-177)"""
    import torch
    n = z1.shape[0]
    if mask is not None:
        pos, neg = (mask == 1), (mask == 0)
    else:
        lab = torch.as_tensor(list(target))
        pos = lab[:, None] == lab[None, :]
        neg = ~pos
    off = ~torch.eye(2 * n, dtype=torch.bool)
    pos, neg = pos.repeat(2, 2) & off, neg.repeat(2, 2) & off
    P = torch.cat([z1, z2], 0).double()
    logits = P @ P.t() / t
    logits = logits - logits.max()
    denom = (logits.exp() * (pos | neg)).sum(1, keepdim=True) + 1e-16
    return torch.sort((denom.log() - logits)[pos]).values


def gamma_of(p, mode, l=None):
    """gamma by the problem's rule, from its own float64 positive-pair losses"""
    import torch
    if l is None:
        z1, z2, target, mask = tensors(p)
        l = positive_losses(z1, z2, target, mask)
    if p.rows == "twin":
        return 1.0   # every l_ij is 0
    if p.rows == "rand" and mode == "soft":
        return float(l[l.numel() // 2])
    if p.rows == "rand":
        l = l[l.numel() // 4: l.numel() - l.numel() // 4]
    gaps = l[1:] - l[:-1]
    k = int(torch.argmax(gaps))
    return float((l[k] + l[k + 1]) / 2)
