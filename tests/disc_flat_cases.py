"""Case tables of the flat-kernel tests of tests/test_gpu_adversarial.py (csrc/cy_disc.hip: softmax + concat,
BatchNorm + LeakyReLU, LeakyReLU, sigmoid + BCE): the sizes that pass FLAT_GRID_CAP and LOSS_GRID_CAP, reach
BN_CHUNKS_MAX, run the scalar LeakyReLU kernel as the whole launch and take Ci = CI_MAX, next to the small sizes the
tests had.  Each case carries a note saying what it reaches; tests/test_disc_flat_coverage.py checks the claims on the
CPU.  Inputs are drawn in the tests from a seeded `torch.Generator`; the references are the f64 formulas there.
"""
from collections import namedtuple

import torch

# ---------------------------------------------------------------------------------------------- the launch rules
FLAT_GRID_CAP = 2048   # csrc/cy_disc.hip: blocks of 256 of the flat sweeps
LOSS_GRID_CAP = 1024   # csrc/cy_reduce.h: blocks of 256 of a loss forward (one f64 partial each)
CI_MAX = 4
BN_C_MAX, BN_CHUNKS_MAX, BN_ROWS_PER_LANE = 1024, 256, 8
FLAT_TRIP, LOSS_TRIP = FLAT_GRID_CAP * 256, LOSS_GRID_CAP * 256


def cy_blocks(items, per_block, cap):
    """csrc/cy_common.h: blocks of `per_block` items for `items`, at least 1, at most `cap`"""
    return max(1, min(cap, -(-items // per_block)))


def trips(items, cap):
    return -(-items // (cy_blocks(items, 256, cap) * 256))


BnGeom = namedtuple("BnGeom", "V ncv lpr rl tiles wanted chunks")


def bn_geom(M, C):
    """bn_geom of csrc/cy_disc.hip, and `wanted`: the chunks before the cap"""
    V = 4 if C % 4 == 0 else 1
    ncv = C // V
    lpr = 1
    while lpr < ncv and lpr < 64:
        lpr *= 2
    rl = 256 // lpr
    tiles = -(-ncv // lpr)
    wanted = -(-M // (rl * BN_ROWS_PER_LANE))
    return BnGeom(V, ncv, lpr, rl, tiles, wanted, max(1, min(BN_CHUNKS_MAX, wanted)))


def bn_combination(M, C):
    """what distinguishes the launches of two shapes: (V, lpr, more than one column tile, chunks capped)"""
    g = bn_geom(M, C)
    return g.V, g.lpr, g.tiles > 1, g.wanted > g.chunks


# ---------------------------------------------------------------------------------------------- softmax + concat
CAT_K, CAT_CI = (2, 4, 5, 16), (0, 1, 3, 4)  # the small parametrisation on 286 pixels; Ci = 4 is CI_MAX
CAT_SMALL_NHW = (2, 13, 11)
CAT_SIDE = 725  # 725 * 725 = 525 625 pixels = one trip of 524 288 + five blocks + 57
# (K, Ci, note) on (1, K, 725, 725)
CAT_PAST_CAP = (
    (4, 0, "KT = 4, Ci = 0: the 16-byte store of the probabilities"),
    (4, 1, "KT = 4, Ci = 1: 16-byte load of the logits, scalar stores behind the image column"),
    (5, 3, "KT = 0: the run-time class count"),
)

# ---------------------------------------------------------------------------------------------- LeakyReLU
LRELU_BIG = 4 * (FLAT_TRIP + 257) + 3  # 2 098 183: the vector kernel past its cap, then a tail of 3
LRELU_MISALIGNED = FLAT_TRIP + 257     # 524 545 on a view one float into its allocation: the scalar kernel alone
# n -> note; every buffer 16-byte aligned
LRELU_ALIGNED = {
    1: "tail only (one element)",
    2: "no vector launch, a tail of 2",
    3: "no vector launch, a tail of 3",
    4: "one vector, no tail launch",
    5: "one vector and a tail of 1: one launch of each",
    1023: "255 vectors (one block, its last thread idle) and a tail of 3",
    1025: "256 vectors (exactly one block) and a tail of 1",
    LRELU_BIG: "the vector kernel past FLAT_GRID_CAP (second trip: block 0 and thread 0 of block 1), a tail of 3",
}


def lrelu_launches(n, aligned=True):
    """(vectors of the 16-byte kernel, elements of the 4-byte kernel) of cy_leaky_relu_fwd / _bwd"""
    nv = n // 4 if aligned else 0
    return nv, n - 4 * nv


def one_float_in(n, device="cpu"):
    """a dense f32 view of n elements that starts one float into its allocation"""
    return torch.zeros(n + 1, dtype=torch.float32, device=device)[1:]


# ---------------------------------------------------------------------------------------------- sigmoid + BCE
# n -> note
BCE_SIZES = {
    1: "one live thread", 6: "a few", 363: "two blocks", 1025: "five blocks",
    LOSS_TRIP + 257: "262 401: the forward past LOSS_GRID_CAP, the backward (FLAT_GRID_CAP) not",
    FLAT_TRIP + 257: "524 545: both past their caps (the forward makes three trips)",
}

# ---------------------------------------------------------------------------------------------- BatchNorm + LeakyReLU
# (M, C) -> (note, the earlier shape whose (V, lpr, tiles > 1, capped) it repeats, or None)
BN_SHAPES = {
    (48, 512): ("V = 4, two full column tiles", None),
    (770, 128): ("V = 4, lpr = 32, 13 row chunks", None),
    (257, 20): ("V = 4, ncv = 5 of lpr = 8: idle column lanes", None),
    (2, 4): ("V = 4, one lane per row; M = 2, the fewest rows batch statistics take", None),
    (259, 7): ("V = 1, ncv = 7 of lpr = 8", None),
    (45, 1023): ("V = 1, sixteen column tiles, the last with one idle lane", None),
    (8225, 1024): ("V = 4, C = BN_C_MAX: four column tiles; 258 chunks wanted, 256 given: a ninth trip over the rows",
                   None),
    (131585, 3): ("V = 1, lpr = 4; 258 chunks wanted, 256 given", None),
    (70, 260): ("V = 4, ncv = 65: the second tile has one live lane of 64 (a partial tile, which (48, 512) has not)",
                (48, 512)),
}
BN_NEW = ((8225, 1024), (131585, 3), (70, 260))

# two runs give the same bits
SAME_BITS_BN = (8225, 1024)
SAME_BITS_BCE = (LOSS_TRIP + 257, FLAT_TRIP + 257)
