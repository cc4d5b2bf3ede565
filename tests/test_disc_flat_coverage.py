"""The flat-kernel tests of tests/test_gpu_adversarial.py claim to pass FLAT_GRID_CAP and LOSS_GRID_CAP, to reach
BN_CHUNKS_MAX, to run the scalar LeakyReLU kernel as the whole launch on a misaligned base and to take Ci = CI_MAX
(csrc/cy_disc.hip).  The claims are conditions on the case tables (tests/disc_flat_cases.py), on the constants parsed
out of the source and on the restated launch rules alone, so they are checked here without a GPU.  Each assertion names
its condition: deleting a case fails here, by name."""
import re
from pathlib import Path

import disc_flat_cases as dc

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "contrast-you_amd" / "csrc"
SOURCE = CSRC / "cy_disc.hip"


def test_constants_and_launches_match_the_source():
    text = SOURCE.read_text()
    consts = dict(re.findall(r"constexpr int (\w+) = (\d+);", text))
    names = ("FLAT_GRID_CAP", "CI_MAX", "BN_CHUNKS_MAX", "BN_ROWS_PER_LANE", "BN_C_MAX")
    assert {k: int(consts[k]) for k in names} == {
        "FLAT_GRID_CAP": dc.FLAT_GRID_CAP, "CI_MAX": dc.CI_MAX, "BN_CHUNKS_MAX": dc.BN_CHUNKS_MAX,
        "BN_ROWS_PER_LANE": dc.BN_ROWS_PER_LANE, "BN_C_MAX": dc.BN_C_MAX}
    assert re.findall(r"constexpr int LOSS_GRID_CAP = (\d+);", (CSRC / "cy_reduce.h").read_text()) == [
        str(dc.LOSS_GRID_CAP)]
    assert (dc.FLAT_TRIP, dc.LOSS_TRIP) == (524288, 262144)
    # every flat launch is cy_blocks(items, 256, cap): the loss forward (and its workspace) under LOSS_GRID_CAP, every
    # other sweep under FLAT_GRID_CAP
    calls = re.findall(r"\bcy_blocks\(([^,]+), (\w+), (\w+)\)", text)
    assert {c[1] for c in calls} == {"256"}, calls
    assert sorted(c[0] for c in calls if c[2] == "LOSS_GRID_CAP") == ["n", "n"]
    flat = sorted(c[0] for c in calls if c[2] == "FLAT_GRID_CAP")
    assert flat == sorted(["npix"] * 4 + ["nv"] * 2 + ["n - 4 * nv"] * 2 + ["n"]) and len(calls) == len(flat) + 2, calls
    assert re.search(r"sigmoid_bce_bwd_kernel, dim3\(cy_blocks\(n, 256, FLAT_GRID_CAP\)\)", text), \
        "the BCE backward is a flat sweep: it passes its cap at another size than the forward"
    # softmax + concat forward and backward, LeakyReLU, BCE forward and backward
    assert text.count("+= (long)gridDim.x * 256L") == 5 == text.count("= blockIdx.x * 256L + threadIdx.x;")
    # the four BatchNorm row kernels step over the row chunks
    assert text.count("r += (long)gridDim.y * nrl") == 4 == text.count("long r = (long)blockIdx.y * nrl + rl;")
    assert "dim3((G).tiles, (G).chunks)" in text
    assert "atomicAdd" not in text and "__hip_atomic" not in text


def test_the_restated_launch_rules_are_the_library_s():
    assert [dc.cy_blocks(n, 256, 8192) for n in (0, 1, 256, 257, 8192 * 256 + 1)] == [1, 1, 1, 2, 8192]
    from cyhip import _lib
    lib = _lib.load()
    for n in dc.BCE_SIZES:
        assert lib.cy_sigmoid_bce_ws_bytes(n) == 8 * dc.cy_blocks(n, 256, dc.LOSS_GRID_CAP), n
    # chunks * 2 * C doubles of partial sums
    for M, C in list(dc.BN_SHAPES) + [(3000, 128), (1, 1), (10 ** 6, 1024), (10 ** 6, 1), (513, 8), (100, 64)]:
        assert lib.cy_bn_rows_ws_bytes(M, C) == dc.bn_geom(M, C).chunks * 2 * C * 8, (M, C)
    g = dc.bn_geom(100, 256)
    assert (g.V, g.ncv, g.lpr, g.rl, g.tiles) == (4, 64, 64, 4, 1)
    assert all(dc.bn_geom(7, C).lpr in (1, 2, 4, 8, 16, 32, 64) for C in range(1, dc.BN_C_MAX + 1))


# ---------------------------------------------------------------------------------------------- softmax + concat
def test_softmax_cat_cases():
    assert set(dc.CAT_CI) == {0, 1, 3, dc.CI_MAX} and set(dc.CAT_K) == {2, 4, 5, 16}
    N, H, W = dc.CAT_SMALL_NHW
    assert N * H * W == 286
    npix = dc.CAT_SIDE ** 2
    assert npix == 525625 == dc.FLAT_TRIP + 5 * 256 + 57 and dc.trips(npix, dc.FLAT_GRID_CAP) == 2
    forms = {(K, Ci) for K, Ci, _ in dc.CAT_PAST_CAP}
    assert (4, 0) in forms, "KT = 4 without an image: the 16-byte store"
    assert (4, 1) in forms, "KT = 4 behind an image column: 16-byte load, scalar stores"
    assert (5, 3) in forms, "the run-time class count"
    assert len(forms) == 3 and all(Ci <= dc.CI_MAX for _, Ci in forms)


# ---------------------------------------------------------------------------------------------- LeakyReLU
def test_leaky_relu_cases():
    n = dc.LRELU_BIG
    assert n == 2098183 == 4 * (dc.FLAT_TRIP + 257) + 3 and n in dc.LRELU_ALIGNED
    nv, tail = dc.lrelu_launches(n)
    assert tail == 3 and dc.trips(nv, dc.FLAT_GRID_CAP) == 2 and nv - dc.FLAT_TRIP == 257, \
        "the vector kernel past its cap (second trip: block 0 and thread 0 of block 1), then a tail of 3"
    launches = {n: dc.lrelu_launches(n) for n in (2, 3, 4, 5)}
    assert set(launches) <= set(dc.LRELU_ALIGNED)
    assert launches == {2: (0, 2), 3: (0, 3), 4: (1, 0), 5: (1, 1)}, "no vector launch, no tail launch, one of each"
    assert {1, 1023, 1025} <= set(dc.LRELU_ALIGNED), "the sizes the test had"
    assert all(dc.lrelu_launches(n)[1] <= 3 for n in dc.LRELU_ALIGNED), "aligned: the scalar kernel is a tail only"


def test_leaky_relu_misaligned_case():
    n = dc.LRELU_MISALIGNED
    assert n == 524545 == dc.FLAT_TRIP + 257
    assert dc.lrelu_launches(n, aligned=False) == (0, n) and dc.trips(n, dc.FLAT_GRID_CAP) == 2, \
        "the scalar kernel alone, and past its cap"
    x = dc.one_float_in(n)
    assert x.data_ptr() % 16 == 4 and x.numel() == n and x.is_contiguous()
    # what the GPU test builds from it, and what LeakyReLUFn makes of that: the same memory, no aligned copy
    from cyhip.functions import _rows
    leaf = x.reshape(1, 1, n, 1).requires_grad_(True)
    assert leaf.is_leaf and leaf.data_ptr() == x.data_ptr()
    assert _rows(leaf).data_ptr() == x.data_ptr() and _rows(leaf).shape == (1, n, 1, 1)


# ---------------------------------------------------------------------------------------------- sigmoid + BCE
def test_sigmoid_bce_cases():
    a, b = dc.LOSS_TRIP + 257, dc.FLAT_TRIP + 257
    assert (a, b) == (262401, 524545) and {a, b, 1, 6, 363, 1025} == set(dc.BCE_SIZES)
    assert dc.trips(a, dc.LOSS_GRID_CAP) == 2 and dc.trips(a, dc.FLAT_GRID_CAP) == 1, \
        "the forward is past LOSS_GRID_CAP, the backward is not past its cap"
    assert dc.trips(b, dc.LOSS_GRID_CAP) == 3 and dc.trips(b, dc.FLAT_GRID_CAP) == 2, "both are past their caps"
    assert all(dc.trips(n, dc.LOSS_GRID_CAP) == 1 for n in (1, 6, 363, 1025))
    assert set(dc.SAME_BITS_BCE) == {a, b}


# ---------------------------------------------------------------------------------------------- BatchNorm + LeakyReLU
def test_bn_capped_cases():
    g = dc.bn_geom(8225, 1024)
    assert (g.V, g.lpr, g.tiles, g.wanted, g.chunks) == (4, 64, 4, 258, dc.BN_CHUNKS_MAX), "V = 4, 4 column tiles"
    g = dc.bn_geom(131585, 3)
    assert (g.V, g.lpr, g.tiles, g.wanted, g.chunks) == (1, 4, 1, 258, dc.BN_CHUNKS_MAX), "V = 1, lpr = 4"
    for M, C in ((8225, 1024), (131585, 3)):
        g = dc.bn_geom(M, C)
        assert (M, C) in dc.BN_SHAPES and g.chunks == dc.BN_CHUNKS_MAX < g.wanted, "more chunks wanted than given"
        # a lane's ninth trip over the rows (one more than BN_ROWS_PER_LANE), which only some row lanes make
        assert 0 < M - g.chunks * g.rl * dc.BN_ROWS_PER_LANE < g.chunks * g.rl
    assert dc.SAME_BITS_BN == (8225, 1024) and 8225 * 1024 * 4 < 2 ** 26, "the largest tensor of the suite's new cases"
    assert max(C for _, C in dc.BN_SHAPES) == dc.BN_C_MAX


def test_bn_partial_tile_case():
    g = dc.bn_geom(70, 260)
    assert (70, 260) in dc.BN_SHAPES and (g.V, g.ncv, g.lpr, g.tiles) == (4, 65, 64, 2)
    assert g.ncv - (g.tiles - 1) * g.lpr == 1, "the second tile has one live lane of 64"
    assert g.wanted == g.chunks == 3


def test_bn_shapes_are_distinct_launches_or_say_what_they_repeat():
    assert set(dc.BN_NEW) <= set(dc.BN_SHAPES) and len(dc.BN_SHAPES) == 6 + len(dc.BN_NEW)
    assert list(dc.BN_SHAPES)[:6] == [(48, 512), (770, 128), (257, 20), (2, 4), (259, 7), (45, 1023)], \
        "the shapes the test had"
    seen = {}
    for shape, (note, repeats) in dc.BN_SHAPES.items():
        combo = dc.bn_combination(*shape)
        if combo in seen:
            assert repeats == seen[combo], f"{shape} repeats {seen[combo]} and must say so"
            assert "partial tile" in note, "and say what it adds"
        else:
            assert repeats is None, shape
            seen[combo] = shape
    assert {c[0] for c in seen} == {1, 4} and {c[3] for c in seen} == {False, True}
    assert {(c[0], c[3]) for c in seen} == {(1, False), (1, True), (4, False), (4, True)}, "each V capped and not"
    assert all(M >= 2 for M, _ in dc.BN_SHAPES), "batch statistics need two rows"
