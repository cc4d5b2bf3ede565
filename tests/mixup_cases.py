"""The cases of the MixUp / ICT kernels (csrc/cy_mixup.hip), shared by tests/golden/gen_goldens_mixup.py, the CPU tests
(tests/test_mixup_host.py) and the GPU tests (tests/test_gpu_mixup.py): the smallest shapes at which each thing can go
wrong.

Loss cases (both losses run on every one):
    K        2, 4, 8 compiled; 3, 5, 16 run-time
    N/index  2 with the swap; 4 with a fixed point; 6 from a recorded draw; 4 with a repeated index (a gather, not a
             permutation); the identity
    HW       1; 5x7; 19x19 (crosses a 256-pixel block inside an image); 363x363 with N = 2, so that npix > 1024 * 256 and
             the forward's grid-stride loop takes a second trip, and with N = 4 (npix > 2048 * 256: the backward's too)
    weights  a recorded alpha = 1 draw; a recorded alpha = 0.2 draw near 0; (1, 0); (0, 1); (0.5, 0.5)
    labels   "same": a == b everywhere; "diff": a != b everywhere; "mixed"; "oob": mixed with some labels equal to K
`golden`: the reference's values are recorded in tests/golden/mixup.npz (not the 363x363 cases: too large to commit; not
the out-of-range labels: the reference's one-hot refuses them).  Those are held to the f64 restatement alone.
"""
from collections import namedtuple

import numpy as np

SEEDS = (0, 1, 2, 3, 7, 10, 123, 4242, 99991, 1234567)  # of the recorded draws
BATCHES = (2, 4, 6)
ALPHAS = (1.0, 0.2)
DRAW_A1 = (0, 1.0)   # (seed, alpha): lam = 0.449...
DRAW_A02 = (7, 0.2)  # lam = 8.97e-6

Loss = namedtuple("Loss", "tag K N H W index weights labels golden")

SWAP, FIXED, REPEAT = (1, 0), (0, 2, 3, 1), (1, 1, 3, 0)
IDENT4 = (0, 1, 2, 3)
DRAW6 = "draw6"  # the index recorded for (seed 3, batch 6): (4, 0, 3, 2, 1, 5)

LOSS_CASES = (
    Loss("k2_hw1_swap", 2, 2, 1, 1, SWAP, DRAW_A1, "mixed", True),
    Loss("k4_hw1_swap", 4, 2, 1, 1, SWAP, (1.0, 0.0), "diff", True),
    Loss("k3_5x7_fixed", 3, 4, 5, 7, FIXED, DRAW_A02, "mixed", True),
    Loss("k8_5x7_ident", 8, 4, 5, 7, IDENT4, DRAW_A02, "same", True),
    Loss("k16_5x7_swap", 16, 2, 5, 7, SWAP, (0.0, 1.0), "mixed", True),
    Loss("k5_5x7_oob", 5, 2, 5, 7, SWAP, DRAW_A1, "oob", False),
    Loss("k4_19_repeat", 4, 4, 19, 19, REPEAT, (0.5, 0.5), "mixed", True),
    Loss("k5_19_draw", 5, 6, 19, 19, DRAW6, DRAW_A1, "mixed", True),
    Loss("k16_19_swap", 16, 2, 19, 19, SWAP, (1.0, 0.0), "diff", True),
    Loss("k2_19_fixed", 2, 4, 19, 19, FIXED, DRAW_A02, "same", True),
    Loss("k8_19_draw", 8, 6, 19, 19, DRAW6, (0.5, 0.5), "mixed", True),
    Loss("k3_19_swap", 3, 2, 19, 19, SWAP, (0.0, 1.0), "diff", True),
    Loss("k2_363_swap", 2, 2, 363, 363, SWAP, DRAW_A1, "mixed", False),
    Loss("k2_363_repeat", 2, 4, 363, 363, REPEAT, DRAW_A02, "mixed", False),
)
LOSS_BY_TAG = {c.tag: c for c in LOSS_CASES}

# image cases: (tag, N, E, index, weights, base): base "aligned", or "slice": the batch starts one float into its buffer
Image = namedtuple("Image", "tag N E index weights base")
IMAGE_CASES = (
    Image("e1", 2, 1, SWAP, DRAW_A1, "aligned"),
    Image("e35", 4, 35, FIXED, DRAW_A02, "aligned"),
    Image("e1444", 4, 4 * 19 * 19, REPEAT, DRAW_A1, "aligned"),
    Image("e1083", 6, 3 * 19 * 19, DRAW6, (0.5, 0.5), "aligned"),
    Image("e1444_slice", 2, 4 * 19 * 19, SWAP, DRAW_A1, "slice"),
    Image("e1444_w10", 4, 4 * 19 * 19, IDENT4, (1.0, 0.0), "aligned"),
    Image("vec_past_cap", 3, 1048580, (2, 0, 0), DRAW_A02, "aligned"),   # N * E / 4 > 2048 * 256
    Image("scalar_past_cap", 2, 349527, SWAP, DRAW_A1, "aligned"),       # E odd, N * E > 2048 * 256
)

HOOK_MIXUP = dict(B=2, K=4, H=19, W=19, weight=0.3, seed=123)  # the 2B = 4 batch of _MixUpEpocherHook
HOOK_ICT = dict(B=2, K=4, H=19, W=19, weight=0.7, seed=4242)   # alpha = 0.2 draw of seed 4242: lam = 0.0049


def _rng(tag: str) -> np.random.RandomState:
    return np.random.RandomState(sum(ord(c) * (i + 1) for i, c in enumerate(tag)) % (2 ** 31))


def logits_i8(case: Loss, which: str) -> np.ndarray:
    """int8 [N,K,H,W] logits on the 1/8 grid (exact in f32); a per-image scale spreads the confidences.  `which`:
    "s" (the logits / the student) or "t" (the teacher)"""
    r = _rng(case.tag + which)
    u = r.standard_normal((case.N, case.K, case.H, case.W))
    s = 0.25 + 2.0 * r.random_sample((case.N, 1, 1, 1))
    return np.clip(np.round(u * s * 8), -48, 48).astype(np.int8)


def labels(case: Loss) -> np.ndarray:
    """int64 [N,H,W].  Image n carries (c_n + position) % K; "same": one c for all images; "diff": c_n = n, which
    differs from its partner's for the case's index (asserted); "mixed": random; "oob": random over [0, K]"""
    N, K, HW = case.N, case.K, case.H * case.W
    pos = np.arange(HW, dtype=np.int64)[None, :]
    if case.labels == "same":
        lab = np.broadcast_to((1 + pos) % K, (N, HW)).copy()
    elif case.labels == "diff":
        c = np.arange(N, dtype=np.int64)[:, None]
        lab = (c + pos) % K
    else:
        lab = _rng(case.tag + "y").randint(0, K + (case.labels == "oob"), size=(N, HW)).astype(np.int64)
    return lab.reshape(N, case.H, case.W)


def image_values(case: Image) -> np.ndarray:
    """f32 [N, E] of full-mantissa values, some negative, with a few exact zeros and tiny values"""
    r = _rng(case.tag)
    x = (r.standard_normal((case.N, case.E)) * np.exp(r.uniform(-8, 8, (case.N, case.E)))).astype(np.float32)
    x[:, :: 17] = 0.0
    return x
