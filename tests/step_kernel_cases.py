"""The cases tests/test_gpu_step_kernels.py is parametrised with, and what tests/test_step_kernel_coverage.py requires of
them: the four kernels of csrc/cy_misc.hip that run in every training step (affine_fwd_kernel, affine_bwd_kernel,
ema_kernel, radam_kernel) and contrastyou/optim/fused_radam.py, which drives the last.
A plain module: no GPU, no torch and no library call at import.

Every shape is the smallest that reaches its edge.  The launch cap is restated below FOR COVERAGE ONLY, next to a
pointer at its source line; no expected value of the GPU file comes from it.

Two tolerances are measured, not derived (powf on the device, and the RAdam step as a whole): `yardstick` is the error
of torch's own f32 CPU operator against the float64 reference on the same inputs, measured once with the `yardstick_*`
functions of the GPU file; the bound is 4 x yardstick.  Everything else is compared exactly or at a bound derived from
the number of f32 roundings (see the GPU file)."""
import math
import struct
from collections import namedtuple

TYPES = ("f32", "bf16", "f16")

# ---------------------------------------------------------------- restated launch geometry (coverage only)
GRID_CAP = 8192             # cy_misc.hip: `constexpr int GRID_CAP = 8192;`, the cap of every cy_blocks(items, 256, GRID_CAP)
ONE_TRIP = GRID_CAP * 256   # items one trip of the grid-stride loops covers (256 threads per workgroup)


def f32(v):
    """the value a C `float` argument holds"""
    return struct.unpack("f", struct.pack("f", v))[0]


# ---------------------------------------------------------------- EMA / RAdam element counts
# 1 thread, one short of / exactly / one past a workgroup, exactly one trip, and a second trip taken by one full
# workgroup and one thread of the next
ELEMENT_COUNTS = (1, 255, 256, 257, ONE_TRIP, ONE_TRIP + 257)
SLICE_OFF = 3               # kernels act on [off : off + n] of a larger buffer; the rest are guard elements
GUARD = 5                   # guard elements behind the slice
EMA_ALPHAS = (0.0, 0.5, 0.999)
EMA_WDS = (0.0, 1e-5)

# ---------------------------------------------------------------- affine geometries
Geom = namedtuple("Geom", "N C H W")
AFFINE_GEOMS = (
    Geom(3, 12, 10, 23), Geom(3, 12, 23, 10),   # non-square both ways; one full channel group and a 4-channel tail
    Geom(2, 4, 16, 16),                         # the class-logit case: one channel group that is a 4-channel tail
    Geom(2, 1, 16, 16), Geom(2, 8, 7, 9), Geom(2, 20, 7, 9),
    Geom(1, 3, 1, 1), Geom(1, 3, 1, 9), Geom(1, 3, 9, 1),
)
# N * H * W * ceil(C / 8) = 3 * 592 * 592 * 2 = 2 102 784 items > ONE_TRIP = 2 097 152, with a tail group
AFFINE_CAP = Geom(3, 12, 592, 592)
AFFINE_CAP_TYPE = "bf16"
GAMMA_GEOMS = (Geom(4, 1, 7, 9), Geom(4, 4, 7, 9), Geom(4, 12, 7, 9))   # one gamma per image
GAMMAS = (0.5, 1.0, 1.7, 2.0)


def make_theta_rows(scale, rot_deg, tx, ty, flip_h, flip_w):
    """oracle.losses.make_theta without torch (the coverage file asserts that the two agree bit for bit)"""
    a = math.radians(rot_deg)
    c, s = math.cos(a) / scale, math.sin(a) / scale
    m = [[f32(c), f32(-s), f32(tx)], [f32(s), f32(c), f32(ty)]]
    if flip_w:
        m[0][0], m[1][0] = -m[0][0], -m[1][0]
    if flip_h:
        m[0][1], m[1][1] = -m[0][1], -m[1][1]
    return tuple(tuple(r) for r in m)


def _rows(m):
    return tuple(tuple(f32(v) for v in r) for r in m)


def det(m):
    """exact determinant of the f32 entries (a product of two f32 values is exact in f64; the difference is rounded once)"""
    return m[0][0] * m[1][1] - m[0][1] * m[1][0]


_NEAR_ROW = (0.9, 0.4, 0.02)
_NEAR = _rows([_NEAR_ROW, [v * (1 + 1e-6) for v in _NEAR_ROW]])

Theta = namedtuple("Theta", "name rows kind note")
# kind: "production" (the parameter ranges of the augmentation), "wide" (invertible, outside them), "outside" (no source
# inside the image), "singular" (determinant zero or next to it)
THETAS = (
    Theta("identity", _rows([[1, 0, 0], [0, 1, 0]]), "production", ""),
    # the four thetas of tests/test_gpu_kernels.py::test_affine_fwd_bwd
    Theta("prod-identity", make_theta_rows(1.0, 0.0, 0.0, 0.0, False, False), "production", "a -0.0 entry"),
    Theta("prod-1.25-30-flipw", make_theta_rows(1.25, 30.0, 0.08, -0.05, False, True), "production", ""),
    Theta("prod-0.82-m41-fliph", make_theta_rows(0.82, -41.0, -0.1, 0.1, True, False), "production", ""),
    Theta("prod-1.1-12-flipboth", make_theta_rows(1.1, 12.0, 0.02, 0.03, True, True), "production", ""),
    Theta("scale-0.25", make_theta_rows(0.25, 0.0, 0.0, 0.0, False, False), "wide",
          "entries 4: every 4th source pixel is picked, the others receive nothing; 1/16 of the output is inside"),
    Theta("scale-4", make_theta_rows(4.0, 0.0, 0.0, 0.0, False, False), "wide",
          "entries 0.25: about 16 output pixels per source pixel"),
    Theta("anisotropic-shear", _rows([[1.7, 0.6, 0.05], [-0.2, 0.45, -0.1]]), "wide", ""),
    Theta("half-pixel", _rows([[1, 0, 1 / 16], [0, 1, 0]]), "wide",
          "px = ox + 0.5 exactly at W = 16: round-half-to-even ties"),
    Theta("translate-3", _rows([[1, 0, 3.0], [0, 1, 0]]), "outside", "output and dx all zero"),
    Theta("rank-1", _rows([[1, 1, 0], [1, 1, 0]]), "singular", "every pick on the diagonal"),
    Theta("rank-0", _rows([[0, 0, 0.1], [0, 0, -0.1]]), "singular", "every pick on one pixel"),
    Theta("near-singular", _NEAR, "singular",
          f"second row = first row * (1 + 1e-6), rounded to f32; exact determinant of the f32 entries {det(_NEAR):.3e}"),
)
THETA_NAMES = tuple(t.name for t in THETAS)
PRODUCTION_THETAS = tuple(t for t in THETAS if t.kind == "production")


def batch_thetas(k, N, thetas=THETAS):
    """image n of case k runs under theta (k + n) % len: every theta meets every image index and every batch mixes them"""
    return [thetas[(k + n) % len(thetas)] for n in range(N)]


# ---------------------------------------------------------------- gamma
# yardstick: max relative error of torch's CPU f32 `x ** g` against float64 on the inputs of the gamma test
# (yardstick_gamma of the GPU file); measured 5.80e-8.  The device (powf of affine_fwd_kernel, f32) measured 1.08e-7.
GAMMA_YARDSTICK = 5.80e-8
GAMMA_BOUND = 4 * GAMMA_YARDSTICK

# ---------------------------------------------------------------- RAdam
RAdamSet = namedtuple("RAdamSet", "name beta1 beta2 eps wd lr")
RADAM_SETS = (
    RAdamSet("trainer", 0.9, 0.999, 1e-8, 1e-5, 1e-3),
    RAdamSet("trainer-wd0", 0.9, 0.999, 1e-8, 0.0, 1e-3),
    RAdamSet("fast", 0.8, 0.99, 1e-6, 1e-2, 1e-2),
    RAdamSet("never-rectified", 0.9, 0.5, 1e-8, 0.0, 1e-3),   # rho_inf = 3
)
RADAM_LONG_STEPS = (1000, 100000)   # 100 000: both bias corrections have saturated
RADAM_COUNTS_ALL_SETS = (257, ONE_TRIP + 257)


def rho_inf(beta2):
    return 2.0 / (1.0 - f32(beta2)) - 1.0


def rho_t(beta2, step):
    """cy_misc.hip, cy_radam_step(): `rho_t = rho_inf - 2.0 * (double)step * b2t / bc2` on the f32 value of beta2"""
    b2t = math.pow(f32(beta2), float(step))
    return rho_inf(beta2) - 2.0 * step * b2t / (1.0 - b2t)


def rectified(beta2, step):
    return rho_t(beta2, step) > 5.0   # cy_radam_step(): `if (rho_t > 5.0)`


def first_rectified_step(beta2, limit=10 ** 6):
    """rho_t rises with the step and stays below rho_inf: a set with rho_inf <= 5 never rectifies"""
    if rho_inf(beta2) <= 5.0:
        return None
    return next(t for t in range(1, limit) if rectified(beta2, t))


def radam_steps(s):
    """step 1, the last un-rectified step, the first rectified one, the one after it, and the long runs"""
    t = first_rectified_step(s.beta2)
    around = (1, 2) if t is None else (1, t - 1, t, t + 1)
    return tuple(sorted({st for st in around + RADAM_LONG_STEPS if st >= 1}))


def radam_cases():
    """(set, step, n): every set at 257 and past the cap, the trainer's set at every other count too"""
    out = []
    for s in RADAM_SETS:
        counts = ELEMENT_COUNTS if s.name == "trainer" else RADAM_COUNTS_ALL_SETS
        out += [(s, st, n) for st in radam_steps(s) for n in counts]
    return out


# yardstick: torch.optim.RAdam in f32 on the CPU against the float64 transcription, same inputs, walked to the step by
# setting its state; max over radam_cases() of max|err| / max|ref| per output (yardstick_radam of the GPU file).
# measured p 2.16e-7, exp_avg 6.68e-8, exp_avg_sq 6.04e-8; the device measured p 1.65e-7,
# exp_avg 6.68e-8, exp_avg_sq 4.78e-8
RADAM_YARDSTICK = {"p": 2.16e-7, "exp_avg": 6.68e-8, "exp_avg_sq": 6.04e-8}
RADAM_BOUND = {k: 4 * v for k, v in RADAM_YARDSTICK.items()}

# ---------------------------------------------------------------- FusedRAdam end to end
FUSED_SHAPES = ((5, 7), (7,), (3, 7))   # flat offsets 0, 35, 42
FUSED_STEPS = 12
FUSED_SKIP_UNTIL = 3                    # the second parameter takes no part in the loss for steps 1..3
FUSED_RESUME_AFTER = 6
FUSED_LR, FUSED_WD = 1e-2, 1e-5

# ---------------------------------------------------------------- rejections: (what, expected status)
ERR_ARG, ERR_SHAPE, ERR_DTYPE = -1, -2, -3
REJECTS = ("radam step 0", "radam n 0", "ema n 0", "affine fwd dtype 7", "affine bwd dtype 7", "affine fwd C 0",
           "affine bwd C 0")


def ident(c):
    return c if isinstance(c, str) else c.name if hasattr(c, "name") else "x".join(str(v) for v in c)
