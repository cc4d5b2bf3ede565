"""The cases of the flat-buffer optimizer kernels (csrc/cy_optim.hip: cy_sgd_step, cy_adamw_step), float64 restatements
of torch.optim.SGD / Adam / AdamW's single-tensor update, and torch.optim itself walked to a given step (what the bounds
are measured from).  Shared by tests/test_optim_host.py, tests/test_gpu_optim_kernels.py and tests/test_gpu_optim_step.py.

Kernel cases: the smallest shapes at which each thing can go wrong.
    SGD       plain; wd 1e-4; momentum 0.9 + wd; nesterov; dampening 0.1
    Adam(W)   AdamW wd 1e-2 with and without amsgrad; Adam amsgrad with wd 1e-5
    steps     1, 2, 10, 1000, 100000 (both bias corrections saturated); at step 1 the state is zero and SGD's `first` is
              set; zero gradients at steps 1 and 10
    sizes     1, 255, 256, 257; one element and 257 past a full trip of the capped grid (2048 blocks of 256 lanes of 4
              floats, vector form); a base that is only 4-byte aligned (one float at a time: 257, and 257 past ITS full
              trip of 2048 x 256)
    Every step and configuration runs at 257 elements; every size runs at step 10, with and without the optional buffer
    (SGD's momentum buffer, amsgrad's maximum), because the kernels differ there.

Bounds (the rule of tests/dmt_cases.py).  Per kernel and per output (p and each state buffer) the yardstick is the
largest `rel_max` distance from the float64 restatement of torch.optim's own f32 single-tensor update on the CPU
(foreach=False) over these very cases; a kernel may be MARGIN = 4 yardsticks away, because it contracts multiply-adds
and orders operations differently from torch's CPU code; the bound is floored at 2^-23, one f32 rounding.  The tests
compute the yardsticks and print every figure before asserting.  Measured (yardstick from torch 2.10 on x86-64; kernel
column from an MI355X, DESIGN.md section 3 has the table):
    kind                    yardstick   bound      kernel (largest over the cases)
    sgd p                   5.04e-8     2.02e-7    5.04e-8
    sgd momentum_buffer     7.93e-8     3.17e-7    8.26e-8
    adamw p                 1.03e-7     4.13e-7    1.03e-7
    adamw exp_avg           9.91e-8     3.96e-7    9.91e-8
    adamw exp_avg_sq        7.64e-8     3.05e-7    6.14e-8
    adamw max_exp_avg_sq    6.14e-8     2.46e-7    6.14e-8
"""
import functools
from collections import namedtuple

import numpy as np
import torch
from torch import nn

from dmt_cases import FLAT_CASES, FLAT_GRID_CAP, MARGIN, FlatCase, rel_max  # noqa: F401  (FLAT_GRID_CAP: the host test)

BOUND_FLOOR = 2.0 ** -23
STEPS = (1, 2, 10, 1000, 100000)
AT_257 = FlatCase(257, False)

Sgd = namedtuple("Sgd", "tag lr momentum dampening wd nesterov")
SGD_CONFIGS = (
    Sgd("plain", 0.05, 0.0, 0.0, 0.0, False),
    Sgd("wd", 0.05, 0.0, 0.0, 1e-4, False),
    Sgd("mom_wd", 0.05, 0.9, 0.0, 1e-4, False),
    Sgd("nesterov", 0.05, 0.9, 0.0, 1e-4, True),
    Sgd("damp", 0.05, 0.9, 0.1, 0.0, False),
)
Adamw = namedtuple("Adamw", "tag lr beta1 beta2 eps wd decoupled amsgrad")
ADAMW_CONFIGS = (
    Adamw("adamw", 1e-3, 0.9, 0.999, 1e-8, 1e-2, True, False),
    Adamw("adamw_ams", 1e-3, 0.9, 0.999, 1e-8, 1e-2, True, True),
    Adamw("adam_ams", 1e-3, 0.9, 0.999, 1e-8, 1e-5, False, True),
)
SIZE_CONFIGS = {"sgd": ("plain", "mom_wd"), "adamw": ("adamw", "adamw_ams")}   # without / with the optional buffer

Case = namedtuple("Case", "cfg step flat zero")


def _cases(configs, size_tags):
    out = [Case(c, st, AT_257, False) for c in configs for st in STEPS]
    out += [Case(c, 10, f, False) for c in configs if c.tag in size_tags for f in FLAT_CASES if f != AT_257]
    out += [Case(c, st, AT_257, True) for c in configs for st in (1, 10)]
    return out


def sgd_cases():
    return _cases(SGD_CONFIGS, SIZE_CONFIGS["sgd"])


def adamw_cases():
    return _cases(ADAMW_CONFIGS, SIZE_CONFIGS["adamw"])


def case_id(c: Case) -> str:
    return f"{c.cfg.tag}-s{c.step}-n{c.flat.n}{'-slice' if c.flat.sliced else ''}{'-zero' if c.zero else ''}"


def _rng(tag: str) -> np.random.RandomState:
    return np.random.RandomState(sum(ord(ch) * (i + 1) for i, ch in enumerate(tag)) % (2 ** 31))


def _f32(*arrays):
    return tuple(torch.from_numpy(a.astype(np.float32)) for a in arrays)


def _f(x) -> float:
    """the f32 value of a scalar: the kernels take their scalars as f32, and every evaluation reads those values"""
    return float(np.float32(x))


def _grad(r, n, zero):
    return np.zeros(n) if zero else r.standard_normal(n) * np.exp(r.uniform(-6, 1, n))


# ---------------------------------------------------------------- SGD
def sgd_inputs(c: Case):
    """(p, g, buf) f32 CPU tensors; buf is None without momentum; zero before step 1 (and not read: `first`)"""
    n = c.flat.n
    r = _rng(f"sgd{c.step}_{n}_{c.zero}")
    p, g = r.standard_normal(n), _grad(r, n, c.zero)
    buf = np.zeros(n) if c.step == 1 else r.standard_normal(n) * 0.1
    p, g, buf = _f32(p, g, buf)
    return p, g, (buf if c.cfg.momentum != 0 else None)


def sgd64(p, g, buf, cfg: Sgd, first: bool):
    """torch.optim.SGD(maximize=False), one update, in float64 on the f32 values of the scalars -> (p, buf or None)"""
    lr, mom, damp, wd = _f(cfg.lr), _f(cfg.momentum), _f(cfg.dampening), _f(cfg.wd)
    p, g = p.double(), g.double()
    if wd != 0:
        g = g + wd * p
    if mom != 0:
        buf = g.clone() if first else mom * buf.double() + (1 - damp) * g
        g = g + mom * buf if cfg.nesterov else buf
    return p - lr * g, (buf if mom != 0 else None)


def sgd_torch(p, g, buf, cfg: Sgd, first: bool, dtype):
    """the same update by torch.optim.SGD itself (single-tensor form) in `dtype` on the CPU"""
    param = nn.Parameter(p.to(dtype).clone())
    param.grad = g.to(dtype).clone()
    opt = torch.optim.SGD([param], lr=_f(cfg.lr), momentum=_f(cfg.momentum), dampening=_f(cfg.dampening),
                          weight_decay=_f(cfg.wd), nesterov=cfg.nesterov, foreach=False)
    if cfg.momentum != 0 and not first:
        opt.state[param] = dict(momentum_buffer=buf.to(dtype).clone())
    opt.step()
    return param.detach(), (opt.state[param]["momentum_buffer"] if cfg.momentum != 0 else None)


# ---------------------------------------------------------------- Adam / AdamW
def adamw_inputs(c: Case):
    """(p, g, m, v, vmax) f32 CPU tensors: the moments look like those of `step - 1` earlier updates (zero before
    step 1); vmax (None without amsgrad) lies on either side of v, so both arms of the maximum are taken"""
    n = c.flat.n
    r = _rng(f"adamw{c.step}_{n}_{c.zero}")
    p, g = r.standard_normal(n), _grad(r, n, c.zero)
    if c.step == 1:
        m, v, vmax = np.zeros(n), np.zeros(n), np.zeros(n)
    else:
        m = r.standard_normal(n) * 0.1
        v = (r.standard_normal(n) * 0.1) ** 2 + 1e-12
        vmax = v * np.exp(r.uniform(-0.5, 0.5, n))
    p, g, m, v, vmax = _f32(p, g, m, v, vmax)
    return p, g, m, v, (vmax if c.cfg.amsgrad else None)


def adamw64(p, g, m, v, vmax, cfg: Adamw, step: int):
    """torch.optim.Adam / AdamW(maximize=False), one update, in float64 on the f32 values of the scalars
    -> (p, m, v, vmax or None)"""
    lr, b1, b2, eps, wd = _f(cfg.lr), _f(cfg.beta1), _f(cfg.beta2), _f(cfg.eps), _f(cfg.wd)
    p, g, m, v = (t.double() for t in (p, g, m, v))
    if cfg.decoupled:
        p = p * (1 - lr * wd)
    elif wd != 0:
        g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    vd = v
    if cfg.amsgrad:
        vmax = vd = torch.maximum(vmax.double(), v)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p = p - (lr / bc1) * m / (vd.sqrt() / bc2 ** 0.5 + eps)
    return p, m, v, (vmax if cfg.amsgrad else None)


def adamw_torch(p, g, m, v, vmax, cfg: Adamw, step: int, dtype):
    """the same update by torch.optim.Adam / AdamW itself (single-tensor form) in `dtype` on the CPU, walked to `step`
    by setting its state"""
    param = nn.Parameter(p.to(dtype).clone())
    param.grad = g.to(dtype).clone()
    cls = torch.optim.AdamW if cfg.decoupled else torch.optim.Adam
    opt = cls([param], lr=_f(cfg.lr), betas=(_f(cfg.beta1), _f(cfg.beta2)), eps=_f(cfg.eps), weight_decay=_f(cfg.wd),
              amsgrad=cfg.amsgrad, foreach=False)
    st = dict(step=torch.tensor(float(step - 1)), exp_avg=m.to(dtype).clone(), exp_avg_sq=v.to(dtype).clone())
    if cfg.amsgrad:
        st["max_exp_avg_sq"] = vmax.to(dtype).clone()
    opt.state[param] = st
    opt.step()
    st = opt.state[param]
    return param.detach(), st["exp_avg"], st["exp_avg_sq"], st.get("max_exp_avg_sq")


# ---------------------------------------------------------------- yardsticks and bounds
SGD_OUTPUTS = ("p", "momentum_buffer")
ADAMW_OUTPUTS = ("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def worst_over(outputs, triples):
    """{output: largest rel_max} over (got tuple, ref tuple) pairs; an output a case does not have is None in both"""
    worst = dict.fromkeys(outputs, 0.0)
    for got, ref in triples:
        for k, a, b in zip(outputs, got, ref):
            if b is not None:
                worst[k] = max(worst[k], rel_max(a, b))
    return worst


@functools.lru_cache(maxsize=None)
def sgd_yardstick():
    """torch.optim.SGD in f32 on the CPU against float64, the largest over the cases, per output"""
    def pairs():
        for c in sgd_cases():
            ins = sgd_inputs(c)
            yield sgd_torch(*ins, c.cfg, c.step == 1, torch.float32), sgd64(*ins, c.cfg, c.step == 1)
    worst = worst_over(SGD_OUTPUTS, pairs())
    print("SGD yardstick:", {k: f"{e:.3g}" for k, e in worst.items()})
    return worst


@functools.lru_cache(maxsize=None)
def adamw_yardstick():
    """torch.optim.Adam / AdamW in f32 on the CPU against float64, the largest over the cases, per output"""
    def pairs():
        for c in adamw_cases():
            ins = adamw_inputs(c)
            yield adamw_torch(*ins, c.cfg, c.step, torch.float32), adamw64(*ins, c.cfg, c.step)
    worst = worst_over(ADAMW_OUTPUTS, pairs())
    print("Adam(W) yardstick:", {k: f"{e:.3g}" for k, e in worst.items()})
    return worst


def bound(yardstick: float) -> float:
    return max(MARGIN * yardstick, BOUND_FLOOR)
