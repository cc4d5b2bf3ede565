"""The cases of the teacher kernels (csrc/cy_teacher.hip) and of the differentiable-mean-teacher hooks, float64
restatements, the reference's compositions in f32 (what the bounds are measured from), the stand-in model and warp of
tests/golden/dmt.npz, and a plain composition of each method.  Shared by tests/golden/gen_goldens_dmt.py,
tests/test_dmt_host.py, tests/test_gpu_dmt_kernels.py and tests/test_gpu_dmt_hooks.py.

Kernel cases: the smallest shapes at which each thing can go wrong.
    Adam      steps 1, 2, 10, 1000, 100000 (both bias corrections saturated); wd 0 and 1e-5; zero gradients
    sizes     Adam and axpy: 1, 255, 256, 257; one element and 257 past a full trip of the capped grid (2048 blocks of
              256 lanes of 4 floats, vector form); a slice whose base is only 4-byte aligned (one float at a time: 257,
              and 257 past ITS full trip of 2048 x 256)
    EMA       counts 1, 2 and 44 tensors of sizes cycling through 1, 32, 33, 512, 100000 (100000 is a second trip of
              the 64 x 256 lanes that stride over one tensor); alpha 0, 0.5, 0.999; wd 0 and 1e-5
    gather    N = 2; K 2, 4, 8 compiled, 3, 5, 13, 16 run-time, 2, 4 and 8 on a 4-byte-aligned base (run-time form);
              images of 17 x 9 and 1 x 1; maps: identity, all outside, random with about a third outside; at K = 2,
              1024 * 256 + 258 pixels (a second trip of the forward's 1024 blocks) and 2048 * 256 + 258 pixels (a second
              trip of the backward's 2048 blocks, a third of the forward's)

Bounds.  The yardstick of a kind is the largest distance from float64, over the kind's cases, of the reference's own
composition evaluated in f32 by torch on the CPU (torch.optim.Adam; Tensor.add_(alpha=); MSELoss of softmax and the
gathered softmax); a kernel may be MARGIN = 4 yardsticks away, because it orders its sums and contracts multiply-adds
differently from torch's CPU code.  A loss's bound is floored at 1.2e-6 as tests/prior_cases.py floors it.  The
yardsticks are computed by the tests from these very cases (the reference's arithmetic runs on the CPU).  Measured
(yardstick from torch 2.10 on x86-64; kernel column from an MI355X, DESIGN.md section 3 has the table):
    kind                yardstick   bound      kernel (largest over the cases)
    adam p              5.07e-8     2.03e-7    4.81e-8
    adam exp_avg        2.93e-7     1.17e-6    7.06e-7   (the one-element case; at most 1.1e-7 elsewhere)
    adam exp_avg_sq     1.02e-7     4.08e-7    1.02e-7
    axpy                3.96e-8     1.58e-7    4.87e-8
    gather loss         1.70e-7     1.20e-6    1.35e-7
    gather grad2        4.13e-7     1.65e-6    4.26e-7
    gather gradmax      7.91e-7     3.16e-6    1.19e-6
The multi-tensor EMA is held to the bits of the per-tensor kernel.  The hooks' yardsticks are recorded in
tests/golden/dmt.npz next to the reference's trajectories (`*_e_ref`): 1.6e-7 to 2.5e-7 (loss), 1.2e-7 to 2.2e-7 (meters),
1.2e-7 to 1.7e-7 (teacher state); the build measured at most 3.2e-7, 3.2e-7 and 1.7e-7.
"""
import copy
from collections import namedtuple
from pathlib import Path

import numpy as np
import torch
from torch import nn

MARGIN = 4.0
LOSS_FLOOR = 1.2e-6

# ---------------------------------------------------------------- the launch rule, restated (cy_teacher_plan)
FLAT_GRID_CAP = 2048
VEC_TRIP = FLAT_GRID_CAP * 256 * 4      # elements of one full trip of the capped grid, 16 bytes per lane
SCALAR_TRIP = FLAT_GRID_CAP * 256       # ... one float per lane
LOSS_BLOCK_CAP = 1024
EMA_ROW_BLOCKS = 64                     # grid.x of the multi-tensor EMA for up to 128 tensors
EMA_MULTI_MAX = 4096

# ---------------------------------------------------------------- Adam / axpy
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8, lr=1e-3)   # torch.optim.Adam(lr=meta_weight) of dmt.py:66
ADAM_STEPS = (1, 2, 10, 1000, 100000)
ADAM_WDS = (0.0, 1e-5)
FLAT_COUNTS = (1, 255, 256, 257, VEC_TRIP + 1, VEC_TRIP + 257)
SLICE_COUNTS = (257, SCALAR_TRIP + 257)   # on a base one float into its buffer
AXPY_ALPHAS = (-1e-3, 1e-3, 0.37)

FlatCase = namedtuple("FlatCase", "n sliced")
FLAT_CASES = tuple(FlatCase(n, False) for n in FLAT_COUNTS) + tuple(FlatCase(n, True) for n in SLICE_COUNTS)


def adam_cases():
    """(step, wd, FlatCase, zero_grad): every step and wd at 257 elements; every size at step 10 with wd 1e-5; zero
    gradients at steps 1 and 10"""
    out = [(st, wd, FlatCase(257, False), False) for st in ADAM_STEPS for wd in ADAM_WDS]
    out += [(10, 1e-5, c, False) for c in FLAT_CASES if c != FlatCase(257, False)]
    out += [(st, wd, FlatCase(257, False), True) for st in (1, 10) for wd in ADAM_WDS]
    return out


def _rng(tag: str) -> np.random.RandomState:
    return np.random.RandomState(sum(ord(c) * (i + 1) for i, c in enumerate(tag)) % (2 ** 31))


def adam_inputs(step: int, n: int, zero_grad: bool):
    """(p, g, m, v) f32 CPU tensors: the moments look like those of `step - 1` earlier updates (zero before step 1)"""
    r = _rng(f"adam{step}_{n}_{zero_grad}")
    p = r.standard_normal(n)
    g = np.zeros(n) if zero_grad else r.standard_normal(n) * np.exp(r.uniform(-6, 1, n))
    if step == 1:
        m, v = np.zeros(n), np.zeros(n)
    else:
        m = r.standard_normal(n) * 0.1
        v = (r.standard_normal(n) * 0.1) ** 2 + 1e-12
    return tuple(torch.from_numpy(a.astype(np.float32)) for a in (p, g, m, v))


def adam64(p, g, m, v, step: int, wd: float, lr=ADAM["lr"], beta1=ADAM["beta1"], beta2=ADAM["beta2"], eps=ADAM["eps"]):
    """torch.optim.Adam(amsgrad=False, maximize=False), one update, in float64 on the f32 values of the scalars"""
    f = lambda x: float(np.float32(x))  # noqa: E731  (the kernel takes its scalars as f32)
    lr, beta1, beta2, eps, wd = f(lr), f(beta1), f(beta2), f(eps), f(wd)
    p, g, m, v = (t.double() for t in (p, g, m, v))
    g = g + wd * p
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps)
    return p, m, v


def adam_torch(p, g, m, v, step: int, wd: float, dtype):
    """the same update by torch.optim.Adam itself in `dtype` on the CPU, walked to `step` by setting its state"""
    param = nn.Parameter(p.to(dtype).clone())
    param.grad = g.to(dtype).clone()
    f = lambda x: float(np.float32(x))  # noqa: E731  (every evaluation reads the f32 values of the scalars)
    opt = torch.optim.Adam([param], lr=f(ADAM["lr"]), betas=(f(ADAM["beta1"]), f(ADAM["beta2"])), eps=f(ADAM["eps"]),
                           weight_decay=f(wd), foreach=False)
    opt.state[param] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.to(dtype).clone(),
                            exp_avg_sq=v.to(dtype).clone())
    opt.step()
    st = opt.state[param]
    return param.detach(), st["exp_avg"], st["exp_avg_sq"]


def rel_max(got, ref) -> float:
    """max |got - ref| / max |ref|"""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def axpy_inputs(n: int):
    r = _rng(f"axpy{n}")
    return (torch.from_numpy(r.standard_normal(n).astype(np.float32)),
            torch.from_numpy((r.standard_normal(n) * np.exp(r.uniform(-4, 2, n))).astype(np.float32)))


def sliced(t: torch.Tensor) -> torch.Tensor:
    """the same values on a base that is one float into its buffer (4-byte aligned only); keeps the device"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    return buf[1:]


# ---------------------------------------------------------------- multi-tensor EMA
EMA_COUNTS = (1, 2, 44)
EMA_SIZES = (1, 32, 33, 512, 100000)
EMA_SETS = ((0.0, 0.0), (0.5, 1e-5), (0.999, 1e-5), (0.999, 0.0))   # (alpha, weight decay)


def ema_size_lists():
    """the tensor sizes of every launch: each size alone, a pair, and 44 tensors cycling through the sizes"""
    return [[n] for n in EMA_SIZES] + [[33, 100000]] + [[EMA_SIZES[i % len(EMA_SIZES)] for i in range(44)]]


def ema_inputs(sizes):
    """[(teacher, student)] f32 CPU tensors"""
    r = _rng("ema" + "_".join(map(str, sizes[:3])) + f"x{len(sizes)}")
    return [(torch.from_numpy(r.standard_normal(n).astype(np.float32)),
             torch.from_numpy(r.standard_normal(n).astype(np.float32))) for n in sizes]


# ---------------------------------------------------------------- gather-MSE
Gather = namedtuple("Gather", "tag K N H W map sliced")
GATHER_CASES = (
    Gather("k2_id", 2, 2, 17, 9, "identity", False),
    Gather("k3_rand", 3, 2, 17, 9, "random", False),
    Gather("k4_rand", 4, 2, 17, 9, "random", False),
    Gather("k5_out", 5, 2, 17, 9, "outside", False),
    Gather("k8_rand", 8, 2, 17, 9, "random", False),
    Gather("k13_rand", 13, 2, 17, 9, "random", False),
    Gather("k16_rand", 16, 2, 17, 9, "random", False),
    Gather("k16_id", 16, 2, 17, 9, "identity", False),
    Gather("k2_slice", 2, 2, 17, 9, "random", True),
    Gather("k8_slice", 8, 2, 17, 9, "random", True),
    Gather("k4_1px", 4, 2, 1, 1, "random1", False),
    Gather("k3_1px_out", 3, 2, 1, 1, "outside", False),
    Gather("k4_slice", 4, 2, 17, 9, "random", True),
    Gather("k2_past_cap", 2, 2, 1, (LOSS_BLOCK_CAP * 256 + 257 + 1) // 2, "random", False),
    Gather("k2_past_bwd_cap", 2, 2, 1, (2 * LOSS_BLOCK_CAP * 256 + 257 + 1) // 2, "random", False),
)
GATHER_BY_TAG = {c.tag: c for c in GATHER_CASES}
assert GATHER_BY_TAG["k2_past_cap"].N * GATHER_BY_TAG["k2_past_cap"].W == LOSS_BLOCK_CAP * 256 + 258


def gather_map(case: Gather) -> torch.Tensor:
    """int32 [N, H*W]: the source pixel of the same image, or -1"""
    HW = case.H * case.W
    r = _rng("map" + case.tag)
    if case.map == "identity":
        m = np.tile(np.arange(HW), (case.N, 1))
    elif case.map == "outside":
        m = np.full((case.N, HW), -1)
    elif case.map == "random1":   # 1 x 1 images: the first inside, the second outside
        m = np.array([[0], [-1]])
    else:
        m = r.randint(0, HW, (case.N, HW))
        m[r.random_sample((case.N, HW)) < 1 / 3] = -1
    return torch.from_numpy(m.astype(np.int32))


def gather_inputs(case: Gather):
    """(teacher, student) f32 logits [N,K,H,W] on the 1/8 grid with a per-image spread, contiguous CPU tensors"""
    r = _rng(case.tag)
    out = []
    for _ in range(2):
        z = r.standard_normal((case.N, case.K, case.H, case.W)) * (0.25 + 2.0 * r.random_sample((case.N, 1, 1, 1)))
        out.append(torch.from_numpy((np.clip(np.round(z * 8), -48, 48) / 8).astype(np.float32)))
    return out


def warp_by_map(x: torch.Tensor, source_map: torch.Tensor) -> torch.Tensor:
    """the nearest-neighbour warp with zero padding as a gather: out[n, c, hw] = x[n, c, map[n, hw]] or 0"""
    N, C = x.shape[:2]
    m = source_map.reshape(N, 1, -1).to(x.device)
    flat = x.reshape(N, C, -1)
    got = flat.gather(2, m.clamp_min(0).long().expand(N, C, -1))
    return (got * (m >= 0).to(x.dtype)).reshape(x.shape)


def gathermse_composed(teacher, source_map, student):
    """the reference's arithmetic (dmt.py:138-146) in the dtype of its inputs"""
    return nn.MSELoss()(warp_by_map(teacher.softmax(1), source_map), student.softmax(1))


def rel_scalar(v, ref) -> float:
    v, ref = float(v), float(ref)
    return abs(v - ref) / max(abs(ref), 1e-300)


def rel_grad(g, ref):
    """(2-norm, max-norm) of g - ref, each relative to the same norm of the float64 gradient"""
    g, ref = g.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    d = g - ref
    return (float(d.norm() / ref.norm().clamp_min(1e-300)), float(d.abs().max() / ref.abs().max().clamp_min(1e-300)))


def gather_reference(case: Gather):
    """(f64 loss, f64 student gradient, [loss, grad2, gradmax] errors of the f32 composition)"""
    t, s = gather_inputs(case)
    m = gather_map(case)
    res = {}
    for dt in (torch.float32, torch.float64):
        leaf = s.to(dt).clone().requires_grad_(True)
        v = gathermse_composed(t.to(dt), m, leaf)
        v.backward()
        res[dt] = (v.detach(), leaf.grad)
    (v32, g32), (v64, g64) = res[torch.float32], res[torch.float64]
    return v64, g64, [rel_scalar(v32, v64), *rel_grad(g32, g64)]


def bound(yardstick: float, loss: bool = False) -> float:
    return max(MARGIN * yardstick, LOSS_FLOOR) if loss else MARGIN * yardstick


# ---------------------------------------------------------------- the stand-in model and step data of dmt.npz
METHODS = ("mt", "method1", "method2", "method4")
CRITERIA = ("ce", "dice")
HOOK = dict(K=4, hidden=3, H=8, W=8, n_labeled=2, n_unlabeled=2, steps=3, weight=0.3, alpha=0.999, weight_decay=1e-5,
            meta_weight=1e-3, seed=1907)


class StandIn(nn.Module):
    """conv1x1 -> BatchNorm2d -> tanh -> conv1x1: smooth, with every kind of teacher state.  The first convolution has
    no bias: in front of a train-mode BatchNorm its gradient is zero but for rounding, and Adam divides a gradient by
    its own size -- the one quantity of this model whose f32 trajectory is noise in the reference itself."""

    def __init__(self, K: int = HOOK["K"], hidden: int = HOOK["hidden"]):
        super().__init__()
        self.conv1 = nn.Conv2d(1, hidden, 1, bias=False)
        self.bn = nn.BatchNorm2d(hidden)
        self.conv2 = nn.Conv2d(hidden, K, 1)
        self.num_classes = K

    def forward(self, x):
        return self.conv2(torch.tanh(self.bn(self.conv1(x))))


def standin_state(seed: int):
    """a float64 state dict of StandIn with weights of order one and non-trivial running statistics"""
    g = torch.Generator().manual_seed(seed)
    model = StandIn()
    sd = model.state_dict()
    for k, v in sd.items():
        if v.is_floating_point():
            w = torch.randn(v.shape, generator=g, dtype=torch.float64)
            sd[k] = (w.abs() * 0.5 + 0.5) if "running_var" in k or k == "bn.weight" else w
    return sd


def hook_data(step: int):
    """(labeled image [2,1,8,8], labeled target [2,1,8,8] int64, unlabeled image [2,1,8,8], source map int32 [2,64]) of
    one step, float64 where floating"""
    h = HOOK
    g = torch.Generator().manual_seed(h["seed"] + step)
    li = torch.randn(h["n_labeled"], 1, h["H"], h["W"], generator=g, dtype=torch.float64)
    lt = torch.randint(0, h["K"], (h["n_labeled"], 1, h["H"], h["W"]), generator=g)
    ui = torch.randn(h["n_unlabeled"], 1, h["H"], h["W"], generator=g, dtype=torch.float64)
    HW = h["H"] * h["W"]
    m = torch.randint(0, HW, (h["n_unlabeled"], HW), generator=g)
    m[torch.rand(h["n_unlabeled"], HW, generator=g) < 0.3] = -1
    return li, lt, ui, m.to(torch.int32)


class Meters(dict):
    """what an epocher hook sees of a MeterInterface: named recorders, and a focus that changes nothing"""

    class _Rec(list):
        def add(self, v):
            self.append(float(v))

    def register_meter(self, name, meter=None):
        self[name] = Meters._Rec()

    def focus_on(self, name):
        import contextlib
        return contextlib.nullcontext()


STUDENT_LR = 0.1


def drive(trainer_hook, student: nn.Module, dtype, device, teacher_state=None, steps: int = HOOK["steps"]):
    """run `steps` consecutive steps of an epocher hook of `trainer_hook` (the reference's or the build's) as an epocher
    would: before_regularization, the hook's loss on the student's logits of the warped unlabeled image, backward, a
    plain gradient step of the student, after_batch_update.  Returns per step (loss, {meter: value}, teacher state
    vector, teacher counters).  `teacher_state`: a state dict the teacher starts from (None: as constructed)."""
    if teacher_state is not None:
        trainer_hook.teacher_model.load_state_dict({k: v.to(device) for k, v in teacher_state.items()})
    hook = trainer_hook()
    hook._epocher = type("Epocher", (), {"num_classes": HOOK["K"], "device": device})()
    hook._epocher_init = True
    hook.meters = Meters()
    hook.configure_meters_given_epocher(hook.meters)
    out = []
    for step in range(steps):
        li, lt, ui, m = hook_data(step)
        li, ui = li.to(device=device, dtype=dtype), ui.to(device=device, dtype=dtype)
        lt, m = lt.to(device), m.to(device)
        warp = lambda x, m=m: warp_by_map(x, m)  # noqa: E731
        for p in student.parameters():
            p.grad = None
        kw = dict(unlabeled_tf_logits=student(warp(ui)), unlabeled_image=ui, seed=step, affine_transformer=warp,
                  labeled_image=li, labeled_target=lt)
        hook.before_regularization(**kw)
        loss = hook._call_implementation(**kw)
        loss.backward()
        with torch.no_grad():
            for p in student.parameters():
                p.sub_(p.grad, alpha=STUDENT_LR)
        hook.after_batch_update(**kw)
        out.append((float(loss.detach()), {k: v[-1] for k, v in hook.meters.items()}, state_vector(trainer_hook.teacher_model),
                    counters(trainer_hook.teacher_model)))
    return out


def new_student(dtype, device):
    model = StandIn().to(dtype)
    model.load_state_dict(standin_state(HOOK["seed"]))
    return model.to(device).train()


def state_vector(model: nn.Module) -> torch.Tensor:
    """every parameter and floating-point buffer of `model` as one float64 CPU vector, in state-dict order"""
    return torch.cat([v.detach().double().cpu().reshape(-1) for v in model.state_dict().values()
                      if v.is_floating_point()])


def counters(model: nn.Module):
    return [int(v) for v in model.state_dict().values() if not v.is_floating_point()]


def load(golden_dir):
    return dict(np.load(Path(golden_dir) / "dmt.npz"))


# ---------------------------------------------------------------- a plain composition of each method
class PlainDMTHook:
    """The four methods written with torch operations only, in the reference's order: per-tensor torch.optim.Adam,
    deepcopy(state_dict()) / load_state_dict, the per-tensor `updater` (an EMAUpdater(update_bn=True)),
    softmax -> warp -> MSELoss.  The teacher's .grad stays None, so gradients come back through autograd.  Duck-typed
    epocher hook: `meters` is a dict of lists."""

    def __init__(self, *, method: str, model, teacher, updater, criterion, weight: float, meta_weight: float,
                 weights_changed=lambda: None):
        """`weights_changed`: called after parameters were written through `.data` (which no version counter sees):
        a teacher with a packed-weight cache wants cyhip.functions.bump_weights_epoch here"""
        self.weights_changed = weights_changed
        self.method, self.model, self.teacher, self.updater = method, model, teacher, updater
        self.criterion, self.weight, self.meta_weight = criterion, weight, meta_weight
        self.meters = {"loss": [], "consistency_loss": [], "teacher_loss": []}
        self.optimizer = None
        if method in ("method1", "method4"):
            self.optimizer = torch.optim.Adam(teacher.parameters(), lr=meta_weight, weight_decay=1e-5, foreach=False)
        self.teacher.train()

    def _consistency(self, unlabeled_tf_logits, unlabeled_image, affine_transformer):
        with torch.no_grad():
            prob = affine_transformer(self.teacher(unlabeled_image).float().softmax(1))
        return nn.MSELoss()(prob, unlabeled_tf_logits.float().softmax(1))

    def _meta(self, labeled_image, labeled_target, training: bool):
        was = self.teacher.training
        self.teacher.train(training)
        logits = self.teacher(labeled_image).float()
        self.teacher.train(was)
        onehot = torch.nn.functional.one_hot(labeled_target.squeeze(1).long(), logits.shape[1]).movedim(-1, 1)
        loss = self.criterion(logits.softmax(1), onehot.to(logits.dtype))
        params = list(self.teacher.parameters())
        grads = torch.autograd.grad(loss, params, allow_unused=True)
        return loss.detach(), [torch.zeros_like(p) if g is None else g for p, g in zip(params, grads)]

    def _adam(self, grads):
        self.last_grads = [g.detach().clone() for g in grads]   # what Adam was handed, for the tests
        for p, g in zip(self.teacher.parameters(), grads):
            p.grad = g.detach().clone()
        self.optimizer.step()
        for p in self.teacher.parameters():
            p.grad = None

    def before_regularization(self, *, unlabeled_image, labeled_image, labeled_target, **kw):
        if self.method != "method4":
            return
        with torch.no_grad():
            self.teacher(unlabeled_image)
        self.ckpt = copy.deepcopy(self.teacher.state_dict())
        loss, grads = self._meta(labeled_image, labeled_target, training=False)
        self._adam(grads)
        self.meters["teacher_loss"].append(loss)

    def __call__(self, *, unlabeled_tf_logits, unlabeled_image, affine_transformer, labeled_image, labeled_target,
                 **kw):
        if self.method == "method2":
            tloss, grads = self._meta(labeled_image, labeled_target, training=False)
            with torch.no_grad():
                for p, g in zip(self.teacher.parameters(), grads):
                    p.data.sub_(g, alpha=self.meta_weight)
            self.weights_changed()
            loss = self._consistency(unlabeled_tf_logits, unlabeled_image, affine_transformer)
            with torch.no_grad():
                for p, g in zip(self.teacher.parameters(), grads):
                    p.data.add_(g, alpha=self.meta_weight)
            self.weights_changed()
            self.meters["teacher_loss"].append(tloss)
        else:
            loss = self._consistency(unlabeled_tf_logits, unlabeled_image, affine_transformer)
        if self.method == "method1":
            self.ckpt = copy.deepcopy(self.teacher.state_dict())
        self.meters["loss" if self.method == "mt" else "consistency_loss"].append(loss.detach())
        return self.weight * loss

    def after_batch_update(self, *, labeled_image, labeled_target, **kw):
        if self.method == "method1":
            self.updater(ema_model=self.teacher, student_model=self.model)
            loss, grads = self._meta(labeled_image, labeled_target, training=True)
            self.teacher.load_state_dict(self.ckpt)
            self._adam(grads)
            self.meters["teacher_loss"].append(loss)
            return
        if self.method == "method4":
            self.teacher.load_state_dict(self.ckpt)
        self.updater(ema_model=self.teacher, student_model=self.model)
