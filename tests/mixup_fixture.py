"""Layout and decoding of tests/golden/mixup.npz (written by tests/golden/gen_goldens_mixup.py): the reference's
`mixup_data` draws (semi_seg/hooks/utils.py:284-297), its MixUp loss `KL_div()(softmax, mixed one-hot)`
(semi_seg/hooks/mixup.py:49-58) and ICT loss `MSELoss(reduction="none")(...).mean()` (semi_seg/hooks/mt.py:301-319)
with their input gradients, and the `_call_implementation` of `_MixUpEpocherHook` and `_ICTMeanTeacherEpocherHook`,
evaluated on the CPU in f32 and in f64.  The cases are those of tests/mixup_cases.py.

    draw_lam [seed, batch, alpha] f64, draw_index_b<batch> [seed, alpha, batch] int64
                              the (lam, index) `mixup_data` draws under `fix_all_seed_within_context(seed)`
per golden loss case <tag>:
    <tag>_s_i8d8, <tag>_t_i8d8 [N,K,H,W]  int8 logits on the 1/8 grid, exact in f32 (the logits / student; the teacher)
    <tag>_y [N,H,W]           integer labels
    <tag>_kl64, <tag>_mse64   the two losses in f64;  <tag>_gkl64, <tag>_gmse64  their gradients (f64, stored as f32)
    <tag>_kl_e_ref, <tag>_mse_e_ref   the reference's own f32-to-f64 distances [scalar, gradient 2-norm, gradient
                              max-norm], all relative
hooks: mixup_* and ict_*: images and labels, the stand-in model's weights (`*_w`, `*_b`: a fixed 1x1 convolution of the
one-channel image), value64, the gradients of the weights, the meter readings, e_ref.

The tolerance of a kind is max(4 * the largest stored e_ref of that kind, 1e-6) (`tolerances`): a kernel may be four
times as far from f64 as the reference's own f32 evaluation is, with a floor for the kinds where that is 0.
"""
from pathlib import Path

import numpy as np
import torch

import mixup_cases as mc

EPS = 1e-16  # KL_div's default, which the MixUp hook uses
KINDS = ("scalar", "grad2", "gradmax")


def load(golden_dir):
    return dict(np.load(Path(golden_dir) / "mixup.npz"))


def decode(arr) -> torch.Tensor:
    return torch.from_numpy(np.asarray(arr).astype(np.float32) / 8.0)


def recorded_draw(npz, seed: int, batch: int, alpha: float):
    """(lam, index tuple) the reference drew"""
    s, a = mc.SEEDS.index(seed), mc.ALPHAS.index(alpha)
    return float(npz["draw_lam"][s, mc.BATCHES.index(batch), a]), tuple(int(v) for v in npz[f"draw_index_b{batch}"][s, a])


def weights_of(npz, spec):
    """(w_self, w_other) as Python floats: lam and 1 - lam in f64 (the kernels and torch round each to f32).  spec: a
    literal pair, or the (seed, alpha) of a recorded draw (lam does not depend on the batch size)"""
    if spec in (mc.DRAW_A1, mc.DRAW_A02):
        lam, _ = recorded_draw(npz, spec[0], 2, spec[1])
        return lam, 1.0 - lam
    return float(spec[0]), float(spec[1])


def index_of(npz, spec, N: int) -> torch.Tensor:
    if spec == mc.DRAW6:
        spec = recorded_draw(npz, 3, 6, 1.0)[1]
    assert len(spec) == N
    return torch.tensor(spec, dtype=torch.int64)


def case_inputs(npz, case):
    """(student/logits f32 [N,K,H,W], teacher f32, labels int64 [N,H,W], index int64 [N], (w_self, w_other)); golden
    cases read the stored arrays, which the CPU tests hold equal to what mixup_cases builds"""
    if case.golden:
        s, t, y = npz[f"{case.tag}_s_i8d8"], npz[f"{case.tag}_t_i8d8"], npz[f"{case.tag}_y"].astype(np.int64)
    else:
        s, t, y = mc.logits_i8(case, "s"), mc.logits_i8(case, "t"), mc.labels(case)
    return decode(s), decode(t), torch.from_numpy(y), index_of(npz, case.index, case.N), weights_of(npz, case.weights)


def f32w(w: float) -> float:
    """a weight as every f32 evaluation sees it"""
    return float(np.float32(w))


# ---- the three formulas in f64 torch, differentiable ----------------------------------------------------------------
def mix_images64(x, index, w_self, w_other):
    return f32w(w_self) * x.double() + f32w(w_other) * x.double()[index]


def mixkl64(logits, target, index, w_self, w_other, eps=EPS):
    """sum_pix l / npix with l = -sum_{k in {a, b}} t_k log((p_k + eps) / (t_k + eps)), a = target[pix], b the partner
    image's label, t_a = w_self, t_b = w_other in f32 (a == b: the one term with their f32 sum); a weight of 0 adds 0 and
    a label outside [0, K) selects no class (p = 0)"""
    p = torch.softmax(logits.double(), 1)
    K = p.shape[1]
    ws, wo = np.float32(w_self), np.float32(w_other)

    def pick(lab):
        inside = (lab >= 0) & (lab < K)
        return torch.where(inside, p.gather(1, lab.clamp(0, K - 1).unsqueeze(1)).squeeze(1), torch.zeros_like(p[:, 0]))

    def term(w, pk):
        w = float(w)
        return torch.zeros_like(pk) if w == 0.0 else -w * torch.log((pk + eps) / (w + eps))

    a, b = target, target[index]
    pa, pb = pick(a), pick(b)
    return torch.where(a == b, term(ws + wo, pa), term(ws, pa) + term(wo, pb)).mean()


def mixmse64(student, teacher, index, w_self, w_other):
    p = torch.softmax(student.double(), 1)
    q = torch.softmax(teacher.double(), 1)
    m = f32w(w_self) * q + f32w(w_other) * q[index]
    return ((p - m) ** 2).mean()


def grad_of(fn, x, *args):
    x = x.detach().double().clone().requires_grad_(True)
    v = fn(x, *args)
    v.backward()
    return v.detach(), x.grad


# ---- distances -----------------------------------------------------------------------------------------------------
def rel_scalar(v, v64) -> float:
    v64 = float(v64)
    return abs(float(v) - v64) / abs(v64)


def rel_grad(g, g64):
    """[2-norm, max-norm] distance of g from g64, relative, over all elements"""
    g64 = torch.as_tensor(g64, dtype=torch.float64).flatten()
    d = torch.as_tensor(g, dtype=torch.float64).flatten() - g64
    return [float(d.norm() / g64.norm()), float(d.abs().max() / g64.abs().max())]


def distances(v, g, v64, g64):
    return dict(zip(KINDS, [rel_scalar(v, v64)] + rel_grad(g, g64)))


def tolerances(npz) -> dict:
    worst = np.max(np.stack([v for k, v in npz.items() if k.endswith("e_ref")]), axis=0)
    return {kind: max(4.0 * float(w), 1e-6) for kind, w in zip(KINDS, worst)}


# ---- the hooks' stand-in model ---------------------------------------------------------------------------------------
class Conv1x1(torch.nn.Module):
    """logits_k = w_k * image + b_k on a one-channel image: a fixed 1x1 convolution written out, so that every
    implementation evaluates the same two operations"""

    def __init__(self, w, b, dtype=torch.float32):
        super().__init__()
        self.w = torch.nn.Parameter(torch.as_tensor(np.asarray(w)).to(dtype).reshape(1, -1, 1, 1))
        self.b = torch.nn.Parameter(torch.as_tensor(np.asarray(b)).to(dtype).reshape(1, -1, 1, 1))
        self.num_classes = self.w.shape[1]

    def forward(self, x):
        return x * self.w + self.b
