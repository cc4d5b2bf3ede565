"""Float64 CPU references of tests/test_gpu_patch_losses.py, written from the formulas of include/contrastyou_hip.h and
of the losses' docstrings (not from the code under test), each computed once per case and shared; and the comparisons.
"""
import math

import torch
import torch.nn.functional as F

import patch_losses_fixture as fx

# beyond the fixture, J only: twelve images so that a block of the staged forward walks more than one tile
# (16 patches * 6 groups -> 11 blocks per (patch, group) for 12 tiles); (n, k, H, W, patch, pad)
MULTI_TRIP = (12, 4, 40, 33, 16, 3)


def origins(L, p):
    from contrastyou.losses.discreteMI import patch_origins
    return patch_origins(L, p, p // 2)


def patch_joints64(x1, x2, patch, pad):
    """x1, x2: [n,k,H,W] -> J f64 [P, T*T, k, k]:  J[q][d][i][j] = sum_n sum_{(h,w) in q} x1[n,i,h+du,w+dv] x2[n,j,h,w],
    a term counting only if (h+du, w+dv) lies in patch q too; d = (du+pad)*T + (dv+pad); patches rows first"""
    x1, x2 = x1.double(), x2.double()
    n, k, H, W = x1.shape
    T = 2 * pad + 1
    out = []
    for h0 in origins(H, patch):
        for w0 in origins(W, patch):
            a = x1[:, :, h0:min(h0 + patch, H), w0:min(w0 + patch, W)]
            b = x2[:, :, h0:min(h0 + patch, H), w0:min(w0 + patch, W)]
            eh, ew = a.shape[2:]
            ap = F.pad(a, (pad, pad, pad, pad))
            J = [torch.einsum("nihw,njhw->ij", ap[:, :, u:u + eh, v:v + ew], b) for u in range(T) for v in range(T)]
            out.append(torch.stack(J))
    return torch.stack(out)


def patch_losses64(J, pad, lamda, eps):
    """J f64 [P,TT,k,k] (differentiable; padding 0: already scaled by 1 / (n eh ew)) -> (mean loss, losses [P], final
    joints [P,TT,k,k])"""
    TT = J.shape[1]
    if pad > 0:
        p = J - J.amin(dim=(1, 2, 3), keepdim=True).detach() + 1e-8
        p = p / p.sum(dim=(2, 3), keepdim=True)
        p = p / p.sum(dim=(1, 2, 3), keepdim=True)
    else:
        p = J
    pi, pj = p.sum(dim=2, keepdim=True), p.sum(dim=3, keepdim=True)
    loss = -p * (torch.log(p + eps) - lamda * torch.log(pi + eps) - lamda * torch.log(pj + eps))
    losses = loss.sum(dim=(1, 2, 3)) / TT
    return losses.mean(), losses, p


def patch_reference(x1, x2, patch, pad, lamda, eps):
    """-> dict of f64 CPU tensors: J, loss, losses, P, dJ (= d loss / d J), g1, g2 (in the inputs' [n,k,H,W] shape)"""
    a, b = (t.double().clone().requires_grad_(True) for t in (x1, x2))
    n, _, H, W = x1.shape
    J = patch_joints64(a, b, patch, pad) * (1.0 / (n * min(H, patch) * min(W, patch)) if pad == 0 else 1.0)
    J.retain_grad()
    loss, losses, p = patch_losses64(J, pad, lamda, eps)
    loss.backward()
    return dict(J=J.detach(), loss=loss.detach(), losses=losses.detach(), P=p.detach(), dJ=J.grad, g1=a.grad, g2=b.grad)


def puiseg64(x1, x2, lamda, pad):
    """PUISegLoss as its docstring states it, f64, differentiable"""
    n, k, H, W = x1.shape
    T = 2 * pad + 1
    ap = F.pad(x1, (pad, pad, pad, pad))
    J = torch.stack([torch.einsum("nihw,njhw->ij", ap[:, :, u:u + H, v:v + W], x2) for u in range(T) for v in range(T)])
    p = J - J.min().detach() + 1e-16
    p = p / p.sum(dim=(1, 2), keepdim=True)
    p = (0.5 * (p + p.transpose(1, 2))).mean(0)
    ce = -torch.log(torch.diagonal(p) + 1e-16).sum() / (k * k)
    pm = x1.mean(1).reshape(-1)
    return ce + lamda * (math.log(pm.numel()) + (pm * pm.log()).sum())


def pui64(x, y, lamda):
    K = x.shape[1]
    xn = x / x.norm(dim=0, keepdim=True).clamp_min(1e-12)
    yn = y / y.norm(dim=0, keepdim=True).clamp_min(1e-12)
    pui = xn.t() @ yn
    ce = (torch.logsumexp(pui, 1) - torch.diagonal(pui)).mean()
    p = x.mean(0)
    return ce + lamda * (math.log(K) + (p * p.log()).sum())


def jsd64(xs, reduction, eps):
    def ent(t):
        return -(t * (t + eps).log()).sum(1)
    v = ent(sum(xs) / len(xs)) - sum(ent(t) for t in xs) / len(xs)
    return v.mean() if reduction == "mean" else v.sum() if reduction == "sum" else v


def prior64(x, prior, eps):
    C = x.shape[1]
    prior = torch.full((1, C), 1.0 / C, dtype=x.dtype) if prior is None else prior
    kl = (-x * torch.log((prior + eps) / (x + eps))).sum(1).mean()
    return math.log(float(C)) - kl


def reference(fn, ps):
    """fn on f64 leaves of ps -> (value, gradients); an unreduced value is differentiated under fx.none_weights"""
    xs = [p.double().clone().requires_grad_(True) for p in ps]
    v = fn(xs)
    (v if v.dim() == 0 else (v * fx.none_weights(v)).sum()).backward()
    return v.detach(), [x.grad for x in xs]


def check_value(got, want, tol, what=""):
    e = fx.rel_vec(torch.as_tensor(got).detach().cpu(), want)
    print(f"{what}: value {e:.2e} (tol {tol['scalar']:.2e})")
    assert e <= tol["scalar"], (what, e, tol["scalar"])


def check_grad(got, want, tol, what=""):
    """every element: relative 2-norm and max-norm"""
    got = got.detach().cpu()
    want = torch.as_tensor(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    e2, em = fx.rel_grad(got, want)
    print(f"{what}: 2-norm {e2:.2e} (tol {tol['grad2']:.2e}), max-norm {em:.2e} (tol {tol['gradmax']:.2e})")
    assert e2 <= tol["grad2"] and em <= tol["gradmax"], (what, e2, em, tol)
