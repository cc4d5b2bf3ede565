"""The cases of tests/test_gpu_imsat.py beyond the fixture, their float64 references on the CPU, and the comparisons.
tests/test_imsat_coverage.py (no GPU) holds these lists to what they claim: every form of the launch rule
(cy_imsat_plan) is taken by some case and every capped grid-stride loop is entered a second time.

References are the formulas of the issue in float64 torch with autograd, on the same f32 inputs cast up; each is
computed once per (case, upstream) and shared.
"""
import functools

import torch

import imsat_fixture as fx

# upstream gradients of (marg, cond); of (marg1, cond1, marg2, cond2, mse): five values, one of them zero
UPSTREAMS = ((1.0, 1.0), (-2.5, 0.0), (0.0, 3.0))
PAIR_UPSTREAMS = ((1.0, -0.5, 0.75, 2.0, 0.0), (0.0, 1.0, -1.0, 0.5, 3.0))

# inputs taken as slices that start this many floats into a larger (512-byte aligned) buffer -> the bytes the slice's
# base is aligned to
OFFSET_ALIGN = {0: 16, 1: 4, 2: 8, 3: 4}
ALIGN_SHAPES = ((3, 1037), (20, 130), (64, 33))  # (K, R), run at every offset of OFFSET_ALIGN
# the two halves of one [2R][K] tensor with R and K odd: the second half starts R*K floats in (4-byte aligned)
HALVES = ((5, 51), (63, 17))  # (K, R)

LOGIT_K = (2, 4, 5, 8, 16)
LOGIT_NPIX = (1, 257, 3 * 361)
LOGIT_COMPOSED_K = (17, 20)  # past the fused kernels: row softmax + probability rows


def cap_cases(plan):
    """[(form, K, R, align)]: row counts read from the launch rule `plan(form, R, K, align)` (ops.imsat_plan).
    K = 2: one row more than a full trip of the capped forward grid of the 16-byte form; the others: one row more than
    a full trip of the capped backward grid (the larger cap), so every loop of every kernel form runs a second trip."""
    big = 1 << 28

    def rows_of_trip(form, K, align, which):
        p = plan(form, big, K, align)
        per_tile = p["tile"] // K if form != "logits" else p["tile"]
        return p[which] * per_tile

    cases = [("rows", 2, rows_of_trip("rows", 2, 16, "fwd_grid") + 1, 16)]
    for form in ("rows", "pair"):
        cases.append((form, 64, rows_of_trip(form, 64, 16, "bwd_grid") + 1, 16))
        cases.append((form, 2, rows_of_trip(form, 2, 4, "bwd_grid") + 1, 4))
    for K, align in ((2, 16), (4, 16), (8, 16), (5, 16), (8, 4)):
        cases.append(("logits", K, rows_of_trip("logits", K, align, "bwd_grid") + 1, align))
    return cases


def seeded_logits(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 2.5 * 8).round().clamp(-48, 48) / 8


@functools.lru_cache(maxsize=None)
def seeded_rows(K, R, seed):
    """f32 probability rows [R, K] (CPU)"""
    return torch.softmax(seeded_logits((R, K), seed), 1)


def ref_rows(p, g):
    """p: f32 rows or map (CPU) -> (marg64, cond64, gradient of g[0]*marg + g[1]*cond in p's shape, f64)"""
    x = p.double().clone().requires_grad_(True)
    marg, cond = fx.entropies64(x)
    (g[0] * marg + g[1] * cond).backward()
    return marg.detach(), cond.detach(), x.grad


def ref_pair(p1, p2, g):
    a, b = (t.double().clone().requires_grad_(True) for t in (p1, p2))
    m1, c1 = fx.entropies64(a)
    m2, c2 = fx.entropies64(b)
    mse = ((a - b) ** 2).mean()
    out = torch.stack([m1, c1, m2, c2, mse])
    (out * torch.tensor(g, dtype=torch.float64)).sum().backward()
    return out.detach(), a.grad, b.grad


def ref_logits(z, g):
    x = z.double().clone().requires_grad_(True)
    marg, cond = fx.entropies64(torch.softmax(x, 1))
    (g[0] * marg + g[1] * cond).backward()
    return marg.detach(), cond.detach(), x.grad


def check_entropies(got, want, tol, what=""):
    """got, want: (marg, cond) (or more scalars) compared as one vector, relative 2-norm"""
    e = fx.rel_vec(torch.as_tensor([float(v) for v in got]), torch.as_tensor([float(v) for v in want]))
    print(f"{what}: scalars {e:.2e} (tol {tol['scalar']:.2e})")
    assert e <= tol["scalar"], (what, e, tol["scalar"])


def check_value(got, want, scale, tol, what=""):
    e = abs(float(got) - float(want)) / float(scale)
    print(f"{what}: value {e:.2e} of its scale (tol {tol['scalar']:.2e})")
    assert e <= tol["scalar"], (what, e, tol["scalar"])


def check_grad(got, want, tol, what=""):
    """every element: relative 2-norm and max-norm"""
    got = got.detach().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if float(torch.as_tensor(want).abs().max()) == 0.0:
        assert float(got.abs().max()) == 0.0, what
        return
    e2, em = fx.rel_grad(got, want)
    print(f"{what}: gradient 2-norm {e2:.2e} (tol {tol['grad2']:.2e}), max-norm {em:.2e} (tol {tol['gradmax']:.2e})")
    assert e2 <= tol["grad2"] and em <= tol["gradmax"], (what, e2, em, tol)
