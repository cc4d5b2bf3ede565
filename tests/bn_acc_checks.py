"""Checks on BatchNorm accumulators (csrc/cy_bn_acc.h) shared by tests/test_gpu_bn_acc.py and
tests/test_gpu_c2_geometry.py: one definition of each bound."""
import torch


def acc_sums(acc):
    """(sum, sum of squares) per channel as f64 from an accumulator [R][4][C]"""
    R, C = acc.R, acc.C
    w = acc.t[: R * 4 * C].view(R, 4, C).sum(0).double()
    assert int(acc.t[R * 4 * C:].sum()) == 0
    return w[0] / 4096.0 + w[1] / 2.0 ** 44, w[2] / 4096.0 + w[3] / 2.0 ** 44


def acc_encode(parts):
    """the inverse of acc_sums: float64 parts [R][2][C] (per replica: its share of the two sums) -> int64 words
    [R][4][C] as bn_acc_add splits them, hi = rint(s * 2^12), lo = rint((s - hi * 2^-12) * 2^44); no flag words"""
    parts = parts.double()
    hi = torch.round(parts * 4096.0)
    lo = torch.round((parts - hi / 4096.0) * 2.0 ** 44)
    R, _, C = parts.shape
    return torch.stack([hi[:, 0], lo[:, 0], hi[:, 1], lo[:, 1]], dim=1).to(torch.int64).reshape(R, 4, C)


def words_sums(words):
    """what a consumer reads from int64 words [R][4][C]: the replicas added as integers, then the two limbs joined"""
    w = words.sum(0).double()
    return w[0] / 4096.0 + w[1] / 2.0 ** 44, w[2] / 4096.0 + w[3] / 2.0 ** 44


def assert_acc_equals_partial_rows(acc, part, streaming: bool, what=""):
    """the partial rows are f32; their exact sum is what the accumulator holds (each split is exact above 2^-21) -- but
    for the streaming kernel, which sums its four wave rows in f32 before it adds (one add per workgroup).
    Returns the accumulator's (sum, sum of squares)."""
    s1, s2 = acc_sums(acc)
    p = part.double().sum(0)
    tol = 1e-6 if streaming else 1e-9
    assert torch.allclose(s1, p[0], rtol=0, atol=tol * max(1.0, p[0].abs().max().item())), (what, (s1 - p[0]).abs().max())
    assert torch.allclose(s2, p[1], rtol=tol, atol=1e-9), (what, (s2 - p[1]).abs().max())
    return s1, s2


def fold_tolerance(dtype) -> float:
    """a consumer that derives the BN+ReLU coefficients from the accumulator (fold=) against the same consumer fed
    scale / shift from the finalize launch: share of the output's max magnitude"""
    return 1e-5 if dtype == torch.float32 else 1.6e-2


def assert_fold_matches_scale_shift(out_fold, out_ref, dtype, what=""):
    a, b = out_fold.float(), out_ref.float()
    err, scale = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= fold_tolerance(dtype) * scale, f"{what}: fold= output off by {err:.3e} > {fold_tolerance(dtype):.1e} * {scale:.3e}"
