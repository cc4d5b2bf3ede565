"""tests/test_gpu_imsat.py claims to take every form of the IMSAT launch rule (16- and 4-byte sweeps of the row and
pair kernels; the compiled and the run-time class counts of the logit kernels, aligned and not) and to enter every
capped grid-stride loop a second time.  The claims are conditions on the case tables (tests/imsat_cases.py,
tests/imsat_fixture.py) and on the host-side launch rule (cy_imsat_plan), so they are checked here without a GPU.
Each assertion names its condition: deleting a case fails here, by name."""
import re
from pathlib import Path

import pytest

import imsat_cases as ic
import imsat_fixture as fx

REPO = Path(__file__).resolve().parents[1]
SOURCE = REPO / "contrast-you_amd" / "csrc" / "cy_imsat.hip"


@pytest.fixture(scope="module")
def plan():
    from cyhip import ops
    return ops.imsat_plan


def test_caps_and_depth_match_the_source(plan):
    text = SOURCE.read_text()
    caps = dict(re.findall(r"constexpr int IMSAT_(FWD_CAP|BWD_CAP|DEPTH) = (\d+);", text))
    assert caps == {"FWD_CAP": "1024", "BWD_CAP": "2048", "DEPTH": "4"}
    p = plan("rows", 1 << 28, 64, 16)
    assert (p["fwd_grid"], p["bwd_grid"]) == (1024, 2048) and p["tile"] == p["threads"] * p["vec"] * 4
    # the kernels: two sweeps (forward, backward) in four instances each, two pixel kernels in four, one finalize
    assert len(re.findall(r"__global__", text)) == 5
    assert "atomicAdd" not in text and "__hip_atomic" not in text


def test_a_thread_keeps_its_columns_for_every_k(plan):
    """the rule the sweep rests on: the stride between a thread's chunks is a multiple of K, for every K and form"""
    for K in range(2, 65):
        for align in (4, 8, 16):
            for form in ("rows", "pair"):
                p = plan(form, 1000, K, align)
                assert p["vec"] == (4 if align == 16 else 1), (K, align)
                assert (p["threads"] * p["vec"]) % K == 0 and p["tile"] % K == 0, (K, align)
                assert 256 - K < p["threads"] <= 256, (K, align, p["threads"])
                assert p["slots"] == (1 + K if form == "rows" else 3 + 2 * K)
    assert min(plan("rows", 1000, K, 4)["threads"] for K in range(2, 65)) == 208  # K = 52: the fewest working threads


def test_both_sweep_forms_are_taken_by_rows_and_pairs(plan):
    forms = {(form, plan(form, R, K, align)["vec"])
             for K, R in ic.ALIGN_SHAPES for align in ic.OFFSET_ALIGN.values() for form in ("rows", "pair")}
    assert forms == {("rows", 1), ("rows", 4), ("pair", 1), ("pair", 4)}
    assert set(ic.OFFSET_ALIGN) == {0, 1, 2, 3} and set(ic.OFFSET_ALIGN.values()) == {4, 8, 16}
    for K, R in ic.ALIGN_SHAPES:
        p4, p1 = plan("rows", R, K, 16), plan("rows", R, K, 4)
        # more than one block, and a last chunk that is not full in either form (the element-wise tail)
        assert p1["fwd_grid"] > 1 and (R * K) % p1["tile"] and (R * K) % p4["tile"], (K, R)
    assert any((R * K) % 4 for K, R in ic.ALIGN_SHAPES), "a buffer whose last 16-byte chunk is cut"
    for K, R in ic.HALVES:
        assert K % 2 and R % 2 and (R * K * 4) % 8 == 4, "the second half is only 4-byte aligned"
    assert {K for K, _ in fx.ROW_SHAPES} == {2, 3, 5, 20, 40, 63, 64}
    assert {R for _, R in fx.ROW_SHAPES} == {1, 255, 257, 3 * 19 * 19}
    assert all(v[0] * v[2] * v[3] == 3 * 19 * 19 for v in fx.MAP_CASES.values()) and len(fx.MAP_CASES) == 2
    one_hot = fx.onehot_rows()
    assert ((one_hot == 0) | (one_hot == 1)).all() and (one_hot.sum(1) == 1).all() and (one_hot.sum(0) == 0).any()


def test_every_logit_form_is_taken(plan):
    assert ic.LOGIT_K == (2, 4, 5, 8, 16) and ic.LOGIT_NPIX == (1, 257, 3 * 361) and ic.LOGIT_COMPOSED_K == (17, 20)
    assert {plan("logits", 257, K, 16)["kt"] for K in ic.LOGIT_K} == {0, 2, 4, 8}
    assert plan("logits", 257, 5, 16)["kt"] == 0 == plan("logits", 257, 16, 16)["kt"]
    # rows that are not aligned for the compiled forms go one float at a time
    assert plan("logits", 257, 2, 4)["kt"] == 0 and plan("logits", 257, 8, 8)["kt"] == 0
    assert plan("logits", 257, 2, 8)["kt"] == 2
    assert max(ic.LOGIT_NPIX) > 2 * 256 and 257 % 256 == 1, "more than one block, and a block with one pixel"
    from cyhip import ops
    assert ops.IMSAT_LOGITS_KMAX == 16 and min(ic.LOGIT_COMPOSED_K) == 17


def test_every_capped_loop_runs_a_second_trip(plan):
    cases = ic.cap_cases(plan)
    seen = set()
    for form, K, R, align in cases:
        p = plan(form, R, K, align)
        seen.add((form, p["vec"], p["kt"], p["fwd_trips"] >= 2, p["bwd_trips"] >= 2))
    for form in ("rows", "pair"):
        for vec in (1, 4):
            assert (form, vec, 0, True, True) in seen, (form, vec)
    for kt, vec in ((2, 2), (4, 4), (8, 4), (0, 1)):
        assert ("logits", vec, kt, True, True) in seen, kt
    # K = 2 one row past a full trip of the capped forward grid, K = 64 with two (or more) trips
    form, K, R, align = cases[0]
    p = plan(form, R, K, align)
    assert (form, K, p["fwd_grid"], p["fwd_trips"]) == ("rows", 2, 1024, 2)
    assert (R - 1) * K == 1024 * p["tile"], "one row more than a full trip"
    assert any(K == 64 and plan(f, R, K, a)["bwd_trips"] == 2 for f, K, R, a in cases)
    assert max(R * K for _, K, R, _ in cases) <= 1 << 24, "no case above 64 MB of input"
    assert len(ic.PAIR_UPSTREAMS[0]) == 5 and all(g.count(0.0) == 1 for g in ic.PAIR_UPSTREAMS)
    assert ic.UPSTREAMS == ((1.0, 1.0), (-2.5, 0.0), (0.0, 3.0))
