"""Every branch of the information-loss dispatch (csrc/cy_mi.hip) is reached by a parity case of
tests/test_gpu_mi_dispatch.py.  The launch plan is a pure host-side function of the shape (cy_joint_plan,
cy_group_softmax_plan), so the claim is checked here on the CPU, against the same case lists the GPU tests are
parametrised with (tests/mi_cases.py).  Every assertion names the branch it guards: dropping the case that reaches it
shows up here and not as silently lost coverage."""
import ctypes

import pytest
import torch

from tests import mi_cases as mc


def _plans(cases):
    return [(c, mc.plan(c)) for c in cases]


def _need(have, want, what):
    missing = sorted(set(want) - set(have), key=str)
    assert not missing, f"no case reaches {what}: {missing}"


def _some(plans, what, pred):
    hit = [c for c, p in plans if pred(c, p)]
    assert hit, f"no case reaches {what}"
    return hit


def test_tile_kernel_cases_at_pad_0():
    plans = [(c, p) for c, p in _plans(mc.JOINT_CASES) if c.pad == 0]
    assert all(p["fwd_kernel"] == 0 and p["grid_y"] == 1 for c, p in plans)
    _need({c.k for c, p in plans}, mc.K_EDGES, "the tile kernel at k")
    by_k = {c.k: p for c, p in plans if c.shape == mc.TWO_BLOCKS}
    assert by_k[1]["nsl"] == by_k[4]["nsl"] == 256 and by_k[64]["nsl"] == by_k[61]["nsl"] == 1
    assert by_k[12]["idle"] == 4 and by_k[20]["idle"] == 6 and by_k[33]["idle"] == 13 and by_k[64]["idle"] == 0
    assert [by_k[k]["kp"] for k in mc.K_EDGES] == [4, 4, 8, 12, 20, 36, 64, 64]
    _some(plans, "16-byte staging of the tile kernel below one tile", lambda c, p: p["fwd_vec"] and mc.npix(c.shape) < 64)
    _some(plans, "scalar staging of the tile kernel below one tile", lambda c, p: not p["fwd_vec"] and mc.npix(c.shape) < 64)
    for vec, k in ((1, 20), (0, 5)):  # two blocks, the second ends in a partial tile
        _some(plans, f"two blocks with a partial last tile, k = {k}",
              lambda c, p: c.k == k and p["fwd_vec"] == vec and p["nblk"] == 2 and p["per"] == 640
              and 0 < (mc.npix(c.shape) - p["per"]) % 64 < 64 and not c.masked)
    _some(plans, "joint_reduce_kernel past 64 partial blocks per slice", lambda c, p: p["reduce_trips"] >= 2)
    hit = _some(plans, "the forward's cap of 2048 partial blocks", lambda c, p: p["nblk"] == 2048)
    assert all(mc.npix(c.shape) > 2048 * 1024 and c.k == 4 for c in hit)
    _some(plans, "a masked map on the tile kernel", lambda c, p: c.masked)


def test_multi_kernel_cases():
    plans = [(c, p) for c, p in _plans(mc.JOINT_CASES) if p["fwd_kernel"] == 1]
    assert all(c.pad > 0 and p["fwd_lds"] <= 150 * 1024 for c, p in plans)
    vec = [(c, p) for c, p in plans if p["fwd_vec"]]
    _need({(c.pad, p["grid_y"], p["nd_last"]) for c, p in vec}, {(1, 1, 9), (2, 3, 7), (3, 6, 4)},
          "16-byte staging of the multi kernel at (pad, grid_y, nd of the last group)")
    _need({c.k for c, p in vec}, {8, 20}, "16-byte staging of the multi kernel at k")
    for v in (1, 0):
        _some(plans, f"a row-tile tail (R = 6, tiles_h = 2, 4 rows) with fwd_vec = {v}",
              lambda c, p: p["fwd_vec"] == v and p["R"] == 6 and p["tiles_h"] == 2 and c.shape[1] - p["R"] == 4)
    _some(plans, "W > 256 (R = 1)", lambda c, p: c.shape[2] > 256 and p["R"] == 1 and p["tiles_h"] == c.shape[1])
    _some(plans, "nsl > W (slices past the first row at entry)", lambda c, p: p["nsl"] == 256 and p["nsl"] > c.shape[2])
    _some(plans, "idle threads on the multi kernel", lambda c, p: p["idle"] > 0 and c.k == 12 and c.pad == 2)
    _some(plans, "a block that walks more than one tile", lambda c, p: p["ntile"] > p["nblk"])
    _some(plans, "a masked map on the multi kernel", lambda c, p: c.masked)


def test_fallback_cases():
    plans = [(c, p) for c, p in _plans(mc.JOINT_CASES) if p["fwd_kernel"] == 0 and c.pad > 0]
    assert all(not p["fwd_vec"] and p["grid_y"] == (2 * c.pad + 1) ** 2 for c, p in plans)
    _need({c.k for c, p in plans}, {61, 64}, "the per-displacement fallback (pad > 0) at k")
    _some(plans, "the fallback with grid_y = 25", lambda c, p: p["grid_y"] == 25)
    from cyhip import ops
    for c, p in plans:  # the tile these shapes would stage on the multi kernel does exceed 150 KB
        N, H, W = c.shape
        R = min(H, max(1, 256 // W))
        assert ((R + 2 * c.pad) * (W + 2 * c.pad) + R * W) * p["kp"] * 4 > 150 * 1024
    assert [ops.joint_plan(1, 8, 64, k, 1)["fwd_kernel"] for k in (56, 57)] == [1, 0]  # (kp = 56 still fits)


def test_backward_cases():
    plans = _plans(mc.BWD_CASES)
    _need({(p["bwd_kernel"], c.pad) for c, p in plans}, {(v, pad) for v in (0, 1) for pad in (0, 1, 2)},
          "(backward kernel: 1 = vec4, pad)")
    _some(plans, "vec4 backward with pad > 0", lambda c, p: p["bwd_kernel"] == 1 and c.pad > 0)
    hit = _some(plans, "k = 64 at pad 0", lambda c, p: c.k == 64 and c.pad == 0)
    # one displacement of the largest k is 16 KB, and the most the backward ever stages is the 64 KB of its budget
    assert all(mc.plan(c)["bwd_lds"] == 64 * 64 * 4 and mc.plan(c)["bwd_nchunk"] == 1 for c in hit)
    for k, pad, chunks in ((64, 1, (4, 3)), (32, 2, (16, 2))):
        _some(plans, f"the chunked backward at k = {k}, pad = {pad}",
              lambda c, p: (c.k, c.pad) == (k, pad) and (p["bwd_dchunk"], p["bwd_nchunk"]) == chunks
              and p["bwd_lds"] == 64 * 1024)
    _need({p["bwd_kernel"] for c, p in plans if p["bwd_nchunk"] > 1}, {0, 1}, "more than one dJ chunk on backward kernel")
    assert all((2 * c.pad + 1) ** 2 % p["bwd_dchunk"] for c, p in plans if p["bwd_nchunk"] > 1), "a short last chunk"
    hit = _some(plans, "the backward's second trip past 8192 blocks", lambda c, p: p["bwd_trips"] >= 2)
    assert all(p["bwd_grid"] == 8192 for c, p in plans if c in hit)
    assert all(8192 * 256 < mc.npix(c.shape) * c.k // 4 <= 8192 * 256 * 1.05 for c in hit)  # the smallest, within 5 %
    _need({c.need for c, p in plans}, {"1", "2", "12"}, "need")
    _need({(c.normalise, c.pad > 0) for c, p in plans}, {(a, b) for a in (True, False) for b in (True, False)},
          "(normalise, pad > 0)")
    _some(plans, "gscale != 1", lambda c, p: c.gscale != 1.0)
    _some(plans, "gscale < 0", lambda c, p: c.gscale < 0)


def test_the_production_launch_is_unchanged():
    """pad 0, k = 20 at the configured size: the vec4 kernel, the capped grid, dJ staged once in 1600 bytes"""
    from cyhip import ops
    p = ops.joint_plan(16, 224, 224, 20, 0)
    assert (p["bwd_kernel"], p["bwd_grid"], p["bwd_lds"], p["bwd_dchunk"], p["bwd_nchunk"]) == (1, 8192, 1600, 1, 1)
    assert p["bwd_trips"] == -(-16 * 224 * 224 * 5 // (8192 * 256))
    assert (p["fwd_kernel"], p["fwd_vec"], p["nblk"], p["fwd_lds"], p["nsl"]) == (0, 1, 784, (2 * 64 * 20 + 10 * 400) * 4, 10)
    q = ops.joint_plan(16, 224, 224, 20, 1)
    assert (q["fwd_kernel"], q["fwd_vec"], q["R"], q["grid_y"], q["nd_last"]) == (1, 1, 1, 1, 9)
    assert q["fwd_lds"] == (3 * 226 + 224) * 20 * 4 and q["bwd_nchunk"] == 1 and q["bwd_lds"] == 9 * 1600


def test_forward_and_backward_accept_the_same_shapes():
    from cyhip import _lib, ops
    lib = _lib.load()
    for k in range(1, 65):
        for pad in range(0, 5):
            p = ops.joint_plan(1, 8, 64, k, pad)
            TT = (2 * pad + 1) ** 2
            assert p["bwd_lds"] == p["bwd_dchunk"] * k * k * 4 <= 64 * 1024, (k, pad, p)
            assert (p["bwd_nchunk"] - 1) * p["bwd_dchunk"] < TT <= p["bwd_nchunk"] * p["bwd_dchunk"], (k, pad, p)
            assert p["bwd_nchunk"] == 1 or (p["bwd_dchunk"] + 1) * k * k * 4 > 64 * 1024, (k, pad, p)
            assert p["ws_bytes"] == TT * p["nblk"] * k * k * 4
    # refused: by the plan, and by both launches before anything is launched
    plan = _lib.JointPlan()
    one = ctypes.c_void_p(8)  # (never dereferenced: these shapes return before any launch)
    for N, H, W, k, pad in ((1, 8, 64, 65, 0), (1, 8, 64, 0, 0), (1, 8, 64, 20, -1), (1, 8, 64, 20, 8), (2, 3, 260, 4, 3)):
        assert lib.cy_joint_plan(N, H, W, k, pad, plan) == -2, (N, H, W, k, pad)
        assert lib.cy_joint_fwd(one, one, one, N, H, W, k, pad, 0, one, 1 << 40, None) == -2
        assert lib.cy_joint_bwd(one, one, one, one, one, one, N, H, W, k, pad, 0, None) == -2
        assert lib.cy_joint_ws_bytes(N, H, W, k, pad) == 0
    assert lib.cy_joint_plan(0, 8, 64, 20, 0, plan) == -1 and lib.cy_joint_plan(1, 8, 64, 20, 0, None) == -1
    with pytest.raises(_lib.HipKernelError):
        ops.joint_plan(1, 8, 64, 65, 0)


@pytest.mark.parametrize("case", mc.JOINT_CASES + mc.BWD_CASES, ids=mc.case_id)
def test_joint_plan_from_first_principles(case):
    N, H, W = case.shape
    k, pad, n = case.k, case.pad, mc.npix(case.shape)
    p = mc.plan(case)
    TT = (2 * pad + 1) ** 2
    kp = -(-k // 4) * 4
    tps = (kp // 4) ** 2
    assert (p["kp"], p["nsl"], p["idle"]) == (kp, 256 // tps, 256 - 256 // tps * tps)
    assert p["nblk"] == min(2048, -(-n // 1024)) and p["reduce_trips"] == -(-p["nblk"] // 64)
    red = p["nsl"] * kp * kp * 4
    if p["fwd_kernel"] == 1:
        R = min(H, max(1, 256 // W))
        assert (p["R"], p["tiles_h"], p["ntile"], p["per"]) == (R, -(-H // R), N * -(-H // R), 0)
        assert p["fwd_lds"] == max(red, ((R + 2 * pad) * (W + 2 * pad) + R * W) * kp * 4)
        assert p["grid_y"] == -(-TT // 9) and p["nd_last"] == TT - 9 * (p["grid_y"] - 1) and p["fwd_vec"] == (kp == k)
    else:
        assert (p["R"], p["tiles_h"], p["grid_y"], p["nd_last"]) == (0, 0, TT, 1)
        assert p["per"] % 64 == 0 and p["per"] * p["nblk"] >= n > (p["per"] - 64) * p["nblk"] - 64 * p["nblk"]
        assert p["ntile"] == -(-n // 64) and p["fwd_lds"] == 2 * 64 * kp * 4 + red
        assert p["fwd_vec"] == (pad == 0 and kp == k)
    work = n * (k // 4 if k % 4 == 0 else k)
    assert p["bwd_kernel"] == (k % 4 == 0) and p["bwd_grid"] == min(8192, -(-work // 256))
    assert (p["bwd_trips"] - 1) * p["bwd_grid"] * 256 < work <= p["bwd_trips"] * p["bwd_grid"] * 256
    q = mc.sentinel_pixels(case.shape, p)
    assert q[0] == 0 and q[-1] == n - 1


def test_loss_cases():
    cs = mc.LOSS_CASES
    _need({(c.mode, c.symmetric) for c in cs}, {(m, s) for m in (0, 1, 2) for s in (False, True)}, "(mode, symmetric)")
    _need({(c.TT, c.k) for c in cs}, {(1, 1), (1, 20), (9, 20), (25, 12), (9, 64), (25, 64)}, "the loss kernel at (TT, k)")
    assert all((c.mode == 1) == (c.TT > 1) for c in cs)
    _need({(c.kind, c.mode) for c in cs}, {("zeros", 0), ("zeros", 1), ("zeros", 2), ("min_later", 1)}, "(kind, mode)")
    assert set(mc.LAMDAS) == {1.0, 1.5}
    _need({(c.mode, c.pad > 0, c.symmetric) for c in mc.IID_CASES}, {(0, False, False), (2, False, True), (1, True, True),
                                                                    (1, True, False)}, "IIDFn at (mode, pad > 0, symmetric)")
    iid = [(c, mc.plan(c)) for c in mc.IID_CASES]
    _need({(p["fwd_kernel"], c.pad > 0) for c, p in iid}, {(0, False), (1, True), (0, True)},
          "IIDFn on (forward kernel, pad > 0)")
    _some(iid, "IIDFn through the chunked backward", lambda c, p: p["bwd_nchunk"] > 1)


def test_softmax_cases_and_bounds():
    from cyhip import _lib, ops
    cs = mc.SOFTMAX_CASES
    _need({c.M for c in cs}, mc.M_ALL, "grouped softmax at M")
    _need({(c.S, c.k) for c in cs}, mc.SK_ALL, "grouped softmax at (S, k)")
    _need({(c.S, c.k, c.T) for c in cs}, {(S, k, T) for S, k in mc.SK_ALL for T in (1.0, 0.1)}, "(S, k, T)")
    plans = [(c, mc.softmax_plan(c)) for c in cs]
    for rows in (64, 32):  # one block, a short block, exact blocks, a block of one row, many blocks
        ms = {c.M for c, p in plans if p["bwd_rows"] == rows}
        assert ms >= set(mc.M_ALL), (rows, ms)
    for c, p in plans:
        sk = c.S * c.k
        assert p["fwd_ok"] == p["bwd_ok"] == 1 and p["fwd_rows"] == 64 and p["bwd_rows"] == (64 if sk <= 127 else 32)
        assert p["fwd_lds"] == 64 * (sk + 1) * 4 <= 65536 and p["bwd_lds"] == 2 * p["bwd_rows"] * (sk + 1) * 4 <= 65536
        assert p["fwd_grid"] == -(-c.M // 64) and p["bwd_grid"] == -(-c.M // p["bwd_rows"])
    # the edges: 127 | 128 is where the backward halves its rows, 255 | 256 where both directions refuse
    assert ops.group_softmax_plan(65, 1, 127)["bwd_rows"] == 64 and ops.group_softmax_plan(65, 1, 128)["bwd_rows"] == 32
    assert ops.group_softmax_plan(65, 1, 255)["bwd_lds"] == 65536
    assert {(1, 127), (1, 128), (1, 255)} <= {(c.S, c.k) for c in cs}
    lib, plan, one = _lib.load(), _lib.GroupSoftmaxPlan(), ctypes.c_void_p(8)
    for S, k in mc.SOFTMAX_REFUSED:
        assert S * k > 255
        assert lib.cy_group_softmax_plan(65, S, k, plan) == -2
        assert lib.cy_group_softmax_fwd(one, one, 65, S, k, 1.0, None) == -2  # (before any launch: `one` is never read)
        assert lib.cy_group_softmax_bwd(one, one, one, 65, S, k, 1.0, None) == -2
        with pytest.raises(_lib.HipKernelError):
            ops.group_softmax_plan(65, S, k)
    assert lib.cy_group_softmax_plan(0, 1, 4, plan) == -1 and lib.cy_group_softmax_plan(65, 1, 4, None) == -1
    assert ops.group_softmax_plan(65, 10, 20)["bwd_ok"] == 1  # ten sub-heads of twenty clusters: forward and backward


@pytest.mark.parametrize("pad,mode,symmetric", [(0, 0, False), (0, 0, True), (1, 1, False), (2, 1, True)])
def test_reference_of_the_layers_composes_to_the_oracle(pad, mode, symmetric):
    """raw_joint + loss_from_joint (the float64 references of layers 1 and 2 of the GPU tests) give the loss of
    oracle/next_rows.py, which tests/test_oracle_golden.py pins to the reference's own output"""
    from oracle import next_rows as onr
    gen = torch.Generator().manual_seed(7 + pad)
    a = torch.softmax(torch.randn(2, 5, 6, 7, generator=gen, dtype=torch.float64), 1)
    b = torch.softmax(torch.randn(2, 5, 6, 7, generator=gen, dtype=torch.float64), 1)
    want = onr.iid_segmentation_loss(a, b, lamda=1.5, padding=pad, symmetric=symmetric)
    J = mc.raw_joint(a.permute(0, 2, 3, 1), b.permute(0, 2, 3, 1), pad)
    got, P = mc.loss_from_joint(J / (2 * 6 * 7) if mode == 0 else J, mode, symmetric, 1.5, 1e-5)
    assert abs(got.item() - want.item()) <= 1e-12 * max(1.0, abs(want.item()))
    assert torch.allclose(P.reshape(-1), onr.joint_maps(a, b, pad, symmetric).reshape(-1), rtol=0, atol=1e-14)
    # the displacement convention of raw_joint, entry by entry
    for d in range((2 * pad + 1) ** 2):
        du, dv = mc.disp(d, pad)
        x1 = torch.zeros_like(a.permute(0, 2, 3, 1))
        src = a.permute(0, 2, 3, 1)
        H, W = 6, 7
        moved = src[:, max(0, du):H - max(0, -du), max(0, dv):W - max(0, -dv)]
        x1[:, max(0, -du):H - max(0, du), max(0, -dv):W - max(0, dv)] = moved
        want_d = torch.einsum("nhwi,nhwj->ij", x1, b.permute(0, 2, 3, 1))
        assert torch.allclose(J[d], want_d, rtol=0, atol=1e-12), d


def test_reference_of_the_vector_loss_is_the_oracle():
    from oracle import next_rows as onr
    gen = torch.Generator().manual_seed(3)
    a = torch.softmax(torch.randn(37, 5, generator=gen, dtype=torch.float64), 1)
    b = torch.softmax(torch.randn(37, 5, generator=gen, dtype=torch.float64), 1)
    l, l0, pij = onr.iid_loss(a, b, lamb=1.5)
    J = mc.raw_joint(a.view(37, 1, 1, 5), b.view(37, 1, 1, 5), 0)
    got, P = mc.loss_from_joint(J, 2, True, 1.5, 1e-10)
    got0, _ = mc.loss_from_joint(J, 2, True, 1.0, 1e-10)
    assert abs(got.item() - l.item()) <= 1e-12 and abs(got0.item() - l0.item()) <= 1e-12
    assert torch.allclose(P.view(5, 5), pij, rtol=0, atol=1e-15)
