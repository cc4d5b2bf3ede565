"""What tests/test_gpu_selfpaced.py relies on, checked without a GPU: the entry points of the fused self-paced loss are
declared, exported and typed; every rejection returns its exact code (a refused call launches nothing, so host buffers
do); the case tables of tests/selfpaced_cases.py meet the geometry they name (the column-split count read from the
library's workspace query); every hard case leaves its margin and every soft case both branches of the clamp; the
oracle is pinned to the reference's float64 record; `global_negatives` reaches the epoch hook; `defer_checks` defaults
to the reference's behaviour."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import selfpaced_cases as sc

REPO = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from cyhip import _lib
    return _lib.load()


def splits(lib, R, D=8):
    """ns from cy_supcon_fused_ws_bytes: (R + 4 + ns * R * max(3, D)) floats"""
    return (lib.cy_supcon_fused_ws_bytes(R // 2, D) // 4 - R - 4) // (R * max(3, D))


# ---------------------------------------------------------------- symbols
def test_entry_points_are_declared_exported_and_typed(lib):
    from cyhip import _lib
    header = (REPO / "include" / "contrastyou_hip.h").read_text()
    ptr, i, f = C.c_void_p, C.c_int, C.c_float
    want = {
        "cy_supcon_sp_ws_bytes": (C.c_size_t, [i, i]),
        "cy_supcon_sp_fwd": (i, [ptr] * 7 + [C.c_size_t, i, i, f, f, i, i, ptr]),
        "cy_supcon_sp_bwd": (i, [ptr] * 8 + [C.c_size_t, i, i, f, f, i, ptr]),
    }
    for name, (res, args) in want.items():
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name}: declared in the header"
        assert name in _lib.exported_names()
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, f"{name}: {fn.restype}, {fn.argtypes}"
    assert lib.cy_abi_version() == _lib.ABI_VERSION == 19, "no signature of these entries changed"
    from cyhip import functions, ops
    assert callable(ops.supcon_sp_fwd) and callable(ops.supcon_sp_bwd)
    assert issubclass(functions.SelfPacedSupConFn, torch.autograd.Function)


# ---------------------------------------------------------------- rejections
def sp_status(lib, entry, p, *, n=4, D=8, t=sc.T, gamma=2.0, null="", ws_short=0):
    P = None if null == "P" else p
    lab = None if null == "labels+mask" else p
    out = None if null == "out" else p
    stats = None if null == "stats" else p
    ws = None if null == "ws" else p
    nbytes = lib.cy_supcon_sp_ws_bytes(max(n, 1), max(D, 1)) - ws_short
    if entry == "cy_supcon_sp_fwd":
        return lib.cy_supcon_sp_fwd(P, lab, None, out, stats, None, ws, nbytes, n, D, t, gamma, 1, 0, None)
    assert entry == "cy_supcon_sp_bwd"
    return lib.cy_supcon_sp_bwd(P, lab, None, stats, p, p, out, ws, nbytes, n, D, t, gamma, 1, None)


def test_rejections_return_the_exact_code(lib):
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    whats = [r[0] for r in sc.SP_REJECTS]
    for needed in ("P null", "neither labels nor mask", "an output null", "row_stats null", "workspace null", "n = 0", "n < 0",
                   "D = 0", "D < 0", "D = 264", "D = 12", "t = 0", "t < 0", "gamma = 0", "gamma < 0",
                   "workspace one byte short"):
        assert needed in whats, needed
    for what, over, want in sc.SP_REJECTS:
        for entry in sc.SP_ENTRIES:
            assert sp_status(lib, entry, p, **over) == want, f"{entry}: {what}"
    # the backward's further inputs
    nbytes = lib.cy_supcon_sp_ws_bytes(4, 8)
    assert lib.cy_supcon_sp_bwd(p, p, None, p, None, p, p, p, nbytes, 4, 8, sc.T, 2.0, 0, None) == sc.ERR_ARG, "aux null"
    assert lib.cy_supcon_sp_bwd(p, p, None, p, p, None, p, p, nbytes, 4, 8, sc.T, 2.0, 0, None) == sc.ERR_ARG, "gscale null"
    # a mask alone is accepted as far as the next check, in both modes
    for soft in (0, 1):
        assert lib.cy_supcon_sp_fwd(p, None, p, p, p, None, p, 0, 4, 8, sc.T, 2.0, soft, 1, None) == sc.ERR_WORKSPACE
        assert lib.cy_supcon_sp_bwd(p, None, p, p, p, p, p, p, 0, 4, 8, sc.T, 2.0, soft, None) == sc.ERR_WORKSPACE


def test_workspace_query(lib):
    assert lib.cy_supcon_sp_ws_bytes(0, 8) == 0 and lib.cy_supcon_sp_ws_bytes(4, 0) == 0 and lib.cy_supcon_sp_ws_bytes(-1, 8) == 0
    # diag[R] + M[4] + max(forward partials [ns][R][3 + 2], backward partials [ns][R][D]) floats
    for n, D in ((1, 16), (33, 8), (520, 8), (35, 256), (sc.NOMAT_N, sc.NOMAT_D)):
        R = 2 * n
        ns = splits(lib, R, D)
        assert lib.cy_supcon_sp_ws_bytes(n, D) == 4 * (R + 4 + ns * R * max(5, D)), (n, D)
    # C5: 4 splits x 4096 rows x 256 floats = 16 MiB of backward partials
    assert splits(lib, 4096, 256) == 4
    assert lib.cy_supcon_sp_ws_bytes(sc.NOMAT_N, sc.NOMAT_D) - 4 * (4096 + 4) == 16 << 20
    # the query of the plain fused loss has not moved
    assert lib.cy_supcon_fused_ws_bytes(33, 8) == 4 * (66 + 4 + 2 * 66 * 8)


# ---------------------------------------------------------------- tables
def test_case_tables_meet_their_geometry(lib):
    assert (sc.ONE_PAIR.n, sc.ONE_PAIR.D, sc.ONE_PAIR.positives, sc.ONE_PAIR.rows) == (1, 16, "simclr", "twin")
    got = {name: (2 * n, D, sc.row_blocks(2 * n), splits(lib, 2 * n, D)) for name, n, D, _, _ in sc.SIZES}
    assert got["one-full-tile"] == (64, 8, 1, 1), "R = 64: one row block, one split"
    assert got["two-row-second-tile"] == (66, 8, 2, 2), "R = 66: two row blocks, two splits"
    assert got["uneven-splits"] == (1040, 8, 17, 15), "R = 1040: 17 row blocks, 15 splits"
    assert sorted(set(sc.split_blocks(1040, 15))) == [1, 2], "splits of one and of two column blocks"
    for name, n, D, rb, ns in sc.SIZES:
        assert got[name][2:] == (rb, ns), f"{name}: the table's own counts"
        assert any(p.name == f"{name}/camp" for p in sc.SIZE_PROBLEMS), f"{name}: the two-camp input at every size"
        assert any(p.name == f"{name}/rand" for p in sc.SIZE_PROBLEMS) == (n <= sc.RAND_MAX_N), f"{name}: random rows"
    assert (sc.BIG.n, sc.BIG.D) == (520, 8) and sc.BIG in sc.SIZE_PROBLEMS
    assert sc.WIDTH_N == 35 and sc.row_blocks(70) == 2 and splits(lib, 70) == 2
    assert sc.WIDTHS == (8, 40, 248, 256) and [-(-D // 32) for D in sc.WIDTHS] == [1, 2, 8, 8] and 248 % 32 and not 256 % 32
    from cyhip import ops
    from types import SimpleNamespace
    assert all(ops.supcon_fused_ok(SimpleNamespace(shape=(70, D))) for D in sc.WIDTHS)
    assert sc.FALLBACK_WIDTHS == (264, 17) and not any(ops.supcon_fused_ok(SimpleNamespace(shape=(70, D))) for D in sc.FALLBACK_WIDTHS)
    m = sc.kind_d_mask(sc.MASK_PROBLEM.n, sc.MASK_SEED)
    assert (sc.MASK_PROBLEM.n, sc.MASK_SEED) == (35, 61) and set(m.unique().tolist()) == {0, 1, -1, 2}
    assert not torch.equal(m == 1, (m == 1).t()) and not torch.equal(m == 0, (m == 0).t()) and bool((m.diagonal() == 1).all())
    assert sc.GSCALE == 0.7 and sc.T == 0.07
    assert (sc.TOL_LOSS, sc.TOL_GRAD, sc.TOL_PATHS, sc.ONE_PAIR_ABS) == (1e-5, 1e-4, 1e-5, 1e-15)
    assert len({p.name for p in sc.ALL_PROBLEMS}) == len(sc.ALL_PROBLEMS)
    # fused against composition: the mask instantiations, and labels over two and over fifteen splits
    assert all(p in sc.ALL_PROBLEMS for p in sc.PATH_PROBLEMS), "their margins are asserted below"
    assert {p.positives for p in sc.PATH_PROBLEMS} == {"maskd", "mod3"}
    assert {splits(lib, 2 * p.n, p.D) for p in sc.PATH_PROBLEMS if p.positives == "mod3"} == {2, 15}


def test_golden_file_is_what_the_table_says(golden_dir):
    g = np.load(golden_dir / sc.GOLDEN_FILE)
    src = np.load(golden_dir / sc.GOLDEN_INPUTS)
    assert src["z1"].shape == (sc.GOLDEN_N, sc.GOLDEN_D) == (70, 16)
    assert len(sc.GOLDEN_TAGS) == 12 and set(sc.RATIO_F32_F64) == set(sc.GOLDEN_TAGS)
    for name in ("b", "d"):
        m = torch.from_numpy(src[f"{name}_mask"])
        assert not torch.equal(m == 1, (m == 1).t()), f"mask {name}: asymmetric"
    assert set(np.unique(src["d_mask"]).tolist()) == {0, 1, -1, 2}, "mask d: pairs that are neither"
    for tag in sc.GOLDEN_TAGS:
        assert g[f"{tag}_dz1"].shape == g[f"{tag}_dz2"].shape == (70, 16) and np.isfinite(g[f"{tag}_loss"])
        dist = abs(float(g[f"{tag}_ratio32"]) - float(g[f"{tag}_ratio"]))
        assert abs(dist - sc.RATIO_F32_F64[tag]) <= 0.05 * dist + 1e-12, f"{tag}: the recorded f32-f64 distance {dist:.2e}"
        assert sc.ratio_tol(tag) == max(4 * sc.RATIO_F32_F64[tag], 1e-6)
    assert (golden_dir / sc.GOLDEN_FILE).stat().st_size < 300_000


# ---------------------------------------------------------------- margins
@pytest.mark.parametrize("p", sc.ALL_PROBLEMS, ids=lambda p: p.name)
def test_hard_margin_and_soft_branches(p):
    z1, z2, target, mask = sc.tensors(p)
    for z in (z1, z2):
        assert z.dtype == torch.float32 and float((z.double().norm(dim=1) - 1).abs().max()) < 1e-6
    l = sc.positive_losses(z1, z2, target, mask)
    g_hard, g_soft = sc.gamma_of(p, "hard", l), sc.gamma_of(p, "soft", l)
    margin = float((l - g_hard).abs().min())
    print(f"{p.name}: {l.numel()} positive pairs, gamma hard {g_hard:.6f} (margin {margin:.3e}, {float((l <= g_hard).float().mean()):.3f} "
          f"below), soft {g_soft:.6f}")
    assert g_hard > 0 and g_soft > 0
    assert margin >= sc.HARD_MARGIN, f"{p.name}: min |l_ij - gamma| = {margin:.3e} over every positive pair"
    if p.rows == "twin":
        assert float(l.abs().max()) <= 1e-15, "one pair: l_ij = 0, every weight 1"
    else:
        assert bool((l < g_soft).any()) and bool((l > g_soft).any()), f"{p.name}: both branches of the clamp"
        assert bool((l <= g_hard).any()) and bool((l > g_hard).any()), f"{p.name}: weights of both values"


def test_golden_margins(golden_dir):
    g, src = np.load(golden_dir / sc.GOLDEN_FILE), np.load(golden_dir / sc.GOLDEN_INPUTS)
    z1, z2 = torch.from_numpy(src["z1"]), torch.from_numpy(src["z2"])
    for positives in sc.GOLDEN_POSITIVES:
        target = [i % 3 for i in range(sc.GOLDEN_N)] if positives == "mod3" else None
        mask = None if positives == "mod3" else torch.from_numpy(src[f"{positives}_mask"])
        l = sc.positive_losses(z1, z2, target, mask)
        gh, gs = float(g[f"{positives}_hard_c0_gamma"]), float(g[f"{positives}_soft_c0_gamma"])
        assert gh == float(g[f"{positives}_hard_c1_gamma"]) and gs == float(g[f"{positives}_soft_c1_gamma"])
        assert float((l - gh).abs().min()) >= sc.HARD_MARGIN, positives
        assert bool((l < gs).any()) and bool((l > gs).any()), positives


# ---------------------------------------------------------------- the oracle against the reference's record
def test_oracle_is_pinned_to_the_golden(golden_dir):
    from oracle import next_rows as onr
    g, src = np.load(golden_dir / sc.GOLDEN_FILE), np.load(golden_dir / sc.GOLDEN_INPUTS)
    for tag in sc.GOLDEN_TAGS:
        positives, mode, cg = tag.split("_")
        target = [i % 3 for i in range(sc.GOLDEN_N)] if positives == "mod3" else None
        mask = None if positives == "mod3" else torch.from_numpy(src[f"{positives}_mask"])
        a = torch.from_numpy(src["z1"]).double().requires_grad_(True)
        b = torch.from_numpy(src["z2"]).double().requires_grad_(True)
        loss, ratio = onr.self_paced_supcon(a, b, target, gamma=float(g[f"{tag}_gamma"]), weight_update=mode,
                                            correct_grad=cg == "c1", t=sc.T, mask=mask)
        (loss * sc.GSCALE).backward()
        # the reference's hard weights are a float32 tensor whatever the inputs ((l <= gamma).float(), contrastive.py:201),
        # so its "float64" hard ratio is an exact count divided in float32: one rounding, 2^-24 relative -- and so is the
        # loss that correct_grad divides by it
        rtol = 2.0 ** -24 if mode == "hard" else 1e-12
        want = float(g[f"{tag}_loss"])
        ltol = rtol if cg == "c1" else 1e-12
        assert abs(loss.item() - want) <= ltol * abs(want), (tag, loss.item(), want)
        assert abs(ratio - float(g[f"{tag}_ratio"])) <= rtol * abs(float(g[f"{tag}_ratio"])), tag
        for got, key in ((a.grad, "dz1"), (b.grad, "dz2")):   # (the record is rounded to f32: 6e-8 of its size)
            ref = torch.from_numpy(g[f"{tag}_{key}"]).double()
            assert float((got - ref).abs().max()) <= 1e-7 * float(ref.abs().max()), (tag, key)


# ---------------------------------------------------------------- python surface
def test_global_negatives_reaches_the_epoch_hook():
    from contrastyou.arch import UNet
    from contrastyou.hooks.base import TrainerHook
    from semi_seg.hooks import create_sp_infonce_hooks
    from semi_seg.hooks.infonce import SelfPacedINFONCEHook, _SPINFONCEEpochHook
    for fn in (create_sp_infonce_hooks, SelfPacedINFONCEHook.__init__):
        assert inspect.signature(fn).parameters["global_negatives"].default is False
    model = UNet(input_dim=1, num_classes=4, max_channel=128)
    for flag in (False, True):
        type(TrainerHook).names.clear()
        hooks = create_sp_infonce_hooks(model=model, feature_names=["Conv5", "Conv4"], weights=0.5, contrast_ons="partition",
                                        data_name="acdc", mode="soft", max_epoch=4, global_negatives=flag)
        for h in hooks._hooks:
            assert isinstance(h, SelfPacedINFONCEHook) and h._global_negatives is flag
            epoch_hook = h()
            assert isinstance(epoch_hook, _SPINFONCEEpochHook) and epoch_hook._global_negatives is flag
            assert h._criterion.defer_checks is True, "the epoch hook defers the criterion's checks"
            epoch_hook._extractor.remove()
    type(TrainerHook).names.clear()


def test_defer_checks_defaults_to_the_reference_behaviour():
    from contrastyou.losses import SelfPacedSupConLoss, SupConLoss1
    crit = SelfPacedSupConLoss(weight_update="soft")
    assert crit.defer_checks is False and crit.age_param == 1e6
    assert callable(crit.validate) and crit.validate() is None, "nothing pending: nothing raised"
    for name in ("sim_exp", "sim_logits", "pos_mask", "neg_mask", "sp_mask"):
        assert isinstance(getattr(SelfPacedSupConLoss, name), property)
        with pytest.raises(AttributeError):
            getattr(crit, name)
    assert inspect.signature(SelfPacedSupConLoss.validate).parameters.keys() == inspect.signature(SupConLoss1.validate).parameters.keys()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(torch.zeros(2, 8), torch.zeros(2, 8))
