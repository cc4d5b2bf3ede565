"""Host-side checks of the supervised criteria (no GPU): the entry points of csrc/cy_seg_loss.hip are declared, exported
and refuse bad arguments before any launch with the status include/contrastyou_hip.h documents, the workspace queries
follow their documented formulas, `KL_div` / `DiceLoss` construct as the reference's do, and the fused paths have no
CPU fallback.  No kernel runs here and the oracle is not imported."""
import ctypes
import re

import pytest
import torch

from test_abi import HEADER, header_symbols

ARG, SHAPE, WS = -1, -2, -5
ENTRIES = ("cy_softmax_wkl_ws_bytes", "cy_softmax_wkl_fwd", "cy_softmax_wkl_map_fwd", "cy_softmax_wkl_bwd",
           "cy_softmax_wkl_map_bwd", "cy_softmax_dice_ws_bytes", "cy_softmax_dice_fwd", "cy_softmax_dice_bwd")
NPIX = (1, 255, 256, 257, 361, 262144, 262145)


@pytest.fixture(scope="module")
def lib():
    from cyhip import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def host():
    """a host buffer: no launch may ever see its address"""
    buf = (ctypes.c_float * 64)()
    return buf, ctypes.addressof(buf)


def _entries(lib, p, big, npix=361, K=4, N=3, HW=361):
    """name -> (function, arguments, indices of the pointers that must not be NULL), all arguments valid"""
    return {
        "wkl_fwd": (lib.cy_softmax_wkl_fwd, [p, p, p, p, npix, K, 1e-16, float(npix), p, big, None], (0, 1, 3, 8)),
        "wkl_map_fwd": (lib.cy_softmax_wkl_map_fwd, [p, p, p, p, npix, K, 1e-16, None], (0, 1, 3)),
        "wkl_bwd": (lib.cy_softmax_wkl_bwd, [p, p, p, p, p, npix, K, 1e-16, float(npix), None], (0, 1, 3, 4)),
        "wkl_map_bwd": (lib.cy_softmax_wkl_map_bwd, [p, p, p, p, p, npix, K, 1e-16, None], (0, 1, 3, 4)),
        "dice_fwd": (lib.cy_softmax_dice_fwd, [p, p, p, p, N, HW, K, 2, 1.0, -1, 0, p, big, None], (0, 1, 2, 3, 11)),
        "dice_bwd": (lib.cy_softmax_dice_bwd, [p, p, p, p, p, N, HW, K, 2, -1, 0, None], (0, 1, 2, 3, 4)),
    }


def test_the_new_symbols_are_declared_and_exported(lib):
    from cyhip import _lib
    declared = header_symbols()
    for name in ENTRIES:
        assert name in declared, f"{name} is not in the header"
        assert hasattr(lib, name) and name in _lib.exported_names(), name
    assert lib.cy_abi_version() == _lib.ABI_VERSION == 19  # (v19: the plan queries answer through structs)
    # pointers and scalars of types the binding already had a row for: the weight, the table and the workspace travel
    # as plain pointers, denom and smooth as doubles
    from ctypes import c_double, c_float, c_int, c_long, c_size_t, c_void_p as P
    assert _lib._SIGS["cy_softmax_wkl_fwd"] == (c_int, [P, P, P, P, c_long, c_int, c_float, c_double, P, c_size_t, P])
    assert _lib._SIGS["cy_softmax_dice_fwd"] == (c_int, [P, P, P, P, c_int, c_long, c_int, c_int, c_double, c_int,
                                                         c_int, P, c_size_t, P])
    assert _lib._SIGS["cy_softmax_dice_ws_bytes"] == (c_size_t, [c_int, c_long, c_int])


def test_every_ws_query_is_documented_in_the_header():
    text = HEADER.read_text()
    for query in ("cy_softmax_wkl_ws_bytes", "cy_softmax_dice_ws_bytes"):
        assert re.search(r"^ \* ws_bytes >= [^\n]*= %s\(" % query, text, flags=re.M), query


def test_null_pointers_are_refused_before_any_launch(lib, host):
    _, p = host
    for name, (fn, args, ptrs) in _entries(lib, p, 1 << 20).items():
        for i in ptrs:
            bad = list(args)
            bad[i] = None
            assert fn(*bad) == ARG, (name, i)


def test_counts_below_one_are_refused(lib, host):
    _, p = host
    for npix in (0, -1):
        for name, (fn, args, _) in _entries(lib, p, 1 << 20, npix=npix, N=3, HW=npix).items():
            assert fn(*args) == ARG, (name, npix)
    for name, (fn, args, _) in _entries(lib, p, 1 << 20, N=0).items():
        if name.startswith("dice"):
            assert fn(*args) == ARG, name
    # the scalar forms divide by denom
    fn, args, _ = _entries(lib, p, 1 << 20)["wkl_fwd"]
    assert fn(*(args[:7] + [0.0] + args[8:])) == ARG
    fn, args, _ = _entries(lib, p, 1 << 20)["wkl_bwd"]
    assert fn(*(args[:8] + [0.0] + args[9:])) == ARG


def test_dice_refuses_an_exponent_or_reduction_it_has_no_kernel_for(lib, host):
    _, p = host
    big = 1 << 20
    for P in (0, 3):
        assert lib.cy_softmax_dice_fwd(p, p, p, p, 3, 361, 4, P, 1.0, -1, 0, p, big, None) == ARG
        assert lib.cy_softmax_dice_bwd(p, p, p, p, p, 3, 361, 4, P, -1, 0, None) == ARG
    for red in (-1, 3):
        assert lib.cy_softmax_dice_fwd(p, p, p, p, 3, 361, 4, 2, 1.0, -1, red, p, big, None) == ARG
        assert lib.cy_softmax_dice_bwd(p, p, p, p, p, 3, 361, 4, 2, -1, red, None) == ARG


@pytest.mark.parametrize("K", [0, 17, -4, 64])
def test_class_counts_outside_1_to_16_are_a_shape_error(lib, host, K):
    _, p = host
    for name, (fn, args, _) in _entries(lib, p, 1 << 20, K=K).items():
        assert fn(*args) == SHAPE, (name, K)
    assert lib.cy_softmax_dice_ws_bytes(3, 361, K) == 0


def test_a_short_workspace_is_refused(lib, host):
    _, p = host
    need = lib.cy_softmax_wkl_ws_bytes(361)
    assert need == 16
    fn, args, _ = _entries(lib, p, need - 1)["wkl_fwd"]
    assert fn(*args) == WS
    need = lib.cy_softmax_dice_ws_bytes(3, 361, 4)
    assert need == 24 * 3 * 2 * 4
    fn, args, _ = _entries(lib, p, need - 1)["dice_fwd"]
    assert fn(*args) == WS
    fn, args, _ = _entries(lib, p, 0)["dice_fwd"]
    assert fn(*args) == WS


def test_wrapper_raises_on_a_refused_call(host):
    from cyhip import _lib
    _, p = host
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_SHAPE"):
        _lib.call("cy_softmax_wkl_map_fwd", p, p, None, p, 361, 17, 1e-16, None)
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_ARG"):
        _lib.call("cy_softmax_dice_bwd", p, p, None, p, p, 3, 361, 4, 2, -1, 0, None)


@pytest.mark.parametrize("npix", NPIX)
def test_workspace_sizes(lib, npix):
    """weighted KL: one f64 partial per block of 256 pixels, at most 1024 blocks.  Dice: per image
    B = min(ceil(HW / 256), max(1, 1024 // N)) blocks, each K pairs of f64 and K int64 counts"""
    blocks = min(max((npix + 255) // 256, 1), 1024)
    assert lib.cy_softmax_wkl_ws_bytes(npix) == 8 * blocks
    assert lib.cy_softmax_wkl_ws_bytes(npix) == lib.cy_softmax_kl_ws_bytes(npix)  # the shared cy_blocks(npix, 256, LOSS_GRID_CAP)
    for N in (1, 2, 3, 16, 1025):
        for K in (1, 4, 5, 16):
            B = min((npix + 255) // 256, max(1, 1024 // N))
            assert lib.cy_softmax_dice_ws_bytes(N, npix, K) == 24 * N * B * K, (N, npix, K)
    assert lib.cy_softmax_dice_ws_bytes(0, npix, 4) == 0 and lib.cy_softmax_dice_ws_bytes(2, 0, 4) == 0


# ---------------------------------------------------------------------------------------------- modules
def test_the_names_are_exported():
    import contrastyou.losses as losses
    from contrastyou.losses.dice_loss import BinaryDiceLoss, DiceLoss, make_one_hot
    assert losses.DiceLoss is DiceLoss and losses.BinaryDiceLoss is BinaryDiceLoss
    assert losses.make_one_hot is make_one_hot
    from cyhip.functions import SoftmaxDiceFn, SoftmaxWeightedKLFn
    assert issubclass(SoftmaxDiceFn, torch.autograd.Function) and issubclass(SoftmaxWeightedKLFn,
                                                                             torch.autograd.Function)


def test_dice_loss_with_class_weights_is_refused_at_construction():
    from contrastyou.losses.dice_loss import DiceLoss
    with pytest.raises(NotImplementedError, match="self.weights"):
        DiceLoss(weight=torch.ones(4))
    with pytest.raises(NotImplementedError):
        DiceLoss(weight=[1.0, 2.0], ignore_index=0)
    crit = DiceLoss(ignore_index=0, smooth=1e-5, p=1, reduction="sum")
    assert crit.weight is None and crit.ignore_index == 0
    assert crit.kwargs == dict(smooth=1e-5, p=1, reduction="sum")
    with pytest.raises(TypeError):
        DiceLoss(no_such_keyword=1)


def test_kl_div_constructs_as_the_reference_does():
    from contrastyou.losses.kl import KL_div
    assert KL_div(weight=[1, 3]).fusable is True
    assert KL_div().fusable is True and KL_div(reduction="sum").fusable is True
    assert KL_div(reduction="none", weight=[1, 2, 3]).fusable is True
    # kl.py:108: weight / weight.sum() * len(weight), in f32
    for w in ([1, 3], [1.0, 2.0, 3.0, 4.0, 5.0], [1, 0, 3, 4]):
        want = torch.tensor(w).float()
        want = want / want.sum() * len(want)
        for given in (w, torch.tensor(w)):
            got = KL_div(weight=given)._weight
            assert got.dtype == torch.float32 and torch.equal(got, want), (w, got)
    assert KL_div()._weight is None
    with pytest.raises(AssertionError):
        KL_div(reduction="average")


def test_make_one_hot():
    from contrastyou.losses.dice_loss import make_one_hot
    y = torch.tensor([[[[0, 2], [1, 1]]]])
    got = make_one_hot(y, 3)
    assert got.shape == (1, 3, 2, 2) and got.dtype == torch.float32
    assert torch.equal(got, torch.nn.functional.one_hot(y[:, 0], 3).movedim(-1, 1).float())


def _dice_formula(p, onehot, *, smooth=1.0, P=2, ignore=None, reduction="mean"):
    """the issue's formulas in f64, per image and class; the divisor counts the ignored class"""
    p, onehot = p.double(), onehot.double()
    K = p.shape[1]
    num = (p * onehot).flatten(2).sum(2) + smooth
    den = (p ** P).flatten(2).sum(2) + onehot.flatten(2).sum(2) + smooth
    L = 1 - num / den
    if ignore is not None:
        L = L[:, [c for c in range(K) if c != ignore]]
    L = L.sum(1) / K
    return {"mean": L.mean(), "sum": L.sum(), "none": L}[reduction]


@pytest.mark.parametrize("kw", [dict(), dict(reduction="sum"), dict(reduction="none"), dict(ignore_index=0),
                                dict(ignore_index=3), dict(p=1), dict(smooth=1e-5), dict(p=3)])
def test_dice_forward_is_the_formula_on_the_cpu(kw):
    """the probability-space path runs anywhere, in torch ops"""
    from contrastyou.losses.dice_loss import DiceLoss, make_one_hot
    gen = torch.Generator().manual_seed(4)
    p = torch.randn(3, 4, 7, 5, generator=gen, dtype=torch.float64).softmax(1)
    y = torch.randint(0, 4, (3, 1, 7, 5), generator=gen)
    onehot = make_one_hot(y, 4).double()
    got = DiceLoss(**kw)(p, onehot)
    want = _dice_formula(p, onehot, smooth=kw.get("smooth", 1.0), P=kw.get("p", 2), ignore=kw.get("ignore_index"),
                         reduction=kw.get("reduction", "mean"))
    assert got.shape == want.shape and torch.allclose(got, want, rtol=1e-13, atol=0)


def test_kl_forward_takes_images_that_are_not_square():
    """(the reference's weighted forward does not: its weight map comes out as [b, c, W, H])"""
    from contrastyou.losses.kl import KL_div
    gen = torch.Generator().manual_seed(5)
    p = torch.randn(2, 3, 17, 19, generator=gen, dtype=torch.float64).softmax(1)
    y = torch.randint(0, 3, (2, 17, 19), generator=gen)
    onehot = torch.nn.functional.one_hot(y, 3).movedim(-1, 1).double()
    crit = KL_div(weight=[1, 2, 3], reduction="none")
    got = crit(p, onehot)
    want = -crit._weight.double()[y] * torch.log((p.gather(1, y[:, None])[:, 0] + 1e-16) / (1 + 1e-16))
    assert got.shape == (2, 17, 19) and torch.allclose(got, want, rtol=1e-13, atol=0)


def test_fused_paths_have_no_cpu_fallback():
    from contrastyou.losses.dice_loss import DiceLoss
    from contrastyou.losses.kl import KL_div
    z, y = torch.randn(2, 4, 5, 7), torch.randint(0, 4, (2, 5, 7))
    crits = [KL_div(weight=[1, 2, 2, 2]), KL_div(reduction="sum"), KL_div(reduction="none"),
             KL_div(reduction="none", weight=[1, 0, 3, 4]), KL_div(),
             DiceLoss(), DiceLoss(ignore_index=0), DiceLoss(p=1, reduction="none")]
    for crit in crits:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            crit.from_logits(z, y)


def test_what_has_no_kernel_composes_torch_ops():
    """more than 16 classes (other than the unweighted mean KL_div, which keeps its kernels' answer) and a Dice
    exponent other than 1 or 2 run the probability-space forward: on the CPU too"""
    from contrastyou.losses.dice_loss import DiceLoss, make_one_hot
    from contrastyou.losses.kl import KL_div
    gen = torch.Generator().manual_seed(6)
    z, y = torch.randn(2, 17, 5, 7, generator=gen), torch.randint(0, 17, (2, 5, 7), generator=gen)
    onehot = make_one_hot(y[:, None], 17)
    for crit in (KL_div(reduction="sum"), KL_div(weight=list(range(1, 18))), DiceLoss()):
        assert torch.equal(crit.from_logits(z, y), crit(z.softmax(1), onehot))
    z4, y4 = z[:, :4], y % 4
    crit = DiceLoss(p=3)
    assert torch.equal(crit.from_logits(z4, y4), crit(z4.softmax(1), make_one_hot(y4[:, None], 4)))
