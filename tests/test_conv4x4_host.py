"""Host-side checks of the implicit-GEMM 4 x 4 convolutions (csrc/cy_conv4x4.hip; no GPU): the argument checks and the
workspace size of every entry point -- handed host buffers, so no launch may ever happen -- the ABI version, the
CPU-tensor refusal of `Conv4x4Fn` and the class attribute that selects the discriminator's convolution."""
import ctypes

import pytest
import torch

ARG, SHAPE, WS = -1, -2, -5
ENTRIES = ("cy_conv4x4_pack_weights", "cy_conv4x4_fwd", "cy_conv4x4_dgrad", "cy_conv4x4_wgrad_ws_bytes",
           "cy_conv4x4_wgrad")
BIG = 1 << 40
_HOST = (ctypes.c_float * 80)()


@pytest.fixture(scope="module")
def lib():
    from cyhip import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def p():
    """a 16-byte aligned host buffer: no launch may ever see it"""
    addr = ctypes.addressof(_HOST)
    return addr + (-addr) % 16


def geometry_calls(lib, p, geom):
    """every entry that takes the geometry (N, H, W, Cin, Cout, ksize, stride, pad), on host pointers"""
    return [("fwd", lib.cy_conv4x4_fwd(p, p, p, *geom, None)),
            ("dgrad", lib.cy_conv4x4_dgrad(p, p, p, *geom, None)),
            ("wgrad", lib.cy_conv4x4_wgrad(p, p, p, *geom, p, BIG, None))]


def test_library_exports_the_new_entries_and_the_abi_version_stays(lib):
    from cyhip import _lib
    assert lib.cy_abi_version() == _lib.ABI_VERSION
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.exported_names(), name


def test_null_pointers_are_refused_before_any_launch(lib, p):
    geom = [2, 8, 8, 4, 32, 4, 2, 1]

    def each_null(fn, args, slots):
        for i in slots:
            a = list(args)
            a[i] = None
            assert fn(*a) == ARG, (fn.__name__, i)

    each_null(lib.cy_conv4x4_pack_weights, [p, p, 4, 32, 0, None], (0, 1))
    each_null(lib.cy_conv4x4_fwd, [p, p, p] + geom + [None], (0, 1, 2))
    each_null(lib.cy_conv4x4_dgrad, [p, p, p] + geom + [None], (0, 1, 2))
    each_null(lib.cy_conv4x4_wgrad, [p, p, p] + geom + [p, BIG, None], (0, 1, 2, 11))


@pytest.mark.parametrize("slot", range(5))
@pytest.mark.parametrize("bad", [0, -3])
def test_non_positive_sizes_are_refused(lib, p, slot, bad):
    geom = [2, 8, 8, 4, 32, 4, 2, 1]
    geom[slot] = bad  # N, H, W, Cin, Cout
    for name, rc in geometry_calls(lib, p, geom):
        assert rc == ARG, (name, geom, rc)
    assert lib.cy_conv4x4_wgrad_ws_bytes(*geom) == 0
    if slot >= 3:
        cin, cout = geom[3], geom[4]
        assert lib.cy_conv4x4_pack_weights(p, p, cin, cout, 0, None) == ARG
        assert lib.cy_conv4x4_pack_weights(p, p, cin, cout, 1, None) == ARG


@pytest.mark.parametrize("ksp", [(3, 2, 1), (4, 2, 0), (4, 1, 1), (4, 2, 2), (5, 2, 1), (4, 3, 1), (4, 4, 0), (2, 2, 0),
                                 (1, 1, 0)])
def test_unsupported_kernel_stride_pad_is_a_shape_error(lib, p, ksp):
    geom = [2, 8, 8, 4, 32, *ksp]
    for name, rc in geometry_calls(lib, p, geom):
        assert rc == SHAPE, (name, ksp, rc)
    assert lib.cy_conv4x4_wgrad_ws_bytes(*geom) == 0


@pytest.mark.parametrize("hw,stride,pad", [((1, 8), 2, 1), ((8, 1), 2, 1), ((3, 8), 1, 0), ((8, 3), 1, 0), ((1, 1), 2, 1)])
def test_an_input_smaller_than_the_kernel_is_a_shape_error(lib, p, hw, stride, pad):
    geom = [2, hw[0], hw[1], 4, 32, 4, stride, pad]
    for name, rc in geometry_calls(lib, p, geom):
        assert rc == SHAPE, (name, geom, rc)
    # the smallest inputs that do give an output are accepted by the size query
    assert lib.cy_conv4x4_wgrad_ws_bytes(1, 2, 2, 1, 1, 4, 2, 1) > 0
    assert lib.cy_conv4x4_wgrad_ws_bytes(1, 4, 4, 1, 1, 4, 1, 0) > 0


def test_maps_past_the_31_bit_pixel_index_are_refused(lib, p):
    """pixel indices are 32-bit inside the kernels (element offsets are 64-bit): N * H * W > 2^31 - 1 -> CY_ERR_ARG"""
    for geom in ([1 << 16, 256, 256, 1, 32, 4, 2, 1], [2, 1 << 15, 1 << 15, 4, 1, 4, 1, 0],
                 [(1 << 31) // (64 * 64), 64, 64, 4, 32, 4, 2, 1]):
        for name, rc in geometry_calls(lib, p, geom):
            assert rc == ARG, (name, geom, rc)
        assert lib.cy_conv4x4_wgrad_ws_bytes(*geom) == 0
    for geom in ([2, 8, 8, (1 << 20) + 1, 32, 4, 2, 1], [2, 8, 8, 4, (1 << 20) + 1, 4, 2, 1]):
        for name, rc in geometry_calls(lib, p, geom):
            assert rc == ARG, (name, geom, rc)


def ws_formula(N, H, W, Cin, Cout, stride, pad):
    """the formula of include/contrastyou_hip.h"""
    Ho, Wo = (H + 2 * pad - 4) // stride + 1, (W + 2 * pad - 4) // stride + 1
    M, K = N * Ho * Wo, 16 * Cin
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    if Cout >= 32:
        tiles, rows_min = cdiv(Cout, 128) * cdiv(K, 128), 512
    else:
        tiles, rows_min = cdiv(Cout * K, 256), 64
    splits = max(1, min(cdiv(256, tiles), cdiv(M, rows_min), 256))
    return 4 * splits * Cout * K


@pytest.mark.parametrize("geom", [(16, 112, 112, 64, 128, 2, 1), (16, 224, 224, 5, 64, 2, 1), (16, 14, 14, 512, 1, 1, 0),
                                  (5, 34, 30, 12, 24, 2, 1), (1, 4, 4, 3, 6, 2, 1), (16, 28, 28, 256, 512, 2, 1),
                                  (2, 7, 6, 8, 40, 1, 0)])
def test_wgrad_workspace_size_and_a_short_workspace(lib, p, geom):
    N, H, W, Cin, Cout, stride, pad = geom
    want = ws_formula(*geom)
    assert want > 0 and want % (64 * Cin * Cout) == 0
    assert lib.cy_conv4x4_wgrad_ws_bytes(N, H, W, Cin, Cout, 4, stride, pad) == want
    assert lib.cy_conv4x4_wgrad(p, p, p, N, H, W, Cin, Cout, 4, stride, pad, p, want - 1, None) == WS
    assert lib.cy_conv4x4_wgrad(p, p, p, N, H, W, Cin, Cout, 4, stride, pad, p, 0, None) == WS


def test_wrapper_raises_on_a_refused_call(p):
    from cyhip import _lib
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_SHAPE"):
        _lib.call("cy_conv4x4_fwd", p, p, p, 2, 8, 8, 4, 32, 3, 1, 1, None)
    with pytest.raises(_lib.HipKernelError, match="CY_ERR_WORKSPACE"):
        _lib.call("cy_conv4x4_wgrad", p, p, p, 2, 8, 8, 4, 32, 4, 2, 1, p, 15, None)


def test_conv4x4fn_refuses_cpu_tensors():
    from contrastyou.arch.discriminator import conv_implicit
    from cyhip.glue import Conv4x4Fn
    x, w = torch.rand(2, 4, 8, 8), torch.rand(6, 4, 4, 4, requires_grad=True)
    for call in (lambda: Conv4x4Fn.apply(x, w, 2, 1), lambda: Conv4x4Fn.apply(x, w, 1, 0),
                 lambda: conv_implicit(x, w, 2, 1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_discriminator_convolution_is_a_class_attribute():
    """the default is the implicit-GEMM function; the class attribute (no environment switch) restores `Conv2dFn`"""
    from contrastyou.arch import discriminator as D
    from cyhip import glue
    assert D.Discriminator.conv is D.conv_implicit
    assert D.Discriminator(5, 3).conv is D.conv_implicit
    calls = []

    class Tap:
        @staticmethod
        def apply(*args):
            calls.append(args)
            raise RuntimeError("tapped")

    x, w = torch.rand(1, 5, 8, 8), torch.rand(3, 5, 4, 4)
    for fn, owner, nargs in ((D.conv_implicit, "Conv4x4Fn", 4), (D.conv_im2col, "Conv2dFn", 5)):
        original = getattr(D, owner)
        assert original is getattr(glue, owner)
        setattr(D, owner, Tap)
        try:
            with pytest.raises(RuntimeError, match="tapped"):
                fn(x, w, 2, 1)
        finally:
            setattr(D, owner, original)
        assert len(calls.pop()) == nargs and not calls
    D.Discriminator.conv = staticmethod(D.conv_im2col)
    try:
        assert D.Discriminator(5, 3).conv is D.conv_im2col
    finally:
        D.Discriminator.conv = staticmethod(D.conv_implicit)
    assert D.Discriminator.conv is D.conv_implicit
