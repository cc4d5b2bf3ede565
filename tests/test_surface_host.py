"""CPU-side checks of the surface-distance meter: the two C-ABI entries of csrc/cy_surface.hip (present in the
library, the header and the binding; every refusal, made with host pointers so that nothing is launched; the workspace
formula), the class surface of `SurfaceMeter`, and its place among `InferenceEpocher`'s meters."""
import ctypes
import inspect
import math
import re
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
OK, ERR_ARG, ERR_SHAPE, ERR_WORKSPACE = 0, -1, -2, -5
MAX_LINE, MAX_CLASSES = 1024, 64


def _host_buffer():
    """a host address: the entries below return before they would touch it"""
    buf = ctypes.create_string_buffer(4096)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_entries_exist_in_library_header_and_binding():
    from cyhip import _lib
    lib = _lib.load()
    header = (REPO / "include" / "contrastyou_hip.h").read_text()
    assert int(re.search(r"#define CY_SURFACE_MAX_LINE (\d+)", header).group(1)) == MAX_LINE >= 1024
    assert int(re.search(r"#define CY_SURFACE_MAX_CLASSES (\d+)", header).group(1)) == MAX_CLASSES >= 16
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("cy_surface_ws_bytes", "cy_surface_stats"):
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.exported_names(), name
    assert lib.cy_abi_version() == _lib.ABI_VERSION


def test_refusals_are_reported_not_launched():
    from cyhip import _lib
    lib = _lib.load()
    keep, p = _host_buffer()
    classes = (ctypes.c_int32 * 3)(1, 2, 3)
    many = (ctypes.c_int32 * (MAX_CLASSES + 1))(*range(MAX_CLASSES + 1))
    big = 1 << 40

    def stats(pred=p, target=p, cls=classes, R=3, D=4, H=33, W=70, ndim=3, count=p, total=p, maxd2=p, d2=None,
              border=None, ws=p, nbytes=big):
        return lib.cy_surface_stats(pred, target, cls, R, D, H, W, ndim, count, total, maxd2, d2, border, ws, nbytes,
                                    None)

    # a NULL pointer (the two map outputs are optional) or a size < 1 -> CY_ERR_ARG
    for name in ("pred", "target", "cls", "count", "total", "maxd2", "ws"):
        assert stats(**{name: None}) == ERR_ARG, name
    for name in ("D", "H", "W"):
        assert stats(**{name: 0}) == ERR_ARG, name
        assert stats(**{name: -3}) == ERR_ARG, name
    # D * H * W above 2^31 - 1 -> CY_ERR_ARG (whatever the line lengths)
    assert stats(D=2048, H=1024, W=1024) == ERR_ARG
    assert stats(D=1291, H=1291, W=1291) == ERR_ARG
    # a line longer than the LDS line buffer -> CY_ERR_SHAPE
    for name in ("D", "H", "W"):
        assert stats(**{name: MAX_LINE + 1}) == ERR_SHAPE, name
    assert stats(D=1, H=MAX_LINE + 1, W=5, ndim=2) == ERR_SHAPE
    # R outside 1 .. CY_SURFACE_MAX_CLASSES -> CY_ERR_SHAPE
    assert stats(R=0) == ERR_SHAPE
    assert stats(R=-1) == ERR_SHAPE
    assert stats(cls=many, R=MAX_CLASSES + 1) == ERR_SHAPE
    # ndim not 2 or 3, or ndim == 2 with D != 1 -> CY_ERR_SHAPE
    for ndim in (0, 1, 4):
        assert stats(ndim=ndim) == ERR_SHAPE, ndim
    assert stats(ndim=2) == ERR_SHAPE
    assert stats(D=2, ndim=2) == ERR_SHAPE
    # a short workspace -> CY_ERR_WORKSPACE, for every accepted geometry
    for D, H, W, ndim in ((4, 33, 70, 3), (1, 9, 13, 2), (1, 9, 13, 3), (MAX_LINE, 1, 1, 3), (1, 1, MAX_LINE, 2)):
        need = lib.cy_surface_ws_bytes(D, H, W)
        assert need > 0
        assert stats(D=D, H=H, W=W, ndim=ndim, nbytes=need - 1) == ERR_WORKSPACE, (D, H, W)
        assert stats(D=D, H=H, W=W, ndim=ndim, nbytes=0) == ERR_WORKSPACE, (D, H, W)
    with pytest.raises(_lib.HipKernelError):
        _lib.call("cy_surface_stats", p, p, classes, 3, 4, 33, 70, 5, p, p, p, None, None, p, big, None)
    del keep


def test_workspace_size_follows_the_header():
    """roundup(2 V, 16) + 8 V + 2 * 1024 * 24: two border masks, two int32 maps, the partials of both directions"""
    from cyhip import _lib
    lib = _lib.load()
    for D, H, W in ((1, 1, 1), (1, 9, 13), (2, 1, 5), (3, 67, 5), (5, 33, 70), (4, 130, 3), (2, 257, 3), (5, 230, 230),
                    (12, 224, 224), (1024, 1024, 1024)):
        V = D * H * W
        assert lib.cy_surface_ws_bytes(D, H, W) == -(-2 * V // 16) * 16 + 8 * V + 2 * 1024 * 24, (D, H, W)
    # 0 where the launch refuses the sizes
    for D, H, W in ((0, 4, 4), (4, -1, 4), (1025, 4, 4), (4, 4, 1025), (2048, 2048, 2048)):
        assert lib.cy_surface_ws_bytes(D, H, W) == 0, (D, H, W)


def test_surface_meter_class_surface():
    from contrastyou import meters
    from contrastyou.meters import Metric, SurfaceMeter
    from contrastyou.meters import surface_distance as sd
    assert issubclass(SurfaceMeter, Metric)
    assert list(inspect.signature(SurfaceMeter.__init__).parameters) == ["self", "C", "report_axises", "metername"]
    d = {k: v.default for k, v in inspect.signature(SurfaceMeter.__init__).parameters.items() if k != "self"}
    assert d == {"C": 4, "report_axises": None, "metername": "hausdorff"}
    assert SurfaceMeter.meter_choices == {"mod_hausdorff": sd.mod_hausdorff_distance,
                                          "hausdorff": sd.hausdorff_distance,
                                          "average_surface": sd.average_surface_distance}
    assert SurfaceMeter.abbr == {"mod_hausdorff": "MHD", "hausdorff": "HD", "average_surface": "ASD"}
    for name in sd.__all__:
        assert getattr(meters, name) is getattr(sd, name)
    assert list(inspect.signature(sd.hausdorff_distance).parameters) == ["data1", "data2", "voxel_spacing"]
    assert list(inspect.signature(sd.average_surface_distance).parameters) == ["data1", "data2", "voxel_spacing"]
    assert list(inspect.signature(sd.mod_hausdorff_distance).parameters) == ["data1", "data2", "voxel_spacing",
                                                                            "percentile"]
    assert inspect.signature(sd.mod_hausdorff_distance).parameters["percentile"].default == 95
    assert list(inspect.signature(SurfaceMeter._add).parameters) == ["self", "pred", "target", "voxelspacing"]
    # the reference's assertions
    with pytest.raises(AssertionError, match="report_axises"):
        SurfaceMeter(C=4, report_axises=range(1, 4))
    with pytest.raises(AssertionError, match="Incompatible"):
        SurfaceMeter(C=4, report_axises=[1, 5])
    with pytest.raises(AssertionError):
        SurfaceMeter(C=4, metername="chamfer")
    assert SurfaceMeter()._report_axis == [0, 1, 2, 3] and SurfaceMeter()._abbr == "HD"


@pytest.mark.parametrize("metername,ab", [("average_surface", "ASD"), ("hausdorff", "HD"), ("mod_hausdorff", "MHD")])
def test_empty_meter_reports_nans(metername, ab):
    from contrastyou.meters import SurfaceMeter
    m = SurfaceMeter(C=4, report_axises=[1, 2, 3], metername=metername)
    means, stds = m.value()
    assert len(means) == len(stds) == 4 and all(math.isnan(v) for v in list(means) + list(stds))
    s = m.summary()
    assert list(s) == [f"{ab}1", f"{ab}2", f"{ab}3", f"{ab}_mean"]
    assert all(math.isnan(v) for v in s.values())
    assert list(m.detailed_summary()) == [f"{ab}1", f"{ab}2", f"{ab}3"]
    assert m.skipped == 0


def test_voxelspacing_is_refused():
    import torch
    from contrastyou.meters import SurfaceMeter, average_surface_distance, hausdorff_distance, mod_hausdorff_distance
    lab = torch.zeros(1, 2, 4, 4, dtype=torch.int64)
    m = SurfaceMeter(C=4, report_axises=[1, 2, 3], metername="average_surface")
    with pytest.raises(NotImplementedError, match="voxelspacing"):
        m.add(lab, lab, voxelspacing=[1.0, 0.5, 0.5])
    with pytest.raises(NotImplementedError, match="voxelspacing"):
        m.add(lab, lab, 2.0)
    for fn in (average_surface_distance, hausdorff_distance, mod_hausdorff_distance):
        with pytest.raises(NotImplementedError, match="voxel_spacing"):
            fn(lab[0] == 0, lab[0] == 0, voxel_spacing=(1.0, 1.0, 1.0))


def test_cpu_tensors_are_refused():
    import torch
    from contrastyou.meters import SurfaceMeter, average_surface_distance
    from cyhip import ops
    lab = torch.zeros(1, 2, 4, 4, dtype=torch.int64)
    m = SurfaceMeter(C=4, report_axises=[1, 2, 3], metername="average_surface")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.add(lab, lab)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.add(torch.full((1, 4, 4, 4), 0.25), torch.nn.functional.one_hot(lab[:, 0], 4).movedim(-1, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.surface_stats(lab[0], lab[0], [1, 2, 3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        average_surface_distance(lab[0] == 0, lab[0] == 0)
    assert m.summary()["ASD1"] != m.summary()["ASD1"] and m.skipped == 0  # nothing was added


def test_inference_epocher_registers_the_asd_meter():
    import torch
    from contrastyou.arch import UNet
    from contrastyou.losses.kl import KL_div
    from contrastyou.meters import SurfaceMeter
    from semi_seg.epochers import EvalEpocher, InferenceEpocher
    kw = dict(model=UNet(input_dim=1, num_classes=4, max_channel=128), loader=[], sup_criterion=KL_div(), device="cpu",
              scaler=torch.amp.GradScaler("cuda", enabled=False), accumulate_iter=1)
    inf = InferenceEpocher(enable_prediction_saver=False, **kw)
    inf.init()
    stats = dict(inf.meters.statistics())
    assert list(stats) == ["infer"]
    assert set(stats["infer"]) == {"lr", "loss", "dice", "ASD"}
    meter = inf.meters["ASD"]
    assert isinstance(meter, SurfaceMeter)
    assert meter._surface_name == "average_surface" and list(meter._report_axis) == [1, 2, 3] and meter._C == 4
    assert list(stats["infer"]["ASD"]) == ["ASD1", "ASD2", "ASD3", "ASD_mean"]
    # EvalEpocher is unchanged
    ev = EvalEpocher(**kw)
    ev.init()
    assert set(dict(ev.meters.statistics())["eval"]) == {"lr", "loss", "dice"}
