"""Loader augmentation without a GPU: the NumPy restatement of tests/augment_cases.py against Pillow itself and the
goldens, bit for bit; the draws of contrastyou/augment/device.py; augment_zoo against the reference's numbers; the
store; the plan and the refusals of csrc/cy_augment.hip (checked on host copies of the tables, so they need no GPU)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import augment_cases as ac

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
import gen_goldens_augment as gg  # noqa: E402

GOLDEN = np.load(Path(__file__).resolve().parent / "golden" / "augment.npz")


# ---- the restatement is Pillow -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ac.CASES))
def test_restatement_equals_pillow_and_the_goldens(name):
    """0 differing pixels: the geometry (bilinear for images, nearest for labels), the jitter, against Pillow run here
    and against the stored run"""
    c = ac.case(name)
    geo, jit, lab = gg.pillow_case(ac.CASES[name])
    lab_raw = np.stack([ac.geometry(c["sources"][v["slice"]][1], v, c["out_hw"], True) for v in c["views"]])
    for tag, live, mine in (("geo", geo, c["geo"]), ("jit", jit, c["jit"]), ("lab", lab, lab_raw)):
        assert live.dtype == np.uint8 and np.array_equal(live, mine), (name, tag, int((live != mine).sum()))
        assert np.array_equal(GOLDEN[f"{name}_{tag}"], mine), (name, tag)
    assert np.array_equal(GOLDEN[f"{name}_ip"], c["ip"]) and np.array_equal(GOLDEN[f"{name}_fp"], c["fp"])
    assert np.array_equal(c["labels"][:, 0], ac.label_lut(c["mapping"])[lab_raw])
    assert c["images"].dtype == np.float32 and c["labels"].dtype == np.int64


def test_cases_are_not_trivial():
    """the rotations move pixels and mix them, the jitter changes them and clips, the mapping maps, the saturation
    step does nothing"""
    c = ac.case("rot_flip_crop_37x45")
    assert len({g.tobytes() for g in c["geo"]}) == 8 and (c["geo"] == 0).any() and c["labels"].max() == 3
    c = ac.case("jitter_orders")
    assert len({j.tobytes() for j in c["jit"][:6]}) == 2  # brightness before or after contrast; saturation nowhere
    assert all((j != g).any() for j, g, v in zip(c["jit"], c["geo"], c["views"])
               if [s for s in v["jitter"] if s[0] != "s" and s[1] != 1.0])
    c = ac.case("jitter_clip_and_half")
    assert (c["jit"][4:7] == 255).all() and (c["jit"][7] == 127).all() and (c["jit"][:4] == 0).all()
    # contrast 1.5 about mean 12 (11.5 rounds up): 12 - 3 and trunc(12 + 1.5); about 11 it would be 9 and 14
    assert sorted(np.unique(c["jit"][10]).tolist()) == [9, 13]
    c = ac.case("label_mapping_myo")
    assert set(np.unique(c["labels"]).tolist()) == {0, 1}
    c = ac.case("post_window_outside")
    assert not c["geo"].any() and not c["labels"].any()
    sq = ac.case("square_right_angles")
    src = sq["sources"][0][0]
    assert np.array_equal(sq["geo"][1], np.rot90(src)) and np.array_equal(sq["geo"][2], src[::-1, ::-1])
    assert np.array_equal(sq["geo"][0], src) and np.array_equal(sq["geo"][5], src)


def test_to_tensor_table_is_torchs():
    want = torch.arange(256, dtype=torch.uint8).float().div(255).numpy()
    assert np.array_equal(want.view(np.uint32), ac.TENSOR_LUT.view(np.uint32))


def test_record_layout_is_the_headers():
    from contrastyou.augment import device as dv
    from cyhip import _lib
    assert (_lib.CY_AUG_IP_LEN, _lib.CY_AUG_FP_LEN) == (ac.IP_LEN, ac.FP_LEN)
    for k, i in ac.IP.items():
        name = {"fv": "FLIPV", "fh": "FLIPH"}.get(k, k.upper())
        assert getattr(_lib, "CY_AUG_IP_" + name) == i, k
    assert (_lib.CY_AUG_FP_M0, _lib.CY_AUG_FP_F0) == (ac.FP["m0"], ac.FP["f0"])
    assert (_lib.CY_AUG_BRIGHTNESS, _lib.CY_AUG_CONTRAST) == (ac.KIND["b"], ac.KIND["c"])
    assert (_lib.CY_AUG_MAX_SIDE, _lib.CY_AUG_MAX_OUT, _lib.CY_AUG_MAX_VIEWS) == (ac.MAX_SIDE, ac.MAX_OUT, ac.MAX_VIEWS)
    assert (_lib.CY_AUG_GEO_BLOCK, _lib.CY_AUG_JIT_BLOCK) == (ac.GEO_BLOCK, ac.JIT_BLOCK)
    assert ac.IP["kind0"] + 3 <= ac.IP["a0"] and ac.IP["a0"] + 6 <= ac.IP_LEN and ac.FP["f0"] + 3 <= ac.FP_LEN
    for angle, cw, ch in ((13.7, 45, 37), (-44.9, 32, 24), (90, 32, 32), (180, 9, 1), (359.5, 1024, 1024)):
        m, a = dv.rotation_matrix(angle, cw, ch)
        assert m == ac.rotate_matrix(angle, cw, ch) and a == ac.fixed_matrix(m)
        assert all(-2 ** 31 <= v < 2 ** 31 for v in a)  # the int32 row holds them at the largest canvas
    assert dv.rotation_matrix(0.0, 8, 8) is None and dv.rotation_matrix(-720.0, 8, 8) is None


# ---- the draws -----------------------------------------------------------------------------------------------------
def _pretrain(**kw):
    from contrastyou.augment import DevicePipeline
    return DevicePipeline(rotation=45, vflip=True, hflip=True, crop=24, jitter=((0.5, 1.5),) * 3, **kw)


GEO_COLS = [ac.IP[k] for k in ("py", "px", "ch", "cw", "rot", "fv", "fh", "qy", "qx")] + list(range(14, 20))
JIT_COLS = [ac.IP["njit"], 11, 12, 13]


def test_draw_repeats_with_its_seed_and_stays_in_its_families():
    p = _pretrain()
    sizes = np.array([[37, 45], [40, 33], [24, 24]] * 200)
    a, b, other = p.draw(600, 5, sizes), p.draw(600, 5, sizes), p.draw(600, 6, sizes)
    assert a.out_hw == (24, 24) and a.int_params.dtype == np.int32 and a.f64_params.dtype == np.float64
    assert np.array_equal(a.int_params, b.int_params) and np.array_equal(a.f64_params, b.f64_params)
    assert not np.array_equal(a.int_params, other.int_params)
    ip, fp = a.int_params, a.f64_params
    assert (ip[:, ac.IP["slice"]] == 0).all() and (ip[:, [ac.IP["py"], ac.IP["px"]]] == 0).all()
    assert np.array_equal(ip[:, [ac.IP["ch"], ac.IP["cw"]]], sizes)
    # crop origins: uniform on 0 .. size - 24, both ends reached
    for col, size in ((ac.IP["qy"], sizes[:, 0]), (ac.IP["qx"], sizes[:, 1])):
        assert (ip[:, col] >= 0).all() and (ip[:, col] <= size - 24).all()
        assert (ip[:, col] == 0).any() and (ip[:, col] == size - 24).any()
    assert 0.4 < ip[:, ac.IP["fv"]].mean() < 0.6 and 0.4 < ip[:, ac.IP["fh"]].mean() < 0.6
    # the angle, read back from the matrix: within +-45 and spread over it
    ang = np.degrees(np.arctan2(fp[:, 1], fp[:, 0]))
    assert (ip[:, ac.IP["rot"]] == 1).all() and np.abs(ang).max() <= 45 and ang.min() < -40 and ang.max() > 40
    # jitter: brightness and contrast in both orders (saturation is drawn and dropped), f32 factors in range
    assert (ip[:, ac.IP["njit"]] == 2).all() and set(map(tuple, ip[:, 11:14])) == {(1, 2, 0), (2, 1, 0)}
    f = fp[:, 6:8]
    assert (f >= 0.5).all() and (f <= 1.5).all() and np.array_equal(f, f.astype(np.float32).astype(np.float64))
    assert (fp[:, 8] == 0).all()


def test_two_views_share_or_differ_as_total_freedom_says():
    sizes = [[37, 45]] * 50
    v1, v2 = _pretrain(total_freedom=False).draw_twice(50, 9, sizes)
    assert np.array_equal(v1.int_params[:, GEO_COLS], v2.int_params[:, GEO_COLS])
    assert np.array_equal(v1.f64_params[:, :6], v2.f64_params[:, :6])
    assert not np.array_equal(v1.f64_params[:, 6:], v2.f64_params[:, 6:])
    f1, f2 = _pretrain(total_freedom=True).draw_twice(50, 9, sizes)
    assert np.array_equal(f1.int_params, v1.int_params) and np.array_equal(f1.f64_params, v1.f64_params)
    assert not np.array_equal(f1.int_params[:, GEO_COLS], f2.int_params[:, GEO_COLS])
    assert not np.array_equal(f1.f64_params[:, :6], f2.f64_params[:, :6])
    assert not np.array_equal(f1.f64_params[:, 6:], f2.f64_params[:, 6:])
    again = _pretrain(total_freedom=True).draw_twice(50, 9, sizes)
    assert all(np.array_equal(x, y) for a, b in zip((f1, f2), again) for x, y in zip(a[:2], b[:2]))
    p = _pretrain()
    one = p.draw(50, 9, sizes)  # the first of two views is the single view of that seed
    assert np.array_equal(one.int_params, f1.int_params) and np.array_equal(one.f64_params, f1.f64_params)
    assert p._total_freedom is True
    p._total_freedom = False  # what the reference's create_tra_test_dataset does to a pipeline of the zoo
    assert p.total_freedom is False


def test_image_and_label_take_one_record():
    """one record per view serves the image and the label: with a label that IS the image and no rotation (nearest and
    bilinear then agree) the two come out alike, and a rotated label is the image's geometry at nearest"""
    from contrastyou.augment import DevicePipeline
    img, _ = ac.noise(37, 45, 11)
    p = DevicePipeline(vflip=True, hflip=True, crop=24, padding=20)
    params = p.draw(40, 3, [[37, 45]])
    assert len({tuple(r) for r in params.int_params[:, [ac.IP["fv"], ac.IP["fh"], ac.IP["qy"], ac.IP["qx"]]]}) > 30
    assert params.int_params[:, ac.IP["qy"]].min() < 0 and params.int_params[:, ac.IP["qy"]].max() > 37 - 24
    for r in params.int_params[:8]:
        v = ac.view(fv=bool(r[ac.IP["fv"]]), fh=bool(r[ac.IP["fh"]]), post=(int(r[ac.IP["qy"]]), int(r[ac.IP["qx"]])))
        assert np.array_equal(ac.geometry(img, v, (24, 24), False), ac.geometry(img, v, (24, 24), True))


def test_window_draws_of_the_label_pipelines():
    from contrastyou.augment import DevicePipeline, center_crop_offset
    acdc = DevicePipeline(pre_crop=24, rotation=30).draw(300, 1, [[37, 45]])
    ip = acdc.int_params
    assert acdc.out_hw == (24, 24) and (ip[:, [3, 4]] == 24).all() and (ip[:, [8, 9]] == 0).all()
    assert ip[:, 1].min() == 0 and ip[:, 1].max() == 13 and ip[:, 2].min() == 0 and ip[:, 2].max() == 21
    hippo = DevicePipeline(pre_crop=24, padding=20, rotation=10).draw(600, 2, [[24, 24]])
    ip = hippo.int_params
    assert ip[:, 1].min() == -20 and ip[:, 1].max() == 20 and ip[:, 2].min() == -20 and ip[:, 2].max() == 20
    spleen = DevicePipeline(rotation=10, crop=24, padding=20).draw(600, 3, [[37, 45]])
    ip = spleen.int_params
    assert (ip[:, [1, 2]] == 0).all() and ip[:, 8].min() == -20 and ip[:, 8].max() == 33 and ip[:, 9].max() == 41
    val = DevicePipeline(center_crop=24).draw(3, 4, [[37, 45], [24, 24], [20, 30]])
    assert val.int_params[:, [8, 9]].tolist() == [[6, 10], [0, 0], [-2, 3]] and not val.int_params[:, 5].any()
    assert [center_crop_offset(s, 24) for s in (24, 25, 26, 27, 23, 21)] == [0, 0, 1, 2, 0, -1]  # int(round(x / 2.0))
    whole = DevicePipeline().draw(2, 5, [[37, 45]])
    assert whole.out_hw == (37, 45) and not whole.int_params[:, [1, 2, 5, 6, 7, 8, 9, 10]].any()
    with pytest.raises(ValueError, match="one batch, one size"):
        DevicePipeline().draw(2, 5, [[37, 45], [24, 24]])
    with pytest.raises(ValueError, match="does not fit"):
        DevicePipeline(crop=24).draw(1, 5, [[20, 30]])
    with pytest.raises(ValueError):
        DevicePipeline(crop=24, center_crop=24)


# ---- augment_zoo: the reference's numbers, written out (semi_seg/augment.py:36-325) --------------------------------
_A = ((0.5, 1.5),) * 3
_M = ((0.9, 1.1),) * 3
_NONE = dict(pre_crop=None, rotation=None, vflip=False, hflip=False, crop=None, padding=0, center_crop=None,
             jitter=None, total_freedom=True)
_ACDC = dict(presize=None,
             pretrain=dict(rotation=45.0, vflip=True, hflip=True, crop=(224, 224), jitter=_A),
             label=dict(pre_crop=(224, 224), rotation=30.0),
             val=dict(center_crop=(224, 224)), trainval=dict(center_crop=(224, 224)))
ZOO = {
    "acdc": dict(_ACDC, mapping=None),
    "acdc_lv": dict(_ACDC, mapping={0: 0, 1: 0, 2: 0, 3: 1}),
    "acdc_rv": dict(_ACDC, mapping={0: 0, 1: 1, 2: 0, 3: 0}),
    "acdc_myo": dict(_ACDC, mapping={0: 0, 1: 0, 2: 1, 3: 0}),
    "mmwhsct": dict(_ACDC, mapping=None),
    "mmwhsmr": dict(_ACDC, mapping=None),
    "prostate": dict(presize=224, mapping=None,
                     pretrain=dict(rotation=10.0, vflip=True, hflip=True, crop=(224, 224), padding=20, jitter=_M),
                     label=dict(crop=(224, 224)), val=dict(), trainval=dict(center_crop=(224, 224), presize=None)),
    "spleen": dict(presize=320, mapping=None,
                   pretrain=dict(rotation=30.0, vflip=True, hflip=True, crop=(256, 256), padding=20, jitter=_M),
                   label=dict(rotation=10.0, crop=(256, 256), padding=20),
                   val=dict(center_crop=(256, 256)), trainval=dict(center_crop=(256, 256))),
    "hippocampus": dict(presize=(64, 64), mapping=None,
                        pretrain=dict(rotation=10.0, vflip=True, hflip=True, crop=(64, 64), padding=20, jitter=_M),
                        label=dict(pre_crop=(64, 64), padding=20, rotation=10.0),
                        val=dict(), trainval=dict(center_crop=(64, 64), presize=None)),
}
ZOO["prostate_md"] = ZOO["prostate"]


def test_augment_zoo_carries_the_references_numbers():
    from contrastyou.augment import DevicePipeline
    from semi_seg import augment
    assert sorted(augment.augment_zoo) == sorted(ZOO) and len(ZOO) == 10
    assert augment.RisingWrapper is augment.AffineAugment  # the module's earlier names stay
    for key, want in ZOO.items():
        entry = augment.augment_zoo[key]()
        assert entry.presize == want["presize"], key
        for mode in ("pretrain", "label", "val", "trainval"):
            pipe = getattr(entry, mode)
            assert isinstance(pipe, DevicePipeline)
            full = {**_NONE, "presize": want["presize"], "mapping": want["mapping"], **want[mode]}
            got = {k: getattr(pipe, k) for k in full}
            assert got == full, (key, mode, got)
    lut = augment.augment_zoo["acdc_myo"]().label.label_lut()
    assert lut.dtype == np.uint8 and lut[:5].tolist() == [0, 0, 1, 0, 4] and np.array_equal(lut, ac.label_lut(ac.ACDC_MYO))


# ---- the store -----------------------------------------------------------------------------------------------------
def _slices():
    return [ac.noise(*hw, seed=s) for s, hw in enumerate(((37, 45), (45, 37), (24, 24)))]


def test_store_packs_the_arenas_and_the_table():
    from semi_seg.data import DeviceSliceStore
    pairs = _slices()
    names = [f"patient{i // 2:03d}_{i % 2:02d}_{i}" for i in range(3)]
    store = DeviceSliceStore.from_arrays([p[0] for p in pairs], [p[1] for p in pairs], names,
                                         group_re=r"patient\d+_\d+", partitions=[2, 1, 0], device="cpu")
    want_img, want_lab, want_table = ac.pack(pairs)
    assert np.array_equal(store.table.numpy(), want_table) and store.table.dtype == torch.int64
    assert np.array_equal(store.images.numpy(), want_img) and np.array_equal(store.labels.numpy(), want_lab)
    assert store.scan_nums == ["patient000_00", "patient000_01", "patient001_00"] and store.partitions == [2, 1, 0]
    assert len(store) == 3 and store.sizes([2, 0]).tolist() == [[24, 24], [37, 45]]
    with pytest.raises(AttributeError, match="Cannot match pattern"):
        DeviceSliceStore.from_arrays([pairs[0][0]], [pairs[0][1]], ["x"], group_re=r"patient\d+", device="cpu")
    with pytest.raises(ValueError, match="uint8"):
        DeviceSliceStore.from_arrays([pairs[0][0].astype(np.float32)], [pairs[0][1]], ["patient1"], group_re="p",
                                     device="cpu")
    # ToLabel's mapping is checked once, here
    ok = DeviceSliceStore.from_arrays([pairs[0][0]], [pairs[0][1]], ["patient1"], group_re="patient",
                                      mapping=ac.ACDC_MYO, device="cpu")
    assert len(ok) == 1
    with pytest.raises(KeyError, match="not keys of the mapping"):
        DeviceSliceStore.from_arrays([pairs[0][0]], [pairs[0][1]], ["patient1"], group_re="patient",
                                     mapping={0: 0, 1: 1}, device="cpu")


@pytest.mark.parametrize("presize", [20, (16, 20)])
def test_presize_is_torchvisions_resize_with_pillow(presize):
    """an int sets the smaller edge, the other is int(size * long / short); a pair is (h, w); the pixels are
    Image.resize's, bilinear for images and nearest for labels; portrait and landscape"""
    from PIL import Image
    from semi_seg.data import DeviceSliceStore, presize_hw
    assert presize_hw(37, 45, 20) == (20, 24) and presize_hw(45, 37, 20) == (24, 20) and presize_hw(24, 24, 20) == (20, 20)
    assert presize_hw(37, 45, (16, 20)) == (16, 20)
    pairs = _slices()
    store = DeviceSliceStore.from_arrays([p[0] for p in pairs], [p[1] for p in pairs], ["s0", "s1", "s2"],
                                         group_re=r"s\d", presize=presize, device="cpu")
    for (img, lab), (off, h, w) in zip(pairs, store.table.tolist()):
        assert (h, w) == presize_hw(*img.shape, presize)
        want_i = np.array(Image.fromarray(img).resize((w, h), Image.BILINEAR))
        want_l = np.array(Image.fromarray(lab).resize((w, h), Image.NEAREST))
        assert np.array_equal(store.images[off:off + h * w].numpy().reshape(h, w), want_i)
        assert np.array_equal(store.labels[off:off + h * w].numpy().reshape(h, w), want_l)


def test_presize_without_pillow_names_it(monkeypatch):
    from semi_seg.data import DeviceSliceStore
    monkeypatch.setitem(sys.modules, "PIL", None)
    img, lab = ac.noise(8, 8, 0)
    with pytest.raises(ImportError, match="Pillow"):
        DeviceSliceStore.from_arrays([img], [lab], ["s0"], group_re="s", presize=4, device="cpu")
    assert len(DeviceSliceStore.from_arrays([img], [lab], ["s0"], group_re="s", device="cpu")) == 1  # not needed otherwise


# ---- the plan and the refusals -------------------------------------------------------------------------------------
def test_plan_matches_the_cases_and_the_cases_reach_past_every_cap():
    from cyhip import _lib, ops
    plans = {}
    for name, c in ac.CASES.items():
        p = plans[name] = ops.augment_plan(len(c["views"]), *c["out_hw"])
        assert p == ac.plan(len(c["views"]), *c["out_hw"]), name
        assert p["form"] == _lib.CY_AUG_FORM_TWO_STAGE and p["launches"] == 2
    every = list(plans.values())
    # more than one tile of the geometry grid and more than one trip of the jitter block, neither filled evenly; one
    # tile with idle threads; several views; contrast twice where the block steps several times
    assert any(p["geo_grid_x"] > 1 for p in every) and any(p["geo_grid_x"] == 1 for p in every)
    assert plans["past_one_tile"]["jit_trips"] > 1 and (57 * 61) % ac.JIT_BLOCK and (57 * 61) % ac.GEO_BLOCK
    assert [k for k, _ in ac.CASES["past_one_tile"]["views"][0]["jitter"]].count("c") == 2
    assert any(p["geo_grid_y"] > 8 for p in every) and plans["one_by_nine"]["scratch_bytes"] == 5 * 9
    assert len({s[0].shape for s in ac.CASES["three_sizes"]["sources"]}) == 3
    # C2's batch: 64 views of 224 x 224
    p = ops.augment_plan(64, 224, 224)
    assert (p["geo_grid_x"], p["geo_grid_y"], p["jit_trips"], p["scratch_bytes"]) == (196, 64, 49, 64 * 224 * 224)
    # the limits, and one above each
    for args, want in (((4096, 8, 8), ac.OK), ((4097, 8, 8), ac.ERR_SHAPE), ((1, 512, 512), ac.OK),
                       ((1, 513, 512), ac.ERR_SHAPE), ((1, 512, 513), ac.ERR_SHAPE), ((0, 8, 8), ac.ERR_SHAPE),
                       ((1, 0, 8), ac.ERR_SHAPE), ((4096, 512, 512), ac.OK)):
        p = ops.augment_plan(*args)
        assert p["status"] == want == ac.plan(*args)["status"], args
        if want != ac.OK:
            assert all(v == 0 for k, v in p.items() if k != "status")
    assert ops.augment_plan(4096, 512, 512)["scratch_bytes"] == 2 ** 30
    assert _lib.load().cy_aug_plan(1, 8, 8, None) == ac.ERR_ARG
    assert (ops.AUG_MAX_SIDE, ops.AUG_MAX_OUT, ops.AUG_MAX_VIEWS) == (1024, 512, 4096)


def _call(lib, c, ip=None, table=None, views=None, out_hw=None, arena=None, slices=None, scratch_bytes=1 << 40,
          null=(), labels=True):
    """cy_aug_views on host copies and dummy device pointers: only for arguments it refuses (nothing is launched)"""
    ip = np.ascontiguousarray(c["ip"] if ip is None else ip)
    table = np.ascontiguousarray(c["table"] if table is None else table)
    p = 4096
    a = dict(store_img=p, store_lab=p if labels else None, h_table=table.ctypes.data,
             slices=len(table) if slices is None else slices, arena=len(c["arena_img"]) if arena is None else arena,
             ip=p, h_ip=ip.ctypes.data, fp=p, views=len(ip) if views is None else views,
             out_h=(out_hw or c["out_hw"])[0], out_w=(out_hw or c["out_hw"])[1], label_lut=p, tensor_lut=p, images=p,
             labels=p if labels else None, scratch=p, scratch_bytes=scratch_bytes, stream=None)
    for k in null:
        a[k] = None
    return lib.cy_aug_views(*a.values())


def test_entry_point_refusals_have_their_exact_status():
    from cyhip import _lib
    lib = _lib.load()
    c = ac.case("three_sizes")
    for k in ("store_img", "h_table", "ip", "h_ip", "fp", "label_lut", "tensor_lut", "images", "scratch"):
        assert _call(lib, c, null=(k,)) == ac.ERR_ARG, k
    assert _call(lib, c, null=("store_lab",)) == ac.ERR_ARG and _call(lib, c, null=("labels",)) == ac.ERR_ARG
    assert _call(lib, c, out_hw=(513, 8)) == ac.ERR_SHAPE and _call(lib, c, out_hw=(8, 0)) == ac.ERR_SHAPE
    assert _call(lib, c, views=0) == ac.ERR_SHAPE and _call(lib, c, views=4097) == ac.ERR_SHAPE
    assert _call(lib, c, slices=0) == ac.ERR_SHAPE
    assert _call(lib, c, scratch_bytes=5 * 24 * 24 - 1) == ac.ERR_WORKSPACE
    assert _call(lib, c, scratch_bytes=5 * 24 * 24 - 1, labels=False) == ac.ERR_WORKSPACE  # image views alone are fine

    def ip_with(col, value, row=3):
        ip = c["ip"].copy()
        ip[row, col] = value
        return ip

    I = ac.IP
    for col, value, want in ((I["slice"], 3, ac.ERR_SHAPE), (I["slice"], -1, ac.ERR_SHAPE), (I["ch"], 0, ac.ERR_SHAPE),
                             (I["cw"], 1025, ac.ERR_SHAPE), (I["py"], -4097, ac.ERR_SHAPE), (I["qx"], 4097, ac.ERR_SHAPE),
                             (I["rot"], 2, ac.ERR_ARG), (I["fv"], -1, ac.ERR_ARG), (I["fh"], 2, ac.ERR_ARG),
                             (I["njit"], 4, ac.ERR_ARG), (I["njit"], -1, ac.ERR_ARG), (I["kind0"], 3, ac.ERR_ARG),
                             (I["kind0"], 0, ac.ERR_ARG),
                             # the table row a record carries is not the row of its slice
                             (I["off_lo"], int(c["ip"][3, I["off_lo"]]) + 1, ac.ERR_ARG), (I["off_hi"], 1, ac.ERR_ARG),
                             (I["src_h"], 24, ac.ERR_ARG), (I["src_w"], 34, ac.ERR_ARG)):
        assert _call(lib, c, ip=ip_with(col, value)) == want, (col, value)
    assert _call(lib, c, slices=2) == ac.ERR_SHAPE  # view 0 reads slice 2
    # a table row that leaves the arena, by one byte; a slice larger than the limit; a negative offset
    assert _call(lib, c, arena=len(c["arena_img"]) - 1) == ac.ERR_SHAPE
    for row, col, value in ((2, 0, int(c["table"][2, 0]) + 1), (1, 0, -1), (0, 1, 1025), (0, 2, 0)):
        table = c["table"].copy()
        table[row, col] = value
        assert _call(lib, c, table=table) == ac.ERR_SHAPE, (row, col, value)
    # a table that is valid but not the one the records were filled from (a store rebuilt in another order)
    rebuilt = np.array([[0, 24, 24], [576, 37, 45], [2241, 40, 33]], dtype=np.int64)  # slices 0 and 1 changed places
    assert _call(lib, c, table=rebuilt) == ac.ERR_ARG


def test_python_surface_refuses_cpu_tensors_and_wrong_tables():
    from cyhip import ops
    c = ac.case("three_sizes")
    t = torch.from_numpy
    good = {k: t(np.array(c[k])) for k in ("arena_img", "arena_lab", "table", "ip", "fp")}

    def call(lut=None, **change):
        return ops.augment_views(*{**good, **change}.values(), lut, c["out_hw"])

    with pytest.raises(RuntimeError, match="no CPU fallback"):  # everything in order but the device
        call()
    for change, match in ((dict(table=good["table"].int()), "table is a contiguous host tensor"),
                          (dict(table=good["table"][:, :2].contiguous()), r"table is \[S,3\]"),
                          (dict(table=good["table"].t().contiguous().t()), "table is a contiguous host tensor"),
                          (dict(table=good["table"][:0]), r"table is \[S,3\]"),
                          (dict(ip=good["ip"].long()), "int_params is a contiguous host tensor"),
                          (dict(fp=good["fp"].float()), "f64_params is a contiguous host tensor"),
                          (dict(ip=good["ip"][:, :-1].contiguous()), "one record per view"),
                          (dict(fp=good["fp"][:-1]), "one record per view"),
                          (dict(arena_lab=good["arena_lab"][:-1]), "two flat uint8 arenas of one size"),
                          (dict(arena_lab=None), "two flat uint8 arenas of one size"),
                          (dict(arena_img=good["arena_img"].float()), "two flat uint8 arenas of one size")):
        with pytest.raises(ValueError, match=match):
            call(**change)
    with pytest.raises(ValueError, match="label_lut is uint8"):
        call(lut=torch.arange(255, dtype=torch.uint8))
    assert good["ip"].equal(t(np.array(c["ip"])))  # the caller's records are left as they were
