"""The loader augmentation of csrc/cy_augment.hip restated in NumPy, and the cases the host and GPU tests share.

The restatement is the specification of include/contrastyou_hip.h ("On-device loader augmentation") written from
Pillow's formulas: float64 and int64 for the geometry (Image.rotate's matrix, affine_fixed for NEAREST,
affine_transform + bilinear_filter8 for BILINEAR), float32 for the jitter (ImagingBlend), each operation rounded on
its own.  tests/test_augment_host.py holds it against Pillow itself, bit for bit; tests/test_gpu_augment.py holds the
kernels against it, bit for bit: every operation is an integer one or a single IEEE operation both sides round alike,
so the tolerance is zero.

A case is one call: `sources` (image, label) uint8 pairs, `views` (one dict per output view), `out_hw`, `mapping`.
A view: slice, pre = (py, px, ch, cw) or None (the whole source), angle or None, fv, fh, post = (qy, qx),
jitter = [(kind, factor)] in applied order with kind "b", "c" or "s" (saturation: a Pillow step that changes nothing on
mode "L" and that the kernels are not given).
"""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

OK, ERR_ARG, ERR_SHAPE, ERR_WORKSPACE = 0, -1, -2, -5
MAX_SIDE, MAX_OUT, MAX_VIEWS = 1024, 512, 4096
GEO_BLOCK, JIT_BLOCK = 256, 1024
# the record (include/contrastyou_hip.h; test_augment_host.py checks these against the header)
IP_LEN, FP_LEN = 24, 9
IP = dict(slice=0, py=1, px=2, ch=3, cw=4, rot=5, fv=6, fh=7, qy=8, qx=9, njit=10, kind0=11, a0=14, off_lo=20, off_hi=21,
          src_h=22, src_w=23)
FP = dict(m0=0, f0=6)
KIND = {"b": 1, "c": 2}
ACDC_MYO = {0: 0, 1: 0, 2: 1, 3: 0}

TENSOR_LUT = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)  # ToTensor: uint8 -> f32 / 255


# ---- geometry -------------------------------------------------------------------------------------------------------
def rotate_matrix(angle: float, cw: int, ch: int):
    """Image.rotate's matrix for a cw x ch image, None where it returns a copy"""
    angle = angle % 360.0
    if angle == 0:
        return None
    cx, cy = cw / 2, ch / 2
    r = -math.radians(angle)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def fix(v: float) -> int:
    return int(math.floor(v * 65536.0 + 0.5))


def fixed_matrix(m):
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5),
            fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def window(src: np.ndarray, oy: int, ox: int, h: int, w: int) -> np.ndarray:
    """out[y][x] = src[y + oy][x + ox], 0 outside src"""
    out = np.zeros((h, w), dtype=src.dtype)
    H, W = src.shape
    y0, y1, x0, x1 = max(0, -oy), min(h, H - oy), max(0, -ox), min(w, W - ox)
    if y1 > y0 and x1 > x0:
        out[y0:y1, x0:x1] = src[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


def rotate_nearest(c: np.ndarray, m) -> np.ndarray:
    ch, cw = c.shape
    a = [np.int64(v) for v in fixed_matrix(m)]
    y, x = np.meshgrid(np.arange(ch, dtype=np.int64), np.arange(cw, dtype=np.int64), indexing="ij")
    xin = (a[2] + y * a[1] + x * a[0]) >> 16
    yin = (a[5] + y * a[4] + x * a[3]) >> 16
    ok = (xin >= 0) & (xin < cw) & (yin >= 0) & (yin < ch)
    return np.where(ok, c[np.clip(yin, 0, ch - 1), np.clip(xin, 0, cw - 1)], 0).astype(np.uint8)


def rotate_bilinear(c: np.ndarray, m) -> np.ndarray:
    ch, cw = c.shape
    m = [np.float64(v) for v in m]
    y, x = np.meshgrid(np.arange(ch, dtype=np.float64) + 0.5, np.arange(cw, dtype=np.float64) + 0.5, indexing="ij")
    xin = m[0] * x + m[1] * y + m[2]
    yin = m[3] * x + m[4] * y + m[5]
    ok = ~((xin < 0) | (xin >= cw) | (yin < 0) | (yin >= ch))
    xin, yin = xin - 0.5, yin - 0.5
    fx, fy = np.floor(xin), np.floor(yin)
    dx, dy = xin - fx, yin - fy
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    xa, xb, ya = np.clip(x0, 0, cw - 1), np.clip(x0 + 1, 0, cw - 1), np.clip(y0, 0, ch - 1)
    ci = c.astype(np.int64)

    def row(r):
        p, q = ci[r, xa], ci[r, xb]
        return p.astype(np.float64) + (q - p).astype(np.float64) * dx

    v1 = row(ya)
    below = (y0 + 1 >= 0) & (y0 + 1 < ch)
    v2 = np.where(below, row(np.clip(y0 + 1, 0, ch - 1)), v1)
    out = v1 + (v2 - v1) * dy
    return np.where(ok, out.astype(np.int64), 0).astype(np.uint8)  # truncation; out is in 0..255


def geometry(src: np.ndarray, view: dict, out_hw, label: bool) -> np.ndarray:
    """stage A on one slice, forwards as Pillow applies it: pre-window, rotation, flips, post-window"""
    H, W = src.shape
    py, px, ch, cw = view["pre"] or (0, 0, H, W)
    c = window(src, py, px, ch, cw)
    m = view.get("m")  # a matrix given as such (a record read back) stands for the angle
    if m is None and view["angle"] is not None:
        m = rotate_matrix(view["angle"], cw, ch)
    if m is not None:
        c = rotate_nearest(c, m) if label else rotate_bilinear(c, m)
    if view["fv"]:
        c = c[::-1]
    if view["fh"]:
        c = c[:, ::-1]
    return window(c, view["post"][0], view["post"][1], out_hw[0], out_hw[1])


# ---- jitter ---------------------------------------------------------------------------------------------------------
def blend(base: int, f: np.float32, v: np.ndarray) -> np.ndarray:
    """ImagingBlend(degenerate = base everywhere, image, f): f32, product and sum rounded separately, truncation"""
    b = np.float32(base)
    r = b + np.float32(f) * (v.astype(np.float32) - b)
    return np.clip(np.trunc(r), 0, 255).astype(np.uint8)


def jitter(u8: np.ndarray, steps) -> np.ndarray:
    for kind, f in steps:
        if kind == "b":
            u8 = blend(0, np.float32(f), u8)
        elif kind == "c":
            total, count = int(u8.astype(np.int64).sum()), u8.size
            u8 = blend((2 * total + count) // (2 * count), np.float32(f), u8)
        else:
            assert kind == "s"  # ImageEnhance.Color on mode "L": the degenerate image is the image
    return u8


def label_lut(mapping) -> np.ndarray:
    lut = np.arange(256, dtype=np.uint8)
    for k, v in (mapping or {}).items():
        lut[k] = v
    return lut


# ---- records, as the kernels take them ------------------------------------------------------------------------------
def records(c: dict):
    ip = np.zeros((len(c["views"]), IP_LEN), dtype=np.int32)
    fp = np.zeros((len(c["views"]), FP_LEN), dtype=np.float64)
    table = pack(c["sources"])[2]
    for i, v in enumerate(c["views"]):
        H, W = c["sources"][v["slice"]][0].shape
        off = int(table[v["slice"], 0])  # the slice's table row travels in the record
        ip[i, [IP["off_lo"], IP["off_hi"], IP["src_h"], IP["src_w"]]] = off & 0x7fffffff, off >> 32, H, W
        assert off < 2 ** 31
        py, px, ch, cw = v["pre"] or (0, 0, H, W)
        ip[i, [IP["slice"], IP["py"], IP["px"], IP["ch"], IP["cw"]]] = v["slice"], py, px, ch, cw
        m = None if v["angle"] is None else rotate_matrix(v["angle"], cw, ch)
        if m is not None:
            ip[i, IP["rot"]] = 1
            ip[i, IP["a0"]:IP["a0"] + 6] = fixed_matrix(m)
            fp[i, FP["m0"]:FP["m0"] + 6] = m
        ip[i, [IP["fv"], IP["fh"], IP["qy"], IP["qx"]]] = int(v["fv"]), int(v["fh"]), v["post"][0], v["post"][1]
        steps = [(k, f) for k, f in v["jitter"] if k != "s"]
        ip[i, IP["njit"]] = len(steps)
        for k, (kind, f) in enumerate(steps):
            ip[i, IP["kind0"] + k] = KIND[kind]
            fp[i, FP["f0"] + k] = np.float32(f)
    return ip, fp


def pack(sources):
    """(image arena, label arena, table [S,3] = offset, H, W)"""
    table, off = [], 0
    for img, _ in sources:
        table.append((off, img.shape[0], img.shape[1]))
        off += img.size
    return (np.concatenate([s[0].reshape(-1) for s in sources]), np.concatenate([s[1].reshape(-1) for s in sources]),
            np.array(table, dtype=np.int64))


def expected(c: dict):
    """(image views uint8 [B,h,w] before the jitter, after it, f32 [B,1,h,w], labels int64 [B,1,h,w])"""
    geo = np.stack([geometry(c["sources"][v["slice"]][0], v, c["out_hw"], False) for v in c["views"]])
    jit = np.stack([jitter(g, v["jitter"]) for g, v in zip(geo, c["views"])])
    lab = np.stack([geometry(c["sources"][v["slice"]][1], v, c["out_hw"], True) for v in c["views"]])
    return geo, jit, TENSOR_LUT[jit][:, None], label_lut(c["mapping"])[lab].astype(np.int64)[:, None]


# ---- the cases ------------------------------------------------------------------------------------------------------
def noise(h: int, w: int, seed: int):
    """(image: smooth ramp plus noise over the whole 0..255 range; label: blocks of 0..3)"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = (rs.randint(0, 256, size=(h, w)) // 2 + (yy * 5 + xx * 3) % 128).astype(np.uint8)
    lab = ((yy // 5 + xx // 7 + rs.randint(0, 2, size=(h, w)) * (rs.uniform(size=(h, w)) < 0.1)) % 4).astype(np.uint8)
    return img, lab


def view(slice=0, pre=None, angle=None, fv=False, fh=False, post=(0, 0), jitter=()):
    return dict(slice=slice, pre=pre, angle=angle, fv=fv, fh=fh, post=post, jitter=list(jitter))


def _case(sources, views, out_hw, mapping=None):
    return dict(sources=sources, views=views, out_hw=out_hw, mapping=mapping)


def _build():
    C = {}
    odd = [noise(37, 45, 1)]
    # rotation + flips + crop (ACDC `pretrain`): every flip combination at both angles, crop origins at both ends
    C["rot_flip_crop_37x45"] = _case(odd, [view(angle=a, fv=fv, fh=fh, post=post)
                                           for a, post in ((13.7, (5, 9)), (-44.9, (13, 0)))
                                           for fv in (False, True) for fh in (False, True)], (24, 32))
    sq = [noise(32, 32, 2)]
    # where Image.rotate takes a transpose shortcut (0, 90, 180, 270 on a square) the kernel takes its general path
    C["square_right_angles"] = _case(sq, [view(angle=a) for a in (0, 90, 180, 270, 45, 360.0, -90)], (32, 32))
    C["angles_37x45"] = _case(odd, [view(angle=a) for a in (0, 30, 45, 90, -7.123456, 180, 270)], (37, 45))
    # crop before the rotation (ACDC `label`)
    C["crop_then_rotate"] = _case(odd, [view(pre=(3, 11, 24, 32), angle=30), view(pre=(13, 13, 24, 32), angle=-30),
                                        view(pre=(0, 0, 24, 32), angle=17.5)], (24, 32))
    small = [noise(24, 24, 3)]
    # pad 20 + crop before the rotation (hippocampus `label`): the window's offsets are negative, the canvas is
    # larger than what it holds of the source, and the bilinear clamps are the canvas's
    C["pad_crop_then_rotate"] = _case(small, [view(pre=(-20, -20, 24, 24), angle=10), view(pre=(-7, 12, 24, 24), angle=-10),
                                              view(pre=(20, 20, 24, 24), angle=5), view(pre=(-3, -2, 24, 24), angle=-3.3)],
                                      (24, 24))
    # rotation, then pad 20 + crop (spleen `label`)
    C["rotate_then_pad_crop"] = _case(odd, [view(angle=10, post=(-20, -20)), view(angle=-10, post=(33, 53)),
                                            view(angle=7, post=(-4, 21), fv=True)], (24, 32))
    C["post_window_outside"] = _case(odd, [view(angle=10, post=(37, 0)), view(post=(0, -32)), view(post=(-24, 45))],
                                     (24, 32))
    C["crop_equals_source"] = _case(odd, [view(pre=(0, 0, 37, 45), angle=21), view(angle=21), view()], (37, 45))
    C["one_by_nine"] = _case([noise(1, 9, 4)], [view(), view(angle=33), view(angle=180), view(fh=True, fv=True),
                                                view(post=(0, -2))], (1, 9))
    # `val`, `trainval`: a centre crop and nothing else; one whose window starts above the source (CenterCrop pads)
    C["no_rotation"] = _case(odd, [view(post=(6, 6)), view(post=(6, 6), fh=True), view(post=(-2, 10))], (24, 24))
    # jitter: all six orders at mixed factors, every factor alone, and the saturation step in its place
    J = {"b": ("b", 1.31), "c": ("c", 0.73), "s": ("s", 1.2)}
    orders = [[J[k] for k in o] for o in ("bcs", "bsc", "cbs", "csb", "sbc", "scb")]
    singles = [[(k, f)] for k in "bc" for f in (0.5, 1.0, 1.5)] + [[("c", 1.5), ("b", 0.5), ("c", 0.5)]]
    C["jitter_orders"] = _case(odd, [view(angle=13.7, post=(5, 9), jitter=j) for j in orders + singles], (24, 32))
    flat = [(np.zeros((16, 16), np.uint8), np.zeros((16, 16), np.uint8)),
            (np.full((16, 16), 255, np.uint8), np.full((16, 16), 3, np.uint8))]
    half = np.zeros((16, 16), np.uint8)
    half[:8], half[8:] = 10, 13  # mean 11.5 exactly: rounds to 12
    flat.append((half, (half // 10).astype(np.uint8)))
    C["jitter_clip_and_half"] = _case(flat, [view(slice=s, jitter=j) for s in range(3)
                                             for j in ([("b", 1.5), ("c", 1.5)], [("c", 0.5), ("b", 1.5)],
                                                       [("c", 1.5)], [("b", 0.5)])], (16, 16))
    C["label_mapping_myo"] = _case(odd, [view(angle=13.7, post=(5, 9)), view(post=(0, 0))], (24, 32), ACDC_MYO)
    # slices of three sizes in one batch, read in an order that is not the store's
    mixed = [noise(37, 45, 5), noise(24, 24, 6), noise(40, 33, 7)]
    C["three_sizes"] = _case(mixed, [view(slice=s, angle=a, post=p, jitter=[("c", 1.2)])
                                     for s, a, p in ((2, 12, (3, 1)), (0, -12, (8, 10)), (1, 40, (-6, -7)),
                                                     (2, None, (16, 9)), (1, 3, (0, 0)))], (24, 24))
    # past the caps of the plan: more than one tile of the geometry grid (GEO_BLOCK pixels) and more than one trip of the
    # jitter block (JIT_BLOCK pixels), neither a multiple; contrast twice, so the block sums over several trips twice
    big = [noise(61, 67, 8)]
    C["past_one_tile"] = _case(big, [view(angle=-20, post=(2, 3), jitter=[("c", 1.4), ("b", 0.9), ("c", 0.6)]),
                                     view(angle=45, fv=True, post=(-1, -1), jitter=[("b", 1.1)])], (57, 61))
    return C


CASES = _build()


@lru_cache(maxsize=None)
def case(name: str):
    """the case with its packed store, records and expected outputs; shared and read-only"""
    c = dict(CASES[name])
    c["arena_img"], c["arena_lab"], c["table"] = pack(c["sources"])
    c["ip"], c["fp"] = records(c)
    c["geo"], c["jit"], c["images"], c["labels"] = expected(c)
    for k in ("arena_img", "arena_lab", "table", "ip", "fp", "geo", "jit", "images", "labels"):
        c[k].setflags(write=False)
    return c


def plan(views: int, out_h: int, out_w: int) -> dict:
    """what cy_aug_plan has to answer"""
    if not 1 <= views <= MAX_VIEWS or not (1 <= out_h <= MAX_OUT and 1 <= out_w <= MAX_OUT):
        return dict(status=ERR_SHAPE)
    hw = out_h * out_w
    return dict(status=OK, form=0, geo_grid_x=-(-hw // GEO_BLOCK), geo_grid_y=views, geo_grid_z=2, jit_grid=views,
                jit_trips=-(-hw // JIT_BLOCK), jit_lds=256 + 1024 + 4 * (JIT_BLOCK // 64), scratch_bytes=views * hw,
                launches=2)
