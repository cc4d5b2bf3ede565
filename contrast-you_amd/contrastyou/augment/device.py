"""Loader-side augmentation described for the device: what a torchvision `Compose` of the reference's `augment_zoo`
(semi_seg/augment.py:36-283) does to a slice and its label, as the per-view records the kernels of
csrc/cy_augment.hip apply (include/contrastyou_hip.h states the record).

Every pipeline of the zoo, once its leading `Resize` is taken out (it draws nothing and is applied when the store is
built), is: [RandomCrop before the rotation] -> [RandomRotation] -> [vertical flip] -> [horizontal flip] ->
[RandomCrop(size, padding) | CenterCrop] for the image (bilinear) and the label (nearest) alike, then ColorJitter and
ToTensor for the image and ToLabel(mapping) for the label.

torchvision is not a dependency and its random stream is not reproduced (as with `AffineAugment`, semi_seg/augment.py):
the same parameter families are drawn from a `numpy.random.RandomState`; what is pinned bit for bit is the
*application* of given parameters (tests/augment_cases.py against Pillow).
"""
from __future__ import annotations

import math
import typing as t

import numpy as np

from cyhip import _lib

IP_LEN, FP_LEN = _lib.CY_AUG_IP_LEN, _lib.CY_AUG_FP_LEN
(IP_SLICE, IP_PY, IP_PX, IP_CH, IP_CW, IP_ROT, IP_FLIPV, IP_FLIPH, IP_QY, IP_QX, IP_NJIT, IP_KIND0, IP_A0) = (
    _lib.CY_AUG_IP_SLICE, _lib.CY_AUG_IP_PY, _lib.CY_AUG_IP_PX, _lib.CY_AUG_IP_CH, _lib.CY_AUG_IP_CW,
    _lib.CY_AUG_IP_ROT, _lib.CY_AUG_IP_FLIPV, _lib.CY_AUG_IP_FLIPH, _lib.CY_AUG_IP_QY, _lib.CY_AUG_IP_QX,
    _lib.CY_AUG_IP_NJIT, _lib.CY_AUG_IP_KIND0, _lib.CY_AUG_IP_A0)
FP_M0, FP_F0 = _lib.CY_AUG_FP_M0, _lib.CY_AUG_FP_F0
BRIGHTNESS, CONTRAST, SATURATION = _lib.CY_AUG_BRIGHTNESS, _lib.CY_AUG_CONTRAST, 3  # saturation never reaches a kernel

_Range = t.Optional[t.Tuple[float, float]]


def rotation_matrix(angle: float, cw: int, ch: int):
    """(m[0..5], a[0..5]) for a canvas of cw x ch, or None where `Image.rotate(angle)` returns a copy: the matrix
    exactly as Image.rotate computes it (angle mod 360, cos and sin of -radians rounded to 15 decimals, centre
    (cw/2, ch/2), translation through the matrix and back) and Pillow's FIX() of it for the nearest path, all in
    Python floats and integers"""
    angle = angle % 360.0
    if angle == 0:
        return None
    cx, cy = cw / 2, ch / 2
    r = -math.radians(angle)
    c, s = math.cos(r), math.sin(r)
    m0, m1, m3 = round(c, 15), round(s, 15), round(-s, 15)
    m4, x, y = m0, -cx, -cy
    m2 = m0 * x + m1 * y + 0.0 + cx
    m5 = m3 * x + m4 * y + 0.0 + cy
    fl = math.floor  # FIX(v) = floor(v * 65536 + 0.5)
    a = [fl(m0 * 65536.0 + 0.5), fl(m1 * 65536.0 + 0.5), fl((m2 + m0 * 0.5 + m1 * 0.5) * 65536.0 + 0.5),
         fl(m3 * 65536.0 + 0.5), fl(m4 * 65536.0 + 0.5), fl((m5 + m3 * 0.5 + m4 * 0.5) * 65536.0 + 0.5)]
    return [m0, m1, m2, m3, m4, m5], a


def center_crop_offset(size: int, target: int) -> int:
    """torchvision's CenterCrop along one axis: the origin of the crop in the source's coordinates; negative where
    the source is the smaller one (it pads (target - size) // 2 in front)"""
    if size < target:
        return -((target - size) // 2)
    return int(round((size - target) / 2.0))


def _pair(v) -> t.Tuple[int, int]:
    return (int(v), int(v)) if isinstance(v, (int, np.integer)) else (int(v[0]), int(v[1]))


class ViewParams(t.NamedTuple):
    int_params: np.ndarray  # int32 [n, IP_LEN]
    f64_params: np.ndarray  # float64 [n, FP_LEN]
    out_hw: t.Tuple[int, int]


class DevicePipeline:
    """One pipeline of the zoo.

    pre_crop      RandomCrop(size) that comes BEFORE the rotation (ACDC and hippocampus `label`)
    rotation      RandomRotation(deg): the angle is U(-deg, deg); None: no rotation
    vflip, hflip  RandomVerticalFlip / RandomHorizontalFlip, p = 0.5 each
    crop          RandomCrop(size) after the rotation and the flips
    padding       the `padding` of `crop`, or of `pre_crop` when there is no `crop`: zeros on every side before the
                  origin is drawn, uniform on the valid integer range
    center_crop   CenterCrop(size), instead of `crop`
    jitter        ColorJitter's (brightness, contrast, saturation) ranges, each (lo, hi) or None; None: no jitter.
                  On 8-bit single-channel slices the saturation step changes no pixel: it takes its place in the
                  drawn order and its factor is drawn, and the kernels are given nothing for it
    mapping       ToLabel(mapping=...): {label value: class}; None: the identity
    total_freedom SequentialWrapperTwice's flag: True, the two views differ in geometry and jitter; False, they share
                  the geometry and differ in the jitter (synchronize.py:141-165)
    presize       the leading Resize of the reference's pipeline, kept for the store to apply once (not used here)

    Without `crop` and `center_crop` the output has the size of the canvas, which then has to be one size per batch.
    """

    def __init__(self, *, pre_crop=None, rotation: t.Optional[float] = None, vflip: bool = False,
                 hflip: bool = False, crop=None, padding: int = 0, center_crop=None,
                 jitter: t.Optional[t.Tuple[_Range, _Range, _Range]] = None,
                 mapping: t.Optional[t.Dict[int, int]] = None, total_freedom: bool = True, presize=None) -> None:
        if crop is not None and center_crop is not None:
            raise ValueError("crop and center_crop are alternatives")
        self.pre_crop = None if pre_crop is None else _pair(pre_crop)
        self.rotation = None if rotation is None else float(rotation)
        self.vflip, self.hflip = bool(vflip), bool(hflip)
        self.crop = None if crop is None else _pair(crop)
        self.padding = int(padding)
        self.center_crop = None if center_crop is None else _pair(center_crop)
        self.jitter = None if jitter is None else tuple(None if r is None else (float(r[0]), float(r[1]))
                                                         for r in jitter)
        self.mapping = None if mapping is None else dict(mapping)
        self.total_freedom = bool(total_freedom)
        self.presize = presize

    # the name the reference's wrapper keeps the flag under: create_tra_test_dataset sets it on a pipeline after taking
    # it from the zoo (semi_seg/data/creator.py:42) and the epochers assert it on the loaders' datasets
    @property
    def _total_freedom(self) -> bool:
        return self.total_freedom

    @_total_freedom.setter
    def _total_freedom(self, value: bool) -> None:
        self.total_freedom = bool(value)

    def __repr__(self) -> str:
        return "DevicePipeline(" + ", ".join(f"{k}={v!r}" for k, v in vars(self).items()) + ")"

    def label_lut(self) -> np.ndarray:
        """uint8 [256]: ToLabel's mapping as a table; values that are no key of the mapping stay as they are (the store
        refuses labels outside the keys when it is built)"""
        lut = np.arange(256, dtype=np.uint8)
        for k, v in (self.mapping or {}).items():
            lut[int(k)] = int(v)
        return lut

    # ---- the draws
    @staticmethod
    def _origin(rs, extent: np.ndarray, target: int, pad: int, what: str) -> np.ndarray:
        """uniform integer in [0, extent + 2 pad - target], minus the padding: the window's origin on the unpadded axis"""
        room = extent + 2 * pad - target
        if (room < 0).any():
            raise ValueError(f"{what}: a crop of {target} does not fit {int(extent.min())} + 2 * {pad} pixels")
        return np.minimum((rs.uniform(size=len(extent)) * (room + 1)).astype(np.int64), room) - pad

    def _geometry(self, rs, n: int, sizes: np.ndarray):
        """(ip, fp, out_hw) with the geometry columns drawn from rs"""
        ip = np.zeros((n, IP_LEN), dtype=np.int32)
        fp = np.zeros((n, FP_LEN), dtype=np.float64)
        pad_pre = self.padding if self.crop is None else 0
        ch, cw = sizes[:, 0].copy(), sizes[:, 1].copy()
        if self.pre_crop is not None:
            ip[:, IP_PY] = self._origin(rs, ch, self.pre_crop[0], pad_pre, "pre_crop")
            ip[:, IP_PX] = self._origin(rs, cw, self.pre_crop[1], pad_pre, "pre_crop")
            ch[:], cw[:] = self.pre_crop
        ip[:, IP_CH], ip[:, IP_CW] = ch, cw
        if self.rotation is not None:
            angles = rs.uniform(-self.rotation, self.rotation, size=n).tolist()
            hits = [rotation_matrix(a, w, h) for a, w, h in zip(angles, cw.tolist(), ch.tolist())]
            rows = [i for i, hit in enumerate(hits) if hit is not None]
            if rows:
                ip[rows, IP_ROT] = 1
                fp[rows, FP_M0:FP_M0 + 6] = [hits[i][0] for i in rows]
                ip[rows, IP_A0:IP_A0 + 6] = [hits[i][1] for i in rows]
        if self.vflip:
            ip[:, IP_FLIPV] = rs.uniform(size=n) < 0.5
        if self.hflip:
            ip[:, IP_FLIPH] = rs.uniform(size=n) < 0.5
        if self.crop is not None:
            ip[:, IP_QY] = self._origin(rs, ch, self.crop[0], self.padding, "crop")
            ip[:, IP_QX] = self._origin(rs, cw, self.crop[1], self.padding, "crop")
            out_hw = self.crop
        elif self.center_crop is not None:
            ip[:, IP_QY] = [center_crop_offset(v, self.center_crop[0]) for v in ch.tolist()]
            ip[:, IP_QX] = [center_crop_offset(v, self.center_crop[1]) for v in cw.tolist()]
            out_hw = self.center_crop
        else:
            if (ch != ch[0]).any() or (cw != cw[0]).any():
                raise ValueError("a pipeline without crop or center_crop keeps the size of its slices: one batch, one size")
            out_hw = (int(ch[0]), int(cw[0]))
        return ip, fp, (int(out_hw[0]), int(out_hw[1]))

    def _jitter(self, rs, ip: np.ndarray, fp: np.ndarray) -> None:
        """the jitter columns of ip and fp, drawn from rs"""
        steps = [(kind, r) for kind, r in zip((BRIGHTNESS, CONTRAST, SATURATION), self.jitter or ()) if r is not None]
        if not steps:
            return
        n = len(ip)
        factors = np.stack([rs.uniform(lo, hi, size=n) for _, (lo, hi) in steps], axis=1)
        order = np.argsort(rs.uniform(size=(n, len(steps))), axis=1)  # a uniform permutation per slice
        kinds = np.array([kind for kind, _ in steps], dtype=np.int32)[order]
        factors = np.take_along_axis(factors, order, axis=1).astype(np.float32)  # ImagingBlend takes a C float
        kept = kinds != SATURATION
        slot = np.cumsum(kept, axis=1) - 1  # where a kept step lands once the saturation step is dropped
        for j in range(len(steps)):
            rows = np.nonzero(kept[:, j])[0]
            ip[rows, IP_KIND0 + slot[rows, j]] = kinds[rows, j]
            fp[rows, FP_F0 + slot[rows, j]] = factors[rows, j]
        ip[:, IP_NJIT] = kept.sum(axis=1)

    @staticmethod
    def _sizes(n: int, source_sizes) -> np.ndarray:
        return np.broadcast_to(np.asarray(source_sizes, dtype=np.int64).reshape(-1, 2), (n, 2))

    def draw(self, n: int, seed: int, source_sizes) -> ViewParams:
        """The records of one view of n slices whose sizes are source_sizes ([n, 2] = H, W; one pair: all alike).  The
        SLICE column is left 0 for the loader to fill.

        One generator, RandomState(seed mod 2^32).  Draw order, each draw a vector over the n slices and made only when
        the pipeline has the step:
          geometry: pre-crop origin y, then x; angle; vertical flip; horizontal flip; crop origin y, then x
          jitter:   the factors, one vector per step in the order brightness, contrast, saturation (a None range is
                    skipped); then uniform(size=(n, steps)), whose argsort along a row is that slice's order
        """
        rs = np.random.RandomState(seed % (2 ** 32))
        ip, fp, out_hw = self._geometry(rs, n, self._sizes(n, source_sizes))
        self._jitter(rs, ip, fp)
        return ViewParams(ip, fp, out_hw)

    def draw_twice(self, n: int, seed: int, source_sizes) -> t.Tuple[ViewParams, ViewParams]:
        """The two views of SequentialWrapperTwice from one RandomState(seed mod 2^32): view 1 as `draw` (so it IS
        draw(n, seed, ...)), then the geometry of view 2 -- drawn with total_freedom, a copy of view 1's without --
        then the jitter of view 2"""
        rs = np.random.RandomState(seed % (2 ** 32))
        sizes = self._sizes(n, source_sizes)
        ip1, fp1, out_hw = self._geometry(rs, n, sizes)
        if self.total_freedom:
            self._jitter(rs, ip1, fp1)
            ip2, fp2, _ = self._geometry(rs, n, sizes)
        else:
            ip2, fp2 = ip1.copy(), fp1.copy()  # before view 1's jitter is written
            self._jitter(rs, ip1, fp1)
        self._jitter(rs, ip2, fp2)
        return ViewParams(ip1, fp1, out_hw), ViewParams(ip2, fp2, out_hw)
