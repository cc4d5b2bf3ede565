#!/usr/bin/env python3
"""Generate tests/golden/augment.npz: Pillow itself run on the cases of tests/augment_cases.py.

    python tests/golden/gen_goldens_augment.py

Needs Pillow.  Per view Pillow is driven the way torchvision's transforms drive it: `ImageOps.expand(border, fill=0)`
and `crop` for a window (a crop, or a pad followed by a crop), `Image.rotate(angle, BILINEAR)` for the image and
`NEAREST` for the label, `transpose` for the flips, `ImageEnhance.Brightness / Contrast / Color` in the view's order, then
`np.array`.  `pillow_case` is also what tests/test_augment_host.py runs live against the NumPy restatement.

The file holds, per case `<name>`: <name>_src<i>_img / _lab (the uint8 sources), <name>_ip / _fp (the records the
kernels take), <name>_out_hw, <name>_geo (image views before the jitter), <name>_jit (after it), <name>_lab (label
views before ToLabel's mapping), all uint8; and `pillow_version`.
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import augment_cases as ac  # noqa: E402

OUT = Path(__file__).resolve().parent / "augment.npz"


def pil_window(im, oy: int, ox: int, h: int, w: int):
    """pixel (y, x) of the result is pixel (y + oy, x + ox) of im, 0 outside: pad as much as the window needs, crop"""
    from PIL import ImageOps
    W, H = im.size
    border = max(0, -oy, -ox, oy + h - H, ox + w - W)
    if border:
        im = ImageOps.expand(im, border=border, fill=0)
    return im.crop((ox + border, oy + border, ox + border + w, oy + border + h))


def pil_geometry(src: np.ndarray, view: dict, out_hw, label: bool):
    from PIL import Image
    im = Image.fromarray(src)
    assert im.mode == "L"
    if view["pre"] is not None:
        im = pil_window(im, *view["pre"])
    if view["angle"] is not None:
        im = im.rotate(view["angle"], Image.NEAREST if label else Image.BILINEAR)
    if view["fv"]:
        im = im.transpose(Image.FLIP_TOP_BOTTOM)
    if view["fh"]:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return pil_window(im, view["post"][0], view["post"][1], out_hw[0], out_hw[1])


def pil_jitter(im, steps):
    from PIL import ImageEnhance
    enhance = {"b": ImageEnhance.Brightness, "c": ImageEnhance.Contrast, "s": ImageEnhance.Color}
    for kind, f in steps:
        im = enhance[kind](im).enhance(f)
    return im


def pillow_case(c: dict):
    """(geo, jit, lab) uint8 [B,h,w] of a case, from Pillow"""
    geo, jit, lab = [], [], []
    for v in c["views"]:
        img, gt = c["sources"][v["slice"]]
        g = pil_geometry(img, v, c["out_hw"], False)
        geo.append(np.array(g))
        jit.append(np.array(pil_jitter(g, v["jitter"])))
        lab.append(np.array(pil_geometry(gt, v, c["out_hw"], True)))
    return np.stack(geo), np.stack(jit), np.stack(lab)


def main():
    import PIL
    out = {"pillow_version": np.array(PIL.__version__)}
    for name, c in ac.CASES.items():
        for i, (img, lab) in enumerate(c["sources"]):
            out[f"{name}_src{i}_img"], out[f"{name}_src{i}_lab"] = img, lab
        out[f"{name}_ip"], out[f"{name}_fp"] = ac.records(c)
        out[f"{name}_out_hw"] = np.array(c["out_hw"], dtype=np.int32)
        out[f"{name}_geo"], out[f"{name}_jit"], out[f"{name}_lab"] = pillow_case(c)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {OUT.stat().st_size} bytes, {len(ac.CASES)} cases, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
