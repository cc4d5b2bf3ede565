"""Superpixel maps on the device, for the superpixel InfoNCE hook.

The reference makes them offline with scikit-image (`script/create_superpixel.py:27`:
`slic(img, n_segments=40, sigma=5, compactness=0.1)`) and loads them from a `superpixel/` folder next to the images
(`_load_superpixel_image`, semi_seg/hooks/infonce.py:24-27).  Here they come from the images of the batch through the
SLIC kernels of csrc/cy_slic.hip (DESIGN.md "On-device superpixels" states the algorithm and where it departs from
scikit-image).
"""
from __future__ import annotations

import typing as t

from torch import Tensor

from cyhip import ops

# script/create_superpixel.py:27
REFERENCE_PARAMS = {"n_segments": 40, "sigma": 5.0, "compactness": 0.1}


def slic_superpixels(images: Tensor, **params) -> Tensor:
    """ids uint8 [N,H,W] of single-channel images in 0..1 ([N,1,H,W] or [N,H,W]); keywords as `cyhip.ops.slic`
    (n_segments, sigma, compactness, max_iter), the reference's values by default"""
    return ops.slic(images, **{**REFERENCE_PARAMS, **params})[0]


def as_batch_entry(ids: Tensor) -> t.List[Tensor]:
    """the form the reference's loader gives a superpixel map (an 8-bit image through ToTensor: id / 255, one channel,
    in a list) -- what `_SuperPixelInfoNCEEPochHook` reads under batch_data["superpixel"]"""
    return [ids.float().div(255).unsqueeze(1)]
