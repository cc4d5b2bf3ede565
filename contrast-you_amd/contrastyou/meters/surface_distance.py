"""The three surface distances of contrastyou/meters/surface_distance.py:11-31 under the reference's names and
signatures, without `medpy`: border voxels and the exact squared Euclidean distance transform come from the HIP
`cy_surface_stats` kernels (csrc/cy_surface.hip), the square roots, means and percentiles are taken in f64.

`data1`, `data2` are boolean (0 / 1) device tensors of the same 2-D or 3-D shape.  An empty mask raises RuntimeError,
as medpy's `__surface_distances` does.  Each call reads its result back; `SurfaceMeter` keeps the statistics on the
device and uses the `*_from_stats` halves of these functions at read-back.
"""
from __future__ import annotations

import math

import numpy as np
import torch

__all__ = ["hausdorff_distance", "mod_hausdorff_distance", "average_surface_distance"]

_INT32_MAX = 2 ** 31 - 1


def sorted_border_d2(d2: torch.Tensor, border: torch.Tensor) -> torch.Tensor:
    """[2, R, ...] maps -> [2, R, V] int32, each row the d2 of the border voxels in ascending order followed by
    2^31 - 1 for the rest (a fixed-size result: no selection by a mask, so no host sync)"""
    flat = torch.where(border.flatten(2).bool(), d2.flatten(2), torch.full_like(d2.flatten(2), _INT32_MAX))
    return flat.sort(dim=-1).values


def asd_from_stats(count, total) -> float:
    """assd: the mean of the two directed average surface distances; count, total: the two directions"""
    return float(np.mean((total[0] / count[0], total[1] / count[1])))


def hd_from_stats(maxd2) -> float:
    return max(math.sqrt(int(maxd2[0])), math.sqrt(int(maxd2[1])))


def mhd_from_stats(count, sorted_d2, percentile=95) -> float:
    """sorted_d2: [2, V] host int32 rows of `sorted_border_d2`"""
    hd = [np.percentile(np.sqrt(sorted_d2[d, :int(count[d])].astype(np.float64)), percentile) for d in (0, 1)]
    return float(max(hd))


def _stats(data1, data2, voxel_spacing, maps=False):
    if voxel_spacing is not None:
        raise NotImplementedError(f"voxel_spacing={voxel_spacing!r}: voxel spacings are not built (the reference "
                                  "never passes one)")
    from cyhip import ops
    data1, data2 = torch.as_tensor(data1), torch.as_tensor(data2)
    ops.require_gpu(data1, data2)
    out = ops.surface_stats(data1.long(), data2.long(), [1], ndim=data1.dim(), maps=maps)
    count = out[0][:, 0].cpu().numpy()
    if count[0] == 0:
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if count[1] == 0:
        raise RuntimeError("The second supplied array does not contain any binary object.")
    return count, out


def hausdorff_distance(data1, data2, voxel_spacing=None):
    _, out = _stats(data1, data2, voxel_spacing)
    return hd_from_stats(out[2][:, 0].cpu().numpy())


def mod_hausdorff_distance(data1, data2, voxel_spacing=None, percentile=95):
    count, out = _stats(data1, data2, voxel_spacing, maps=True)
    return mhd_from_stats(count, sorted_border_d2(out[3], out[4])[:, 0].cpu().numpy(), percentile)


def average_surface_distance(data1, data2, voxel_spacing=None):
    count, out = _stats(data1, data2, voxel_spacing)
    return asd_from_stats(count, out[1][:, 0].cpu().numpy())
