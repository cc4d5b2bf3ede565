#!/usr/bin/env python3
"""Generate tests/golden/surface.npz: the REFERENCE's SurfaceMeter (contrastyou/meters/surface_meter.py) and its three
surface functions (surface_distance.py) evaluated on seeded blob label volumes.

    python tests/golden/gen_goldens_surface.py

Needs the reference checkout (see gen_goldens.py) and scipy; nothing of the reference is copied into the repository,
only label volumes and numbers.  The reference imports `medpy.metric`, which is not installed: the stand-in written
below implements the two functions the reference calls (`assd`, `__surface_distances` with voxelspacing None) over
scipy.ndimage -- face-neighbour erosion with background outside the array, exact Euclidean distance transform.

Per case `<tag>`:
    <tag>_pred, <tag>_target   uint8 [B, *spatial] label volumes, 4 classes (spatial rank 2: the 2-D form)
    <tag>_asd/_hd/_mhd         f64 [B, 3]: the reference's value per (volume, class 1..3), NaN where it raises
    <tag>_sum_asd/_hd/_mhd     f64 [4]: summary() of a SurfaceMeter(C=4, report_axises=[1, 2, 3]) fed every volume of the
                               case under the epocher's ignore_exception() -- (class 1, 2, 3, mean); NaN when empty
    <tag>_skipped              uint8 [B]: 1 where that add raised (a reported class empty on either side)
    <tag>_d2, <tag>_border     small cases only, volume 0: int32 / uint8 [2, 3, *spatial] -- direction 0 is pred ->
                               target: border[0] the prediction's border voxels, d2[0] the squared distance to the
                               target's nearest border voxel; direction 1 the other way round.  Where the other side
                               has no border voxel the distance is undefined and the map holds 2^30, the kernels' value.
"""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import gen_goldens as gg  # noqa: E402

OUT = Path(__file__).resolve().parent / "surface.npz"
NO_BORDER = 1 << 30

gg.STUBS = dict(gg.STUBS)
gg.STUBS["medpy/metric/__init__.py"] = "from .binary import asd, assd\n"
gg.STUBS["medpy/metric/binary.py"] = (
    "import numpy\n"
    "from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure\n"
    "def __surface_distances(result, reference, voxelspacing=None, connectivity=1):\n"
    "    assert voxelspacing is None\n"
    "    result = numpy.atleast_1d(numpy.asarray(result).astype(bool))\n"
    "    reference = numpy.atleast_1d(numpy.asarray(reference).astype(bool))\n"
    "    footprint = generate_binary_structure(result.ndim, connectivity)\n"
    "    if 0 == numpy.count_nonzero(result):\n"
    "        raise RuntimeError('The first supplied array does not contain any binary object.')\n"
    "    if 0 == numpy.count_nonzero(reference):\n"
    "        raise RuntimeError('The second supplied array does not contain any binary object.')\n"
    "    result_border = result ^ binary_erosion(result, structure=footprint, iterations=1)\n"
    "    reference_border = reference ^ binary_erosion(reference, structure=footprint, iterations=1)\n"
    "    return distance_transform_edt(~reference_border)[result_border]\n"
    "def asd(result, reference, voxelspacing=None, connectivity=1):\n"
    "    return __surface_distances(result, reference, voxelspacing, connectivity).mean()\n"
    "def assd(result, reference, voxelspacing=None, connectivity=1):\n"
    "    return numpy.mean((asd(result, reference, voxelspacing, connectivity),\n"
    "                       asd(reference, result, voxelspacing, connectivity)))\n")

# (tag, spatial shape, seeds of the volumes' (pred, target), maps stored)
CASES = [
    ("d1", (1, 9, 13), [(1, 2)], True),        # depth 1 as 3-D: every object voxel is border
    ("flat", (9, 13), [(1, 2)], True),         # the same labels as 2-D
    ("line1", (2, 1, 5), [(1, 2)], True),      # a line of length 1, empty classes
    ("hlong", (3, 67, 5), [(1, 2)], True),     # H line longer than a wavefront
    ("wlong", (5, 33, 70), [(1, 2)], True),    # W line longer than a wavefront
    ("h130", (4, 130, 3), [(1, 2)], True),
    ("h257", (2, 257, 3), [(1, 2)], True),     # a line longer than a 256-thread block
    ("pair", (3, 20, 24), [(5, 6), (5, 6)], False),  # a batch of two; class 2 is wiped from the second prediction
    ("large", (5, 230, 230), [(3, 4)], False),  # 264 500 voxels: more than 1024 blocks of 256, scalars only
]


def blobs(shape, C, seed):
    g = np.random.default_rng(seed)
    lab = np.zeros(shape, np.uint8)
    grids = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    for c in range(1, C):
        for _ in range(2):
            ctr = [g.uniform(0, s) for s in shape]
            rad = [max(1.0, g.uniform(0.15, 0.45) * s) for s in shape]
            lab[sum(((x - c0) / r) ** 2 for x, c0, r in zip(grids, ctr, rad)) <= 1] = c
    return lab


def maps_of(pred, target):
    from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure
    fp = generate_binary_structure(pred.ndim, 1)
    d2 = np.full((2, 3) + pred.shape, NO_BORDER, np.int32)
    border = np.zeros((2, 3) + pred.shape, np.uint8)
    for r, c in enumerate((1, 2, 3)):
        sides = [pred == c, target == c]
        edges = [m ^ binary_erosion(m, structure=fp, iterations=1) for m in sides]
        for d in (0, 1):
            border[d, r] = edges[d]
            if edges[1 - d].any():
                dist = distance_transform_edt(~edges[1 - d])
                d2[d, r] = np.rint(dist ** 2).astype(np.int32)
                assert np.array_equal(np.sqrt(d2[d, r].astype(np.float64)), dist)
    return d2, border


def main():
    scratch = gg.setup_reference()
    from contrastyou.meters.surface_meter import SurfaceMeter

    names = {"asd": "average_surface", "hd": "hausdorff", "mhd": "mod_hausdorff"}
    out = {}
    for tag, shape, seeds, with_maps in CASES:
        if tag == "flat":
            pred, target = out["d1_pred"][:, 0], out["d1_target"][:, 0]
        else:
            pred = np.stack([blobs(shape, 4, a) for a, _ in seeds])
            target = np.stack([blobs(shape, 4, b) for _, b in seeds])
        if tag == "pair":
            assert all((v == c).any() for v in (pred[0], target[0]) for c in (1, 2, 3)), "pair: a class is empty"
            pred[1][pred[1] == 2] = 0
        out[f"{tag}_pred"], out[f"{tag}_target"] = pred, target
        tp, tt = torch.from_numpy(pred).long(), torch.from_numpy(target).long()
        B = len(pred)
        for key, metername in names.items():
            per = np.full((B, 3), np.nan)
            for b in range(B):
                for r, c in enumerate((1, 2, 3)):
                    m = SurfaceMeter(C=4, report_axises=[c], metername=metername)
                    try:
                        m.add(tp[b:b + 1], tt[b:b + 1])
                        per[b, r] = m.value()[0][0]
                    except RuntimeError:
                        pass
            out[f"{tag}_{key}"] = per
            whole = SurfaceMeter(C=4, report_axises=[1, 2, 3], metername=metername)
            skipped = np.zeros(B, np.uint8)
            for b in range(B):
                try:
                    whole.add(tp[b:b + 1], tt[b:b + 1])
                except RuntimeError:
                    skipped[b] = 1
            assert np.array_equal(skipped, np.isnan(per).any(1))
            s = whole.summary()
            ab = SurfaceMeter.abbr[metername]
            out[f"{tag}_sum_{key}"] = np.array([s[f"{ab}1"], s[f"{ab}2"], s[f"{ab}3"], s[f"{ab}_mean"]], np.float64)
            out[f"{tag}_skipped"] = skipped
        if with_maps:
            out[f"{tag}_d2"], out[f"{tag}_border"] = maps_of(pred[0], target[0])
        print(tag, shape, "skipped", out[f"{tag}_skipped"].tolist(), "ASD", out[f"{tag}_asd"].tolist())
    assert out["pair_skipped"].tolist() == [0, 1]
    assert sum(int(out[f"{t}_skipped"].sum()) for t, *_ in CASES) >= 2
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {OUT.stat().st_size} bytes")
    del scratch


if __name__ == "__main__":
    main()
