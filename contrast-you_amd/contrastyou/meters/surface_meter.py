"""`SurfaceMeter` (contrastyou/meters/surface_meter.py:12-130): Hausdorff, 95th-percentile Hausdorff or average symmetric
surface distance per reported class, mean and std over the volumes seen.

`add(pred, target)` enqueues one `cy_surface_stats` per batch entry and keeps the integer / f64 statistics on the
device; they are read back only in `value()` / `summary()`, as `UniversalDice.add_logits` does, so the inference loop
has no per-batch sync.  Each batch entry is one volume.  A volume in which a reported class is absent from the
prediction or from the target has no surface distance: the reference's surface function raises, its epocher ignores
the exception (semi_seg/epochers/epocher.py:203-204) and the volume contributes nothing.  Here such a volume is dropped
whole at read-back and counted in `skipped`.
"""
from __future__ import annotations

import typing as t

import numpy as np
import torch
from torch import Tensor

from ..types import to_float
from ..utils.utils import average_iter
from .metric import Metric
from .surface_distance import (asd_from_stats, average_surface_distance, hausdorff_distance, hd_from_stats,
                               mhd_from_stats, mod_hausdorff_distance, sorted_border_d2)


class SurfaceMeter(Metric):
    meter_choices = {
        "mod_hausdorff": mod_hausdorff_distance,
        "hausdorff": hausdorff_distance,
        "average_surface": average_surface_distance,
    }
    abbr = {"mod_hausdorff": "MHD", "hausdorff": "HD", "average_surface": "ASD"}

    def __init__(self, C=4, report_axises=None, metername: str = "hausdorff") -> None:
        super().__init__()
        assert report_axises is None or isinstance(report_axises, (list, tuple)), \
            f"`report_axises` should be either None or an iterator, given {type(report_axises)}"
        if report_axises is not None:
            assert max(report_axises) <= C, f"Incompatible parameter of `C`={C} and `report_axises`={report_axises}"
        self._C = C
        self._report_axis = list(range(self._C))
        if report_axises is not None:
            self._report_axis = report_axises
        assert metername in self.meter_choices.keys()
        self._surface_name = metername
        self._abbr = self.abbr[metername]
        self._surface_function = self.meter_choices[metername]
        self.reset()

    def reset(self):
        self._mhd: t.List[np.ndarray] = []
        self._pending: t.List[tuple] = []
        self._n = 0
        self.skipped = 0

    @torch.no_grad()
    def _add(self, pred: Tensor, target: Tensor, voxelspacing: t.Union[t.List[float], float] = None):
        """pred, target: class-coded [B, *spatial] tensors, or a simplex prediction [B, C, *spatial] with a one-hot
        target; spatial rank 2 or 3.  Nothing is read back here."""
        if voxelspacing is not None:
            raise NotImplementedError(f"voxelspacing={voxelspacing!r}: voxel spacings are not built (the reference "
                                      "never passes one)")
        from cyhip import ops
        ops.require_gpu(pred, target)
        assert pred.shape == target.shape, \
            f"incompatible shape of `pred` and `target`, given {pred.shape} and {target.shape}."
        assert not pred.requires_grad and not target.requires_grad
        if pred.is_floating_point():  # simplex prediction, one-hot target
            pred, target = pred.argmax(1), target.argmax(1)
        ndim = pred.dim() - 1
        assert ndim in (2, 3), f"volumes are [B, H, W] or [B, D, H, W], given {tuple(pred.shape)}"
        pred, target = pred.long(), target.long()
        want_maps = self._surface_name == "mod_hausdorff"
        for p, g in zip(pred, target):
            out = ops.surface_stats(p, g, self._report_axis, ndim=ndim, maps=want_maps)
            self._pending.append(tuple(out[:3]) + ((sorted_border_d2(out[3], out[4]),) if want_maps else ()))
        self._n += 1

    def _flush(self):
        for stats in self._pending:
            count, total, maxd2 = (s.cpu().numpy() for s in stats[:3])
            if (count == 0).any():
                self.skipped += 1
                continue
            R = len(self._report_axis)
            if self._surface_name == "average_surface":
                row = [asd_from_stats(count[:, r], total[:, r]) for r in range(R)]
            elif self._surface_name == "hausdorff":
                row = [hd_from_stats(maxd2[:, r]) for r in range(R)]
            else:
                ordered = stats[3].cpu().numpy()
                row = [mhd_from_stats(count[:, r], ordered[:, r]) for r in range(R)]
            self._mhd.append(np.asarray(row, dtype=np.float64)[None])
        self._pending = []

    def value(self, **kwargs):
        self._flush()
        if len(self._mhd) == 0:
            return ([np.nan] * self._C, [np.nan] * self._C)
        mhd = np.concatenate(self._mhd, axis=0)
        return (mhd.mean(0), mhd.std(0))

    def _summary(self) -> dict:
        means, stds = self.value()
        result = {f"{self._abbr}{i}": to_float(means[num]) for num, i in enumerate(self._report_axis)}
        result.update({f"{self._abbr}_mean": average_iter(result.values())})
        return result

    def detailed_summary(self) -> dict:
        means, stds = self.value()
        return {**{f"{self._abbr}{i}": to_float(means[num]) for num, i in enumerate(self._report_axis)},
                **{f"{self._abbr}{i}": to_float(stds[num]) for num, i in enumerate(self._report_axis)}}

    def __repr__(self):
        string = f"C={self._C}, report_axis={self._report_axis}\n"
        return string + "\t" + "\t".join([f"{k}:{v}" for k, v in self.summary().items()])
