"""A dataset's slices resident on the device, and a loader that cuts augmented batches from them.

The reference reads 8-bit slices from a folder (contrastyou/data/dataset/base.py), transforms each sample with Pillow
and torchvision on host workers (contrastyou/augment/synchronize.py) and collates them.  The datasets are small (ACDC is
a few thousand slices): `DeviceSliceStore` keeps all of them as uint8 in device memory and `DeviceLoader` produces the
batch dictionary the epochers unpack with two kernel launches per batch and no host worker.  Decoding image files, the
dataset folder classes and the samplers are not part of this: the store is built from arrays and the loader takes any
iterable of index lists.
"""
from __future__ import annotations

import re
import sys
import typing as t

import numpy as np
import torch

from contrastyou.augment.device import IP_SLICE, DevicePipeline
from cyhip import ops


def batch_seed(seed: int, rank: int, batch: int) -> int:
    """the 32-bit seed of one batch's draws: a hash of (seed, rank, batch) through numpy's SeedSequence, so that no
    rank's stream of batches is another rank's stream shifted, however long an infinite sampler runs"""
    words = [int(seed) % (2 ** 64), int(rank), int(batch)]
    return int(np.random.SeedSequence(words).generate_state(1)[0])


def presize_hw(h: int, w: int, presize) -> t.Tuple[int, int]:
    """torchvision's Resize: an int sets the smaller edge and the other becomes int(size * long / short); a pair is
    (h, w)"""
    if isinstance(presize, (int, np.integer)):
        size = int(presize)
        if h <= w:
            return size, int(size * w / h)
        return int(size * h / w), size
    return int(presize[0]), int(presize[1])


def _resize(images, labels, presize):
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("DeviceSliceStore.from_arrays(presize=...) resizes the slices with Pillow (the PIL package), "
                          "which is not installed") from e
    out_i, out_l = [], []
    for img, lab in zip(images, labels):
        h, w = presize_hw(img.shape[0], img.shape[1], presize)
        out_i.append(np.array(Image.fromarray(img).resize((w, h), Image.BILINEAR)))
        out_l.append(np.array(Image.fromarray(lab).resize((w, h), Image.NEAREST)))
    return out_i, out_l


class DeviceSliceStore:
    """two uint8 arenas (images, labels) on the device and the int64 table [S, 3] = (byte offset, H, W) both share,
    kept on the host (the records of a batch carry the rows they need);
    `filenames`, `partitions` and `scan_nums` are host lists, one entry per slice"""

    def __init__(self, images: torch.Tensor, labels: torch.Tensor, table: torch.Tensor, filenames: t.List[str],
                 partitions: t.List, scan_nums: t.List[str]) -> None:
        self.images, self.labels, self.table = images, labels, table
        self.filenames, self.partitions, self.scan_nums = filenames, partitions, scan_nums

    def __len__(self) -> int:
        return self.table.shape[0]

    @property
    def device(self):
        return self.images.device

    def sizes(self, indices) -> np.ndarray:
        return self.table[:, 1:].numpy()[np.asarray(indices, dtype=np.int64)]

    @classmethod
    def from_arrays(cls, images: t.Sequence[np.ndarray], labels: t.Sequence[np.ndarray], filenames: t.Sequence[str], *,
                    group_re: str, partitions: t.Optional[t.Sequence] = None, presize=None,
                    mapping: t.Optional[t.Dict[int, int]] = None, device="cuda") -> "DeviceSliceStore":
        """images, labels: uint8 [H, W] arrays of any sizes, a label for every image and of its size.  `group_re` is
        searched in each filename for the scan's name, as the reference's datasets do; `partitions` defaults to 0 for
        every slice.  `presize`: the pipelines' leading Resize (`ZooEntry.presize`), applied here once with Pillow,
        images bilinear and labels nearest.  `mapping`: the ToLabel mapping the labels will go through; a label value
        that is not one of its keys is refused here (the reference would raise a KeyError for the sample)."""
        if not (len(images) == len(labels) == len(filenames)) or len(images) == 0:
            raise ValueError("one label and one filename per image, and at least one slice")
        for img, lab in zip(images, labels):
            if img.dtype != np.uint8 or lab.dtype != np.uint8 or img.ndim != 2 or img.shape != lab.shape:
                raise ValueError(f"slices are uint8 [H, W] arrays, image and label of one size; given {img.dtype} "
                                 f"{img.shape} and {lab.dtype} {lab.shape}")
        if presize is not None:
            images, labels = _resize(images, labels, presize)
        if mapping is not None:
            seen = sorted(set().union(*(np.unique(lab).tolist() for lab in labels)))
            if not set(seen) <= set(mapping):
                raise KeyError(f"label values {sorted(set(seen) - set(mapping))} are not keys of the mapping {mapping}")
        pattern = re.compile(group_re)
        scans = []
        for f in filenames:
            m = pattern.search(f)
            if m is None:
                raise AttributeError(f"Cannot match pattern: {group_re} for {f}")
            scans.append(m.group(0))
        table = np.zeros((len(images), 3), dtype=np.int64)
        off = 0
        for i, img in enumerate(images):
            h, w = img.shape
            if not (1 <= h <= ops.AUG_MAX_SIDE and 1 <= w <= ops.AUG_MAX_SIDE):
                raise ValueError(f"slice {filenames[i]} is {h} x {w}: sides are 1..{ops.AUG_MAX_SIDE}")
            table[i] = (off, h, w)
            off += h * w
        arena_i = np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in images])
        arena_l = np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in labels])
        parts = [0] * len(images) if partitions is None else list(partitions)
        if len(parts) != len(images):
            raise ValueError("one partition per slice")
        return cls(torch.from_numpy(arena_i).to(device), torch.from_numpy(arena_l).to(device),
                   torch.from_numpy(table), list(filenames), parts, scans)


class _Dataset:
    """what the epochers look for behind a loader: `loader.dataset.transforms._total_freedom`"""

    def __init__(self, store: DeviceSliceStore, transforms: DevicePipeline) -> None:
        self.store, self.transforms = store, transforms

    def __len__(self) -> int:
        return len(self.store)


class DeviceLoader:
    """Iterates `indices` (any iterable of lists of slice indices: a batch sampler, finite or not) and yields, per list,
    the batch the reference's collate gives -- twice: {"img": [v1, v2], "gt": [t1, t2], "filename": [f, f], "partition":
    [p, p], "scan_num": [s, s]} for `preprocess_input_with_twice_transformation`; otherwise the same keys holding one
    view each.  img is f32 [B,1,h,w] in 0..1 and gt int64 [B,1,h,w], both on the store's device; the rest are host
    lists.  Nothing waits for the device: a batch is queued on the current stream and returned.

    Batch b of an iteration is drawn from `batch_seed(seed, rank, b)`: every iteration over the loader repeats the
    same draws, ranks differ, and the stream of views depends on nothing but (seed, rank, indices)."""

    def __init__(self, store: DeviceSliceStore, pipeline: DevicePipeline, indices: t.Iterable[t.Sequence[int]], *,
                 twice: bool = True, seed: int = 0, rank: int = 0) -> None:
        self.store, self.pipeline, self.indices, self.twice = store, pipeline, indices, bool(twice)
        self.seed, self.rank = int(seed), int(rank)
        self.dataset = _Dataset(store, pipeline)
        self._label_lut = torch.from_numpy(pipeline.label_lut()).to(store.device)

    def __len__(self) -> int:
        return len(self.indices) if hasattr(self.indices, "__len__") else sys.maxsize

    def _views(self, params, idx):
        """the views of one batch in one call (two launches): params is a list of ViewParams over the same slices"""
        ip = np.concatenate([p.int_params for p in params])
        ip[:, IP_SLICE] = list(idx) * len(params)
        fp = np.concatenate([p.f64_params for p in params])
        img, gt = ops.augment_views(self.store.images, self.store.labels, self.store.table, torch.from_numpy(ip),
                                    torch.from_numpy(fp), self._label_lut, params[0].out_hw)
        n = len(idx)
        return [(img[k * n:(k + 1) * n], gt[k * n:(k + 1) * n]) for k in range(len(params))]

    def __iter__(self):
        store = self.store
        for b, idx in enumerate(self.indices):
            idx = [int(i) for i in idx]
            if not idx or min(idx) < 0 or max(idx) >= len(store):
                raise IndexError(f"batch {b}: indices outside the store of {len(store)} slices")
            seed = batch_seed(self.seed, self.rank, b)
            sizes = store.sizes(idx)
            meta = {"filename": [store.filenames[i] for i in idx], "partition": [store.partitions[i] for i in idx],
                    "scan_num": [store.scan_nums[i] for i in idx]}
            if self.twice:
                views = self._views(list(self.pipeline.draw_twice(len(idx), seed, sizes)), idx)
                yield {"img": [v[0] for v in views], "gt": [v[1] for v in views],
                       **{k: [v, list(v)] for k, v in meta.items()}}
            else:
                (img, gt), = self._views([self.pipeline.draw(len(idx), seed, sizes)], idx)
                yield {"img": img, "gt": gt, **meta}
