"""contrastive label generation (semi_seg/hooks/utils.py:22-102 of the reference) and `mixup_data` (284-297)"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from cyhip import ops
from semi_seg.epochers.helper import (ACDCCycleGenerator, PartitionLabelGenerator, PatientLabelGenerator,
                                      SIMCLRGenerator)

_GENERATORS = {"partition": PartitionLabelGenerator, "patient": PatientLabelGenerator, "self": SIMCLRGenerator}
_DATASETS = ("acdc", "prostate", "mmwhs", "spleen", "hippocampus")


def global_label_generator(dataset_name: str, contrast_on: str):
    if dataset_name not in _DATASETS:
        raise NotImplementedError(dataset_name)
    if contrast_on == "cycle":
        if dataset_name != "acdc":
            raise NotImplementedError(contrast_on)
        return ACDCCycleGenerator()
    if contrast_on not in _GENERATORS:
        raise NotImplementedError(contrast_on)
    return _GENERATORS[contrast_on]()


def get_label(contrast_on, data_name, partition_group, label_group):
    """list[int] of length n: equal ints = positive pair (same partition / patient / cycle / self)"""
    if data_name == "acdc" or "acdc" in data_name:
        return global_label_generator("acdc", contrast_on)(
            partition_list=partition_group,
            patient_list=[p.split("_")[0] for p in label_group],
            experiment_list=[p.split("_")[1] for p in label_group])
    if data_name in ("prostate", "prostate_md"):
        return global_label_generator("prostate", contrast_on)(
            partition_list=partition_group, patient_list=[p.split("_")[0] for p in label_group])
    if data_name in ("mmwhsct", "mmwhsmr"):
        return global_label_generator("mmwhs", contrast_on)(partition_list=partition_group, patient_list=label_group)
    if data_name in ("spleen", "hippocampus"):
        return global_label_generator(data_name, contrast_on)(partition_list=partition_group,
                                                              patient_list=label_group)
    raise NotImplementedError(data_name)


def mixup_draw(n: int, alpha: float = 1.0) -> Tuple[float, torch.Tensor]:
    """(lam, index) of one mixing of a batch of n, in the reference's draw order: `np.random.beta(alpha, alpha)` first
    (lam = 1 without a draw for alpha <= 0), then `torch.randperm(n)` on the CPU generator"""
    lam = float(np.random.beta(alpha, alpha)) if alpha > 0 else 1.0
    return lam, torch.randperm(n)


def mixup_data(x, y, *, alpha=1.0, device):
    """-> (lam * x + (1 - lam) * x[index], lam * y + (1 - lam) * y[index]) for one draw of (lam, index).  f32 tensors
    go through cy_mix_images (the bits of the torch expression, without the gathered copy); a `y` of another dtype is
    composed in torch.  The hooks never build a mixed target: they hand labels or teacher logits and the draw to the
    fused losses (cyhip.functions.MixupKLFn, MixSoftmaxMSEFn)."""
    lam, index = mixup_draw(x.shape[0], alpha)
    w_self, w_other = ops.mix_weights(lam)
    idx = ops.mix_index(index, x.shape[0], device)

    def mix(t):
        if t.dtype == torch.float32:
            return ops.mix_images(t, idx, w_self, w_other)
        return lam * t + (1 - lam) * t[idx.long(), :]

    return mix(x), mix(y)
