"""Encodings of tests/golden/cc.npz, shared by its generator (tests/golden/gen_goldens_cc.py) and its reader
(tests/test_gpu_cc.py).  Inputs are stored quantised -- images as uint8 / 255, maps as uint16 / 65535, logits and
features as int8 / scale: exact in f32 and a fraction of the size."""
import numpy as np
import torch


def decode(name: str, arr: np.ndarray) -> torch.Tensor:
    """the f32 tensor a quantised fixture entry stands for (suffix of the entry's name = its encoding)"""
    t = torch.from_numpy(np.asarray(arr))
    if name.endswith("_u8"):
        return t.float() / 255.0
    if name.endswith("_u16"):
        return (t.to(torch.int32).float()) / 65535.0
    if name.endswith("_i8d4"):
        return t.float() / 4.0
    if name.endswith("_i8d32"):
        return t.float() / 32.0
    raise KeyError(name)


def softmax_f32(logits: torch.Tensor) -> torch.Tensor:
    """probabilities of decoded logits: softmax in f64, rounded to f32 (what both sides of a comparison are fed)"""
    return logits.double().softmax(1).float()
