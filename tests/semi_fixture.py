"""Encoding and layout of tests/golden/semi_baselines.npz, shared by its generator (tests/golden/gen_goldens_semi.py)
and its readers (tests/test_gpu_semi_baselines.py).  Logits lie on a 1/8 grid in [-6, 6] and are stored as
int8 = 8 * logit (suffix `_i8d8`, as the `_i8d4` / `_i8d32` entries of cc_fixture): exact in f32 and in f64."""
import numpy as np
import torch

KS = (2, 4, 5, 16)          # class counts of the fixture
SHAPE = (2, 13, 11)         # N, H, W: 286 pixels = one full block of 256 plus a tail
ZERO_ROWS = 3               # rows h < 3 are all-zero logits in teacher and student (what the warp pads with)
TEACHERS = 5                # one tracked forward + N = 4 noisy ones
MAX_EPOCH = 10
EPOCHS = (0, 4)             # cur_epoch / max_epoch = 0, 0.4
EXTRA = ("x", 4, 10)        # tag, K, cur_epoch of the extra case at ratio 1, without zero rows


def decode(name: str, arr: np.ndarray) -> torch.Tensor:
    assert name.endswith("_i8d8"), name
    return torch.from_numpy(np.asarray(arr)).float() / 8.0


def uamt_cases():
    """(key prefix, input tag, K, cur_epoch, hard_clip) of every UA-MT case"""
    out = [(f"uamt_K{K}_e{ep}_h{int(hard)}", f"K{K}", K, ep, hard)
           for K in KS for ep in EPOCHS for hard in (False, True)]
    tag, K, ep = EXTRA
    return out + [(f"uamt_{tag}_h{int(hard)}", tag, K, ep, hard) for hard in (False, True)]


class StoredTeacher(torch.nn.Module):
    """a teacher that returns stored logit tensors in turn, whatever it is fed, with a no-op `switch_bn_track`"""

    def __init__(self, logits):
        super().__init__()
        self.logits, self.calls = list(logits), 0

    def forward(self, x):
        out = self.logits[self.calls % len(self.logits)]
        self.calls += 1
        return out

    def switch_bn_track(self, **kwargs):
        from contextlib import nullcontext
        return nullcontext(self)
