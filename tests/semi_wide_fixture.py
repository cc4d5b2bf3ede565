"""Encoding and layout of tests/golden/semi_wide.npz, shared by its generator (tests/golden/gen_goldens_semi_wide.py) and
its readers (tests/test_gpu_wide_reg.py): the cases of tests/semi_fixture.py on multi-prototype logits, 16 < K <= 64,
and the ICT loss next to them.  Logits lie on a 1/8 grid in [-6, 6] and are stored as int8 = 8 * logit (`_i8d8`)."""
import numpy as np
import torch

from semi_fixture import StoredTeacher, decode  # noqa: F401  (re-exported: the readers take them from here)

# 17: one channel in the fifth lane; 20: 5 classes x 4 prototypes, 16-byte rows; 40; 63: the last lane three-quarters
# full, rows of no 16-byte multiple; 64: the full row
KS = (17, 20, 40, 63, 64)
SHAPE = (2, 13, 11)         # N, H, W: 286 pixels = 17 full 16-pixel groups and a group of 14
ZERO_ROWS = 3               # rows h < 3 are all-zero logits in teacher and student (what the warp pads with)
TEACHERS = 5                # one tracked forward + N = 4 noisy ones
MAX_EPOCH = 10
EPOCHS = (0, 4)             # cur_epoch / max_epoch = 0, 0.4
TIE_PIXEL = (1, 5, 2)       # n, h, w of a row whose maximum is tied between two lanes, in the student and every teacher
ICT_INDEX = (1, 0)          # image n is mixed with image ICT_INDEX[n]
ICT_LAM = 0.3125            # exact in f32: w_self = 0.3125, w_other = 0.6875


def tie_channels(K: int):
    """the two channels of the tied maximum at TIE_PIXEL: lane 1 and the last lane that holds a channel"""
    return 5, K - 1


def uamt_cases():
    """(key prefix, K, cur_epoch, hard_clip) of every UA-MT case"""
    return [(f"uamt_K{K}_e{ep}_h{int(hard)}", K, ep, hard) for K in KS for ep in EPOCHS for hard in (False, True)]


def cross_lane_ties(z: torch.Tensor) -> torch.Tensor:
    """[N, H, W] bool: the rows of [N, K, H, W] logits whose maximum is taken in two different 4-channel lanes"""
    top = z == z.max(1, keepdim=True)[0]
    lanes = torch.arange(z.shape[1]).div(4, rounding_mode="floor").view(1, -1, 1, 1).expand_as(z)
    big = torch.iinfo(torch.int64).max
    lo = torch.where(top, lanes, torch.full_like(lanes, big)).min(1)[0]
    hi = torch.where(top, lanes, torch.full_like(lanes, -1)).max(1)[0]
    return lo != hi


def load(golden_dir):
    return np.load(golden_dir / "semi_wide.npz")
