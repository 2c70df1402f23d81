"""Shared by tests/test_event_pre_host.py and tests/test_hip_event_pre.py: the float64 restatement of
EventPreprocessor with hot pixels and flip (e2vid/utils/inference_utils.py:70-87), the torch composition the kernels are compared
with, and the seeded inputs."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "e2vid_hotflip.npz")
SIZES = ("12x20", "13x19")
COMBOS = {"hot": (True, False, False), "flip": (False, True, False), "both": (True, True, False), "both_nonorm": (True, True, True)}


def restate_f64(x, rows, flip, no_normalize):
    """zero -> flip -> normalise in float64 NumPy.  x: [B, C, H, W]; rows: `x,y` pairs or None."""
    e = np.asarray(x, np.float64).copy()
    if rows is not None:
        for px, py in np.asarray(rows).reshape(-1, 2):
            e[:, :, py, px] = 0
    if flip:
        e = e[:, :, ::-1, ::-1]
    if not no_normalize:
        nz = e != 0
        n = nz.sum()
        if n > 0:
            mean = e.sum() / n
            std = np.sqrt((e ** 2).sum() / n - mean ** 2)
            e = nz * (e - mean) / std
    return np.ascontiguousarray(e)


def mask_from_rows(rows, H, W):
    m = np.zeros((H, W), np.uint8)
    for px, py in np.asarray(rows).reshape(-1, 2):
        m[py, px] = 1
    return m


def torch_pre(x, mask, flip, c0=0, cs=None):
    """The hand composition every new entry point is compared with: a zeroed COPY of the slice, then torch.flip."""
    cs = x.shape[1] - c0 if cs is None else cs
    y = x[:, c0:c0 + cs].clone()
    if mask is not None:
        y[:, :, mask.bool()] = 0
    if flip:
        y = torch.flip(y, [2, 3])
    return y.contiguous()


def exact_events(seed, shape, device=None):
    """Multiples of 2^-8 with |v| <= 8, about 70 % zeros: every sum and sum of squares of such values is exact in double in any
    order (|v| 2^8 < 2^11, squares are multiples of 2^-16 below 2^6: 2^22 terms still fit the 53-bit significand)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-2048, 2049, shape, generator=g).float() / 256.0
    v = v * (torch.rand(shape, generator=g) > 0.7).float()
    return v if device is None else v.to(device)


def general_events(seed, shape, device=None):
    g = torch.Generator().manual_seed(seed)
    v = (torch.randn(shape, generator=g) * 1.3 + 0.2) * (torch.rand(shape, generator=g) > 0.6).float()
    return v if device is None else v.to(device)


def hot_mask(H, W, extra=()):
    """Image corners, a duplicate-free scatter and `extra` (y, x) pixels -> uint8 [H, W]."""
    m = torch.zeros((H, W), dtype=torch.uint8)
    for (y, x) in ((0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0), (H // 2, W // 3), (1, 1)) + tuple(extra):
        m[y, x] = 1
    return m
