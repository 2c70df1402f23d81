"""Shapes, inputs and the confidence bound shared by the tests of oess_segment_render and by
tools/exp_segment_render_bounds.py.  Nothing here needs a GPU."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import argmax_labels_reference as ar

# (B, K, h, w), (H, W) or None = same size, align_corners: K31's smallest set with K <= 255
SHAPES = [((1, 1, 1, 1), (1, 1), False),
          ((1, 2, 1, 1), (3, 5), False),
          ((2, 3, 2, 3), None, False),
          ((1, 11, 3, 4), (7, 9), False),
          ((2, 19, 7, 9), (112, 144), False),
          ((2, 11, 5, 6), (13, 17), True),
          ((2, 4, 9, 8), (4, 3), False),          # downsampling
          ((1, 255, 2, 2), (4, 4), False)]
# two source rows of 25 x 255 fp32 = 51 000 bytes: above the kernel's 48 KB LDS budget, the taps come from global memory
GLOBAL_PATH_SHAPE = ((1, 255, 2, 25), (3, 40), False)
ALL_SHAPES = SHAPES + [GLOBAL_PATH_SHAPE]
DTYPES = ("fp32", "bf16")
OUTPUT_SUBSETS = [('labels',), ('conf',), ('rgb',), ('labels', 'conf'), ('labels', 'rgb'), ('conf', 'rgb'), ('labels', 'conf', 'rgb')]
ALPHAS256 = (0, 1, 128, 255, 256)
MIN_CONFS = (0.3, 0.5, 0.9)
EQUAL_K = (1, 2, 4, 11)

# Confidence bound.  tools/exp_segment_render_bounds.py measures torch's own float32 path (F.interpolate in float32, softmax,
# max) against the same in float64 on ALL_SHAPES x DTYPES with the inputs of logits() below: the largest |difference| is
# CONF_FIGURE (printed by the tool; test_segment_render_reference.py holds this constant to what the tool measures).  The bound
# of the kernel's confidence against the float64 restatement is four times that, the convention of K19 - K34.
CONF_FIGURE = 1.9902146775052643e-07          # at 2x4x9x8-4x3-fp32
CONF_BOUND = 4.0 * CONF_FIGURE

case_id = ar.case_id


def out_size(shape, size):
    return tuple(shape[2:]) if size is None else tuple(size)


def logits(shape, dtype, seed_offset=0):
    """float32 CPU logits of a case, already rounded to `dtype`'s grid (the values the kernel sees after widening)"""
    x = ar.randn_logits(shape, seed=sum(shape) + seed_offset)
    return x.to(torch.bfloat16).float() if dtype == "bf16" else x


def palette(K, seed=0):
    """u8 [K, 3] random colours with a 0 and a 255 byte planted in every channel (as far as K allows)"""
    p = torch.randint(0, 256, (K, 3), generator=torch.Generator().manual_seed(100 + seed), dtype=torch.int64)
    p[0, :] = torch.tensor([0, 255, 0])
    p[K - 1, :] = torch.tensor([255, 0, 255]) if K > 1 else p[K - 1, :]
    return p.to(torch.uint8)


def grey(B, H, W, seed=0):
    """u8 [B, H, W] with 0 and 255 present"""
    g = torch.randint(0, 256, (B, H, W), generator=torch.Generator().manual_seed(200 + seed), dtype=torch.int64)
    g.view(-1)[0] = 0
    g.view(-1)[-1] = 255
    return g.to(torch.uint8)


def torch_conf(x, size, align, dtype):
    """softmax(F.interpolate(x)).max(1) of torch on the CPU in `dtype` (torch.float32 / torch.float64): [B, H, W]"""
    v = x.to(dtype)
    if size is not None and tuple(size) != tuple(x.shape[2:]):
        v = F.interpolate(v, size=tuple(size), mode='bilinear', align_corners=align)
    return v.softmax(1).max(1).values


def measure_conf_figure(report=None):
    """largest |torch float32 confidence - torch float64 confidence| over ALL_SHAPES x DTYPES, and where"""
    worst, where = 0.0, None
    for shape, size, align in ALL_SHAPES:
        for dtype in DTYPES:
            x = logits(shape, dtype)
            d = float((torch_conf(x, size, align, torch.float32).double() - torch_conf(x, size, align, torch.float64)).abs().max())
            if report is not None:
                report(f"{case_id(shape, size, align)}-{dtype}", d)
            if d > worst:
                worst, where = d, f"{case_id(shape, size, align)}-{dtype}"
    return worst, where


def special_upsampled_logits():
    """[2, 11, 3, 4] randn with one NaN, one +inf and one -inf planted (K31's non-finite blend case)"""
    x = ar.randn_logits((2, 11, 3, 4), seed=5)
    x[0, 2, 1, 1], x[1, 7, 0, 3], x[1, 4, 2, 0] = float('nan'), float('inf'), float('-inf')
    return x


def finite_pixels(v):
    """bool [B, H, W]: every class value of float32 v [B, K, H, W] is finite"""
    return np.isfinite(v).all(axis=1)
