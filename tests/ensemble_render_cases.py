"""Cases, inputs and the confidence bound shared by the tests of oess_segment_render_ensemble and by
tools/exp_ensemble_render_bounds.py.  Nothing here needs a GPU."""
import numpy as np
import torch

from tests import argmax_labels_reference as ar
from tests import ensemble_render_reference as er
from tests import segment_render_cases as sc

# (B, K), [(h, w, flip) per view], (H, W) or None = view 0's size, align_corners
CASES = [((1, 1), [(1, 1, 0)], (1, 1), False),
         ((1, 2), [(1, 1, 0), (1, 1, 1)], (3, 5), False),
         ((2, 3), [(2, 3, 0), (2, 3, 1)], None, False),                                        # all raw
         ((1, 11), [(3, 4, 0), (3, 4, 1), (5, 6, 0)], (7, 9), False),                          # odd V
         ((2, 19), [(7, 9, 0), (7, 9, 1), (5, 7, 0), (5, 7, 1), (9, 12, 0), (9, 12, 1)], (56, 72), False),
         ((2, 11), [(5, 6, 0), (5, 6, 1)], (13, 17), True),
         ((2, 4), [(9, 8, 0), (4, 3, 1)], (4, 3), False),                                      # downsampling + a raw view
         ((1, 255), [(2, 2, 0), (2, 2, 1)], (4, 4), False),
         # 2 views x two source rows of 25 x 255 fp32 = 102 000 bytes: above the kernel's 48 KB LDS budget, global taps
         ((1, 255), [(2, 25, 0), (2, 25, 1)], (3, 40), False),
         ((1, 5), [(3, 4, v % 2) for v in range(8)], (6, 8), False),                           # V = 8
         ((1, 3), [(2, 130, 0), (2, 130, 1)], (2, 259), False)]            # the mirrored column crosses a 256-pixel chunk
DTYPES = sc.DTYPES
OUTPUT_SUBSETS = sc.OUTPUT_SUBSETS
ALPHAS256 = sc.ALPHAS256
MIN_CONFS = sc.MIN_CONFS
EQUAL_K = sc.EQUAL_K
EQUAL_V = (1, 2, 4, 8)
GUARD_WIDTHS = (1, 2, 3, 5, 257, 259)
palette, grey = sc.palette, sc.grey

# Confidence bound.  tools/exp_ensemble_render_bounds.py measures torch's own float32 softmax -> mean over the views -> max
# against the same in float64, BOTH started from the restatement's float32 class values (so torch's float32 index arithmetic,
# which the kernel does not share, stays out), on CASES x DTYPES with the inputs of logits() below: the largest |difference| is
# ENSEMBLE_CONF_FIGURE (test_ensemble_render_reference.py holds this constant to what the tool's function measures).  The bound
# of the kernel's confidence against the float64 restatement is four times that, the convention of K19 - K36.
ENSEMBLE_CONF_FIGURE = 7.74727365593364e-08          # at 1x3-2x130_2x130f-2x259-fp32
ENSEMBLE_CONF_BOUND = 4.0 * ENSEMBLE_CONF_FIGURE
WEAK_SHARE_CAP = 0.005                        # at most 0.5 % of a case's pixels may have a top-two gap within 2 x the bound


def case_id(bk, views, size, align):
    runs = [f"{h}x{w}{'f' if f else ''}" for h, w, f in views]             # "7x9_7x9f": a view and its mirrored copy
    return (f"{bk[0]}x{bk[1]}-" + "_".join(runs) + "-" + ("same" if size is None else f"{size[0]}x{size[1]}")
            + ("-ac" if align else ""))


CASE_IDS = [case_id(*c) for c in CASES]


def out_size(views, size):
    return tuple(views[0][:2]) if size is None else tuple(size)


def logits(bk, views, dtype):
    """list of float32 CPU logits [B, K, h_v, w_v], one per view (seeded per view), rounded to `dtype`'s grid"""
    xs = []
    for v, (h, w, f) in enumerate(views):
        x = ar.randn_logits((bk[0], bk[1], h, w), seed=bk[0] + bk[1] + h + w + 31 * v)
        xs.append(x.to(torch.bfloat16).float() if dtype == "bf16" else x)
    return xs


def flips_of(views):
    return [bool(f) for _, _, f in views]


def torch_conf(vals, dtype):
    """max_k of the mean over the views of torch.softmax of the class values `vals` (float32 numpy [B, K, H, W] each), in `dtype`"""
    q = torch.stack([torch.from_numpy(np.ascontiguousarray(v)).to(dtype).softmax(1) for v in vals])
    return q.mean(0).max(1).values


def measure_conf_figure(report=None):
    """largest |torch float32 - torch float64| of softmax -> mean -> max from the restated float32 values over CASES x DTYPES"""
    worst, where = 0.0, None
    for bk, views, size, align in CASES:
        for dtype in DTYPES:
            vals = er.view_values([x.numpy() for x in logits(bk, views, dtype)], flips_of(views), out_size(views, size), align)
            d = float((torch_conf(vals, torch.float32).double() - torch_conf(vals, torch.float64)).abs().max())
            name = f"{case_id(bk, views, size, align)}-{dtype}"
            if report is not None:
                report(name, d)
            if d > worst:
                worst, where = d, name
    return worst, where
