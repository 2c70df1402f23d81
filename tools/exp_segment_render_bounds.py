#!/usr/bin/env python3
"""CPU measurement behind the confidence bound of oess_segment_render's tests (tests/test_hip_segment_render.py):
torch's own float32 path -- F.interpolate(mode='bilinear') in float32, softmax over the classes, max -- against the same three
operations in float64, on exactly the shapes, dtypes and inputs the GPU test runs (tests/segment_render_cases.py: ALL_SHAPES x
DTYPES, logits()).  The figure is the largest absolute difference of the two confidences; the test's bound is four times it.
The kernel's own outputs never enter.  No GPU.
    python tools/exp_segment_render_bounds.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import segment_render_cases as sc  # noqa: E402


def main():
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    figure, where = sc.measure_conf_figure(lambda case, d: print(f"conf {d:.3e} {case}", flush=True))
    print(json.dumps({"figure": {"conf": figure}, "at": {"conf": where}, "bound": {"conf": 4.0 * figure},
                      "in_cases_module": {"CONF_FIGURE": sc.CONF_FIGURE, "CONF_BOUND": sc.CONF_BOUND}}))


if __name__ == "__main__":
    main()
