#!/usr/bin/env python3
"""CPU measurement behind the two bounds of the open-vocabulary render tests (tests/test_hip_vocab_render.py), on
exactly the cases, dtypes and inputs the GPU tests run (tests/vocab_render_cases.py):
  group_conf  torch's own float32 path against the same in float64 -- F.interpolate -> per-group amax -> softmax -> max on
              GROUP_CASES: the largest absolute difference of the two confidences;
  head_conf   the same for 1 x 1 conv -> per-group amax -> softmax -> max on RANDOM_CASES;
  value       torch's float32 1 x 1 conv against float64 on RANDOM_CASES, relative to the scale |bias_p| + sum_c |w[p][c] x[c]| of the
         name value's terms.
Each bound is four times its figure.  The kernels' own outputs never enter.  No GPU.
    python tools/exp_vocab_render_bounds.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import vocab_render_cases as vc  # noqa: E402


def main():
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    worst = vc.measure_figures(lambda kind, case, d: print(f"{kind} {d:.3e} {case}", flush=True))
    print(json.dumps({"figure": {k: v[0] for k, v in worst.items()}, "at": {k: v[1] for k, v in worst.items()},
                      "bound": {k: 4.0 * v[0] for k, v in worst.items()},
                      "in_cases_module": {"GROUP_CONF_FIGURE": vc.GROUP_CONF_FIGURE, "HEAD_CONF_FIGURE": vc.HEAD_CONF_FIGURE,
                                          "VALUE_FIGURE": vc.VALUE_FIGURE}}))


if __name__ == "__main__":
    main()
