#!/usr/bin/env python3
"""CPU measurement behind the bounds of the bilinear resize / L2-normalise kernels' tests (tests/test_hip_resize_routes.py): the fp32
models of the kernels' rounding points (tests/resize_cases.py: resize_fwd_model in both associations, resize_bwd_model,
l2_fwd_model, l2_bwd_model, fused_model for the vector and the scalar kernel) against the float64 references, in the error
measures of that module, on exactly the shapes and families the GPU tests run:

  resize_fwd_*   |y - y64| / bilinear(|x|)                       (bf16: less ulp_bf16(y64) / 2, the one final rounding)
  resize_bwd_*   |gx - gx64| / adjoint(|g|)
  l2_fwd_y       |y - y64| / |y64|;  l2_fwd_inv  |inv - inv64| / inv64
  l2_bwd         |gx - gx64| / (inv (|g| + |y| sum |y g|))
  fused_y        |y - y64| / ((A + |y64| |A|) / n), A = bilinear(|x|), n = |bilinear(x)|;  fused_inv  |inv - 1/n| / (|A| / n^2)

The bound of a quantity is four times its largest figure (the fused vector kernel's gets one fp32 ulp more for its rsqrtf).  The
kernels' own outputs never enter.  No GPU.
    python tools/exp_resize_bounds.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import resize_cases as rc  # noqa: E402


def report(quantity, value, where):
    print(f"{quantity} {value:.3e} {where}", flush=True)


def main():
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    worst = rc.measure(report)
    print(json.dumps({"figure": {k: v[0] for k, v in worst.items()}, "at": {k: v[1] for k, v in worst.items()},
                      "bound": {k: 4.0 * v[0] for k, v in worst.items()}, "in_cases_module": rc.BOUND}))


if __name__ == "__main__":
    main()
