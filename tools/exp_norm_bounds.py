#!/usr/bin/env python3
"""CPU measurement behind the bounds of the bf16 normalisation kernels' tests (tests/test_hip_norm_routes.py): the fp32 models of
the kernels' rounding points (tests/norm_cases.py: stats_model, finalize_model, apply_model, bwd_apply_model) against the float64
references, in the error measures of that module, on exactly the cases and families the GPU tests run (bounded_cases x FAMILIES):

  mean      |mean - mean64| / rms(x)
  rstd      |rstd - rstd64| / rstd64, in units of E[x^2] / (var + eps)
  y         max(0, |y - y64| - ulp_bf16(y64) / 2) / ((|x| + |mean|) |scale| + |beta| + |residual|)
  s1, s2    |s - s64| / sum |g|, |s - s64| / sum |g xhat|           (d(beta) and d(gamma) of BatchNorm)
  dx        max(0, |dx - dx64| - ulp_bf16(dx64) / 2) / (|gamma rstd| (|g| + sum|g| / N + |xhat| sum|g xhat| / N)), mean and rstd operands
  s2_chain, dx_chain  the same as s2 and dx with the statistics taken from the forward model (the reference's from float64),
            in units of 1 + E[x^2] / (var + eps)

The bound of a quantity is four times its largest figure.  The kernels' own outputs never enter.  No GPU.
    python tools/exp_norm_bounds.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import norm_cases as nc  # noqa: E402


def report(kind, G, ppg, C, tiles, family, fig):
    print(f"{kind} G={G} ppg={ppg} C={C}" + (f" tiles={tiles}" if tiles else "") + f" {family}: " +
          " ".join(f"{k} {v:.3e}" for k, v in sorted(fig.items())), flush=True)


def main():
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    worst = nc.measure(report)
    print(json.dumps({"figure": {k: v[0] for k, v in worst.items()}, "at": {k: list(v[1:]) for k, v in worst.items()},
                      "bound": {k: 4.0 * v[0] for k, v in worst.items()}, "in_cases_module": nc.BOUND}))


if __name__ == "__main__":
    main()
