#!/usr/bin/env python3
"""Where the bounds of the K28 fp32 ConvGRU test come from (CPU only, no GPU, seconds):

  step_fp32_vs_f64   max |torch fp32 on the CPU - float64 restatement| of the new hidden state over three recurrent steps of
                     tests/convgru_cases.py's fp32 geometries; each step starts from the fp32 state of the step before, in both
                     precisions, as tests/test_hip_convgru.py's fp32 test continues from the kernel's own state.  That test
                     allows ConvGRU.step_f32 four times the figure of its geometry.
  exact_cases_hold   the float64 restatement and torch fp32 both give exactly the host integers for h' on the exact cases
                     (tests/test_convgru_host.py checks the gates as well).

    python tools/exp_convgru_bounds.py        -> one JSON line; the values are recorded in DESIGN.md K28
"""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import convgru_cases as cases                 # noqa: E402
from tests import convgru_reference as ref               # noqa: E402


def torch_step(x, h, c, dtype=torch.float32):
    """ConvGRU.forward of the reference written out in torch at `dtype`."""
    t = lambda k: c[k].to(dtype)
    x, h = x.to(dtype), h.to(dtype)
    s = torch.cat([x, h], 1)
    u = torch.sigmoid(F.conv2d(s, t('wu'), t('bu'), padding=1))
    r = torch.sigmoid(F.conv2d(s, t('wr'), t('br'), padding=1))
    o = torch.tanh(F.conv2d(torch.cat([x, h * r], 1), t('wo'), t('bo'), padding=1))
    return h * (1 - u) + o * u


def main():
    torch.set_num_threads(4)
    res = {'step_fp32_vs_f64': {}, 'exact_cases_hold': True}
    for geom in cases.GEOMS_F32:
        c = cases.random_case(*geom)
        h = torch.zeros_like(c['x'])
        worst = 0.0
        for s in range(3):
            x = cases.random_case(*geom, seed=77 + s)['x']
            got = torch_step(x, h, c)
            want = ref.step(x, h, c['wu'], c['bu'], c['wr'], c['br'], c['wo'], c['bo'])[0]
            worst = max(worst, float((got.double() - want).abs().max()))
            h = got
        res['step_fp32_vs_f64']['%dx%dx%dx%d' % geom] = worst
    for geom in cases.EXACT_GEOMS:
        c = cases.exact_case(*geom)
        want = cases.exact_expected(c)[-1].double()
        a = ref.step(c['x'], c['h'], c['wu'], c['bu'], c['wr'], c['br'], c['wo'], c['bo'])[0]
        b = torch_step(c['x'], c['h'], c).double()
        res['exact_cases_hold'] = res['exact_cases_hold'] and bool(torch.equal(a, want)) and bool(torch.equal(b, want))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
