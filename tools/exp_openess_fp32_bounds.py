#!/usr/bin/env python3
"""CPU measurement behind the bounds of the joint OpenESS stage's fp32 tests (K23): torch's own fp32 CPU arithmetic against
float64, relerr = max|a32 - a64| / max|a64| per tensor (|a32 - a64| / |a64| for a loss).

  node:  every case of tests/upsampled_l1_cases.py (tests/test_hip_upsampled_l1_f32.py): F.l1_loss(F.interpolate(a),
         F.interpolate(b)) and its two gradients, with the conditioning rounds and the margin that holds for every element;
  step:  step 0 of OracleOpenESSStep on the batch and weights of tests/openess_fp32_cases.py (tests/test_hip_openess_fp32.py)
         against a .double() copy from identical weights: the five losses.

The bound of a quantity is four times its largest figure, with a floor of 1e-5 (the rule of K16 - K22).  No GPU.
    python tools/exp_openess_fp32_bounds.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import openess_fp32_cases as oc  # noqa: E402
from tests import upsampled_l1_cases as uc  # noqa: E402


def node_figures():
    fig = {'loss': 0.0, 'grad_a': 0.0, 'grad_b': 0.0}
    runs = [(i, None) for i in range(len(uc.CASES))] + [(uc.FALLBACK_CASE, uc.FALLBACK_C)]
    for i, C in runs:
        c, e = uc.case(i, C), uc.fp32_cpu_errors(i, C)
        print(f"node case {i} {uc.CASES[i]}" + (f" C={C}" if C else "") + ": " + " ".join(f"{k} {v:.3e}" for k, v in e.items()) +
              f", {c['rounds']} conditioning rounds, margin {c['margin']:.3e}", flush=True)
        fig = {k: max(fig[k], e[k]) for k in fig}
    return fig


def product_keys():
    """state_dict keys of the product's students (the index of a key in the sorted list seeds its values, tests/synth.py)"""
    from openess_amd.models.deeplabv3 import deeplabv3_resnet50
    m = deeplabv3_resnet50(num_classes=oc.K, text_embeddings_path='', output_stride=oc.OUTPUT_STRIDE, pretrained_backbone='')
    return {name: list(m.state_dict().keys()) for name in oc.MODELS}


def step_figures():
    keys = product_keys()
    l64, l32 = oc.oracle_losses(keys, torch.float64), oc.oracle_losses(keys, torch.float32)
    fig = {k: abs(l32[k] - l64[k]) / abs(l64[k]) for k in oc.LOSS_KEYS}
    for k in oc.LOSS_KEYS:
        print(f"step {k}: float64 {l64[k]:.9g} fp32 {l32[k]:.9g} relerr {fig[k]:.3e}", flush=True)
    return fig


def main():
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    fig = {'node': node_figures(), 'step': step_figures()}
    print(json.dumps({'largest': fig, 'bound': {g: {k: max(4.0 * v, 1e-5) for k, v in f.items()} for g, f in fig.items()}}))


if __name__ == "__main__":
    main()
