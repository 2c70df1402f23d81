#!/usr/bin/env python3
"""CPU measurement behind the bounds of tests/test_hip_deeplab_fp32_train.py (K22): torch's own fp32 CPU autograd against float64
on every case of that test (tests/deeplab_fp32_train_cases.py), relerr = max|a32 - a64| / max|a64| per tensor, the largest per
group:

  pool:      the ASPP pooling branch (AdaptiveAvgPool2d(1), 1 x 1 conv, BatchNorm over the B pooled vectors, ReLU, broadcast):
             output, dx, dW, dgamma, dbeta;
  head:      the DeepLab head with a fixed dropout mask: logits, the ASPP feature, every parameter gradient;
  model_out: the mini dilated backbone + head + bilinear resize [+ linear probe]: full-size logits and ASPP feature;
  model:     the same, and every parameter gradient.

The bound of a group is four times its largest figure, with a floor of 1e-5 (the rule of K16 - K21).  No GPU.
    python tools/exp_deeplab_fp32_train_bounds.py"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import deeplab_fp32_train_cases as dc  # noqa: E402


def errs(names, got, want):
    return {n: dc.relerr(a.detach().numpy(), b.detach().numpy()) for n, a, b in zip(names, got, want) if b is not None}


def worst(e):
    k = max(e, key=e.get)
    return k, e[k]


def pool_figures():
    fig = 0.0
    for i, case in enumerate(dc.POOL_CASES):
        t0 = time.time()
        ref, x, dy, y64, want, _, margin = dc.pool_case(i)
        assert margin >= dc.RELU_MARGIN, (case, margin)
        (y32,), got, _ = dc.grads_of(dc.pool_forward, ref, x, dy, torch.float32)
        e = errs(['out', 'dx', 'dW', 'dgamma', 'dbeta'], (y32,) + tuple(got), (y64,) + tuple(want))
        print(f"pool {case}: " + " ".join(f"{k} {v:.3e}" for k, v in e.items()) + f", ReLU margin {margin:.2e}, {time.time() - t0:.1f} s",
              flush=True)
        fig = max(fig, worst(e)[1])
    return fig


def head_figures():
    fig = 0.0
    for i, case in enumerate(dc.HEAD_CASES):
        t0 = time.time()
        ref, x, dy, names, ys64, want, margin = dc.head_case(i)
        assert margin >= dc.RELU_MARGIN, (case, margin)
        ys32, got = dc.head_grads_fp32(i)
        e_out = errs(['logits', 'feature'], ys32, ys64)
        k, e_g = worst(errs(['x'] + names, got, want))
        print(f"head {case}: logits {e_out['logits']:.3e} feature {e_out['feature']:.3e}, worst gradient {e_g:.3e} ({k}), "
              f"ReLU margin {margin:.2e}, {time.time() - t0:.1f} s", flush=True)
        fig = max(fig, e_g, *e_out.values())
    return fig


def model_figures():
    out_fig = fig = 0.0
    for probe in (False, True):
        t0 = time.time()
        ref, x, dy, names, ys64, want, margin = dc.model_case(probe=probe)
        assert margin >= dc.RELU_MARGIN, margin
        _, _, _, _, ys32, got, _ = dc.model_case(probe=probe, dtype=torch.float32)
        e_out = errs(['logits', 'feats'], ys32, ys64)
        k, e_g = worst(errs(['x'] + names, got, want))
        print(f"model probe={probe}: logits {e_out['logits']:.3e} feats {e_out['feats']:.3e}, worst gradient {e_g:.3e} ({k}), "
              f"ReLU margin {margin:.2e}, {time.time() - t0:.1f} s", flush=True)
        out_fig = max(out_fig, *e_out.values())
        fig = max(fig, e_g, *e_out.values())
    return out_fig, fig


def main():
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    fig = {'pool': pool_figures(), 'head': head_figures()}
    fig['model_out'], fig['model'] = model_figures()
    print(json.dumps({'largest': fig, 'bound': {k: max(4.0 * v, 1e-5) for k, v in fig.items()}}))


if __name__ == "__main__":
    main()
