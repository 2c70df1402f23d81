#!/usr/bin/env python3
"""CPU measurement behind the bounds of tests/test_hip_resnet_fp32_train.py (K21): torch's own fp32 CPU autograd against float64
on every case of that test (tests/resnet_fp32_cases.py), relerr = max|g32 - g64| / max|g64| per tensor, the largest per group:

  wgrad / dgrad: F.conv2d with stride, padding and dilation; bn: train-mode F.batch_norm [+ residual] [+ ReLU];
  pool: F.max_pool2d(3, 2, 1); blocks: oracle.nets.Bottleneck in train mode (seeds 0 and 1; the tests run seed 0);
  backbone: the mini dilated ResNet, every parameter gradient, on the seed the tests run (0).

The bound of a group is four times its largest figure, with a floor of 1e-5 (the rule of K16 - K20).  No GPU.
    python tools/exp_resnet_fp32_bounds.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import resnet_fp32_cases as rc  # noqa: E402


def worst(got, want):
    return max(rc.relerr(a.detach().numpy(), b.detach().numpy()) for a, b in zip(got, want) if b is not None)


def conv_figures():
    w_fig = d_fig = 0.0
    for i, case in enumerate(rc.CONV_CASES):
        (x, w, b, dy), (dx64, dw64, db64) = rc.conv_case(i)
        dx, dw, db = rc.conv_grads(x, w, b, dy, case[6], case[7], case[8], torch.float32)
        e_w, e_d = worst([dw, db], [dw64, db64]), rc.relerr(dx.numpy(), dx64.numpy())
        print(f"conv {case}: dW/db {e_w:.3e} dX {e_d:.3e}", flush=True)
        w_fig, d_fig = max(w_fig, e_w), max(d_fig, e_d if i != rc.STEM_CASE else 0.0)
    return w_fig, d_fig


def bn_figures():
    fig = 0.0
    cases = [(i, v, True) for i in range(len(rc.BN_SHAPES)) for v in rc.BN_VARIANTS] + [(1, 'relu', False)]
    for i, v, affine in cases:
        (x, gamma, beta, res, dy, relu), want, margin = rc.bn_case(i, v, affine)
        assert margin is None or margin >= rc.RELU_MARGIN, (i, v, margin)
        e = worst(rc.bn_grads(x, gamma, beta, res, dy, relu, torch.float32), want)
        print(f"bn {rc.BN_SHAPES[i]} {v} affine={affine}: {e:.3e}", flush=True)
        fig = max(fig, e)
    return fig


def pool_figures():
    fig = 0.0
    for i in range(len(rc.POOL_SHAPES)):
        x, dy = rc.pool_case(i)
        e = rc.relerr(rc.pool_grad(x, dy, torch.float32).numpy(), rc.pool_grad(x, dy, torch.float64).numpy())
        print(f"pool {rc.POOL_SHAPES[i]}: {e:.3e}", flush=True)
        fig = max(fig, e)
    return fig


def net_figures(name, case, forward, n, seeds=(0, 1), skip_x=False):
    fig = 0.0
    for i in range(n):
        for seed in seeds:
            ref, x, dy, names, y64, want, margin = case(i, seed) if n > 1 else case(seed)
            assert margin >= rc.RELU_MARGIN, (name, i, seed, margin)
            _, got = rc.net_grads(forward, ref, x, dy, torch.float32)
            errs = [rc.relerr(a.numpy(), b.numpy()) for a, b in zip(got, want)]
            if skip_x:
                errs[0] = 0.0                    # the image's gradient: the product does not compute it
            k = max(range(len(errs)), key=errs.__getitem__)
            print(f"{name} {i} seed {seed}: worst gradient relerr {errs[k]:.3e} ({(['x'] + names)[k]}), ReLU margin {margin:.2e}",
                  flush=True)
            fig = max(fig, errs[k])
    return fig


def main():
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    w_fig, d_fig = conv_figures()
    fig = {'wgrad': w_fig, 'dgrad': d_fig, 'bn': bn_figures(), 'pool': pool_figures(),
           'blocks': net_figures('block', rc.block_case, rc.block_forward, len(rc.BLOCK_CASES)),
           'backbone': net_figures('backbone', rc.backbone_case, rc.backbone_forward, 1, seeds=(0,), skip_x=True)}
    print(json.dumps({'largest': fig, 'bound': {k: max(4.0 * v, 1e-5) for k, v in fig.items()}}))


if __name__ == "__main__":
    main()
