#!/usr/bin/env python3
"""CPU measurement behind the bounds of tests/test_hip_headpool_fp32.py and tests/test_hip_pretrain_fp32.py (K20): torch's own
fp32 CPU autograd against the same computation in float64, on the cases of those tests (tests/pretrain_fp32_cases.py).

  head-pool node: k and grad_x of interpolate -> normalize -> index_add_ -> / (count + 1e-6) on the five cases and the three
      variants (max|a - a64| / max|a64|; the zero-norm variant's grad_x by |g - g64|_2 / |g64|_2 over the whole tensor).
  teacher head conv: y, dx, dw, db of the 2048 -> 256 1 x 1 convolution on a 2 x 16 x 24 map (L2 ratio per tensor).
  step, teacher-forced (test b): oracle.step.OracleStep (frame2voxel) in fp32 against float64 from the same weights, with and
      without the contrastive loss: the relative error of each loss and, per trainable tensor of the student and of the teacher's
      head, |g - g64|_2 / |g64|_2 (a bias in front of an InstanceNorm: max|db - db64| / max|dW64| of its conv).
  step, free-running (test c): three steps of the fp32 and of the float64 oracle from the same start, contrastive loss on: the
      relative error of every loss at every step.

The bound of a group is four times its largest figure, with a floor of 1e-5 (the rule of K16 - K19).  No GPU.
    python tools/exp_pretrain_fp32_bounds.py [--steps N] [--height H --width W]
The defaults are the tests' cases (three free steps at 64 x 96); other values are for trying the tool out and give no bound.
The last line is one JSON object."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import pretrain_fp32_cases as pc  # noqa: E402


def headpool():
    fig = {'k': 0.0, 'gx': 0.0, 'zero_norm_gx_l2': 0.0}
    cases = [(f"{c}", pc.headpool_inputs(*c)) for c in pc.HEADPOOL_CASES]
    cases += [(n, pc.headpool_inputs(*v[:4], sps=v[4], nids=v[5], S=v[6], zero_block=v[7])) for n, v in pc.HEADPOOL_VARIANTS.items()]
    for name, (x, sp, sps, S, gk) in cases:
        k64, _, g64 = pc.headpool_reference(x, sp, sps, S, gk, torch.float64)
        k32, _, g32 = pc.headpool_reference(x, sp, sps, S, gk, torch.float32)
        ek, eg, el2 = pc.max_ratio(k32, k64), pc.max_ratio(g32, g64), pc.l2_ratio(g32, g64)
        print(f"head-pool {name}: k {ek:.3e} (abs {float((k32.double() - k64).abs().max()):.3e}), gx max-ratio {eg:.3e}, gx L2 ratio {el2:.3e}",
              flush=True)
        fig['k'] = max(fig['k'], ek)
        if name == 'zero_norm':
            fig['zero_norm_gx_l2'] = el2
        else:
            fig['gx'] = max(fig['gx'], eg)
    return fig


def head_conv():
    x, w, b, gy = pc.head_conv_inputs()
    r64 = pc.head_conv_reference(x, w, b, gy, torch.float64)
    r32 = pc.head_conv_reference(x, w, b, gy, torch.float32)
    errs = {n: pc.l2_ratio(a, r) for n, a, r in zip(('y', 'dx', 'dw', 'db'), r32, r64)}
    print("teacher head conv 2048 -> 256:", {k: f"{v:.3e}" for k, v in errs.items()}, flush=True)
    return {'head_conv': max(errs.values())}


def product_keys():
    from openess_amd.e2vid.model.model import E2VID_LIGHTWEIGHT_CONFIG, E2VIDRecurrent
    from openess_amd.models.image_model import DilationFeatureExtractor
    from openess_amd.models.style_networks import SemSegE2VID
    models = {'front_sensor_b': E2VIDRecurrent(E2VID_LIGHTWEIGHT_CONFIG),
              'back_end': SemSegE2VID(256, pc.K, skip_connect=True, skip_type='concat', text_embeddings_path='',
                                      materialize_ch256='pooled'),
              'model_frame': DilationFeatureExtractor(image_weights=None)}
    return {name: sorted(m.state_dict().keys()) for name, m in models.items()}


def teacher_forced(f32, f64, contr, batch):
    """one evaluation of both oracles from their common weights; nothing is stepped (train-mode BatchNorm reads batch statistics, so
    the running statistics the call moves change no later figure)"""
    f32.contr = f64.contr = contr
    l64, t64, g64 = pc.oracle_loss_and_grads(f64, batch)
    l32, t32, g32 = pc.oracle_loss_and_grads(f32, batch)
    assert set(g32) == set(g64)
    errs = pc.grad_errors(g32, g64)
    worst = {'loss': max(pc.relerr(l32[k], l64[k]) for k in l64),
             'grad_l2': max(e for n, e in errs.items() if not pc.is_student_norm_bias(n)),
             'norm_bias': max([e for n, e in errs.items() if pc.is_student_norm_bias(n)] or [0.0])}
    top = sorted(((e, n) for n, e in errs.items() if not pc.is_student_norm_bias(n)), reverse=True)[:4]
    print(f"teacher-forced contrastive={contr}: losses {l64}, relerr {worst['loss']:.3e}, worst grad L2 ratio {worst['grad_l2']:.3e}, "
          f"worst norm-bias {worst['norm_bias']:.3e}; largest: {[(n, f'{e:.2e}') for e, n in top]}", flush=True)
    return worst


def free_running(f32, f64, steps, batch):
    f32.contr = f64.contr = True
    dev = []
    for it in range(steps):
        l32, t32 = pc.oracle_step(f32, batch)
        l64, t64 = pc.oracle_step(f64, batch)
        dev.append(max([pc.relerr(l32[k], l64[k]) for k in l64] + [pc.relerr(t32, t64)]))
        print(f"free-running step {it}: float64 losses {l64}, worst relerr {dev[-1]:.3e}", flush=True)
    return dev


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=3, help="free-running steps")
    ap.add_argument("--height", type=int, default=pc.H)
    ap.add_argument("--width", type=int, default=pc.W)
    args = ap.parse_args(argv)
    if args.height % 8 or args.width % 8 or args.steps < 1:
        ap.error("height and width must be multiples of 8 (the superpixel blocks), steps >= 1")
    hw = (args.height, args.width)
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    fig = {}
    fig.update(headpool())
    fig.update(head_conv())
    keys, batch = product_keys(), pc.make_batch(3, *hw)
    f32, f64 = pc.make_oracle(True, keys, torch.float32), pc.make_oracle(True, keys, torch.float64)
    tf = [teacher_forced(f32, f64, c, batch) for c in (False, True)]
    for k in ('loss', 'grad_l2', 'norm_bias'):
        fig[k] = max(v[k] for v in tf)
    fig['trajectory'] = max(free_running(f32, f64, args.steps, batch))
    print(json.dumps({'largest': fig, 'bound': {k: max(4.0 * v, 1e-5) for k, v in fig.items()}}))


if __name__ == "__main__":
    main()
