#!/usr/bin/env python3
"""CPU measurement behind the bounds of tests/test_hip_train_fp32.py (K19): torch's own fp32 CPU autograd of the stage-2/3 oracle
step (oracle.step.OracleSupervisedStep, frame2voxel) against the same oracle in float64, on the cases of that test.

  teacher-forced (test b): three optimiser steps of the fp32 oracle; before each, its weights are copied into the float64 oracle;
      the relative error of the loss and, per trainable tensor, |g - g64|_2 / |g64|_2 (a bias in front of an InstanceNorm:
      max|db - db64| / max|dW64| of its conv), fine-tune and linear probe.
  free-running (test c): five steps of the fp32 and of the float64 fine-tune oracle from the same start at the YAML's learning
      rate, the relative error of the loss at every step, three seeds.

The bound of a group is four times its largest figure, with a floor of 1e-5 (the rule of K16 - K18).  No GPU.
    python tools/exp_train_fp32_bounds.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import train_fp32_cases as tc  # noqa: E402

LR = 5e-4                                   # lr_voxel of tests/configs/finetune_dsec_synthetic.yaml
SEEDS = (4, 5, 6)


def product_keys(linear_probing):
    from openess_amd.e2vid.model.model import E2VID_LIGHTWEIGHT_CONFIG, E2VIDRecurrent
    from openess_amd.models.style_networks import SemSegE2VID
    models = {'front_sensor_b': E2VIDRecurrent(E2VID_LIGHTWEIGHT_CONFIG),
              'back_end': SemSegE2VID(256, tc.K, skip_connect=True, skip_type='concat', text_embeddings_path='',
                                      materialize_ch256=False, if_linear_probing=linear_probing)}
    return {name: sorted(m.state_dict().keys()) for name, m in models.items()}


def teacher_forced(linear_probing, steps=3):
    keys = product_keys(linear_probing)
    ev, gt = tc.make_batch(4)
    f32 = tc.make_oracle(linear_probing, LR, keys, torch.float32)
    f64 = tc.make_oracle(linear_probing, LR, keys, torch.float64)
    worst = {'loss': 0.0, 'grad_l2': 0.0, 'norm_bias': 0.0}
    for it in range(steps):
        tc.copy_weights(f64, {n: m.state_dict() for n, m in f32.modules().items()})
        l64, g64 = tc.oracle_loss_and_grads(f64, ev, gt)
        l32, g32 = tc.oracle_loss_and_grads(f32, ev, gt)
        f32.optim.step()
        errs = tc.grad_errors(g32, g64)
        worst['loss'] = max(worst['loss'], tc.relerr(l32, l64))
        for n, e in errs.items():
            k = 'norm_bias' if tc.is_norm_bias(n) else 'grad_l2'
            worst[k] = max(worst[k], e)
        print(f"teacher-forced lp={linear_probing} step {it}: loss {l64:.6f} relerr {tc.relerr(l32, l64):.3e}, "
              f"worst grad L2 ratio {max(e for n, e in errs.items() if not tc.is_norm_bias(n)):.3e}, "
              f"worst norm-bias {max([e for n, e in errs.items() if tc.is_norm_bias(n)] or [0.0]):.3e}", flush=True)
    return worst


def free_running(seed, steps=5):
    keys = product_keys(False)
    ev, gt = tc.make_batch(seed)
    off = seed - SEEDS[0]
    f32 = tc.make_oracle(False, LR, keys, torch.float32, seed_offset=off)
    f64 = tc.make_oracle(False, LR, keys, torch.float64, seed_offset=off)
    dev = []
    for it in range(steps):
        l32 = float(f32.train_step((ev, gt))[1])
        l64 = float(f64.train_step((ev.double(), gt))[1])
        dev.append(tc.relerr(l32, l64))
        print(f"free-running seed {seed} step {it}: loss64 {l64:.6f} relerr {dev[-1]:.3e}", flush=True)
    return dev


def main():
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    out = {'teacher_forced': {('linear_probe' if lp else 'finetune'): teacher_forced(lp) for lp in (False, True)},
           'free_running': {str(s): free_running(s) for s in SEEDS}}
    tf = out['teacher_forced']
    fig = {'loss': max(v['loss'] for v in tf.values()), 'grad_l2': max(v['grad_l2'] for v in tf.values()),
           'norm_bias': max(v['norm_bias'] for v in tf.values()), 'trajectory': max(max(v) for v in out['free_running'].values())}
    out['largest'] = fig
    out['bound'] = {k: max(4.0 * v, 1e-5) for k, v in fig.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
