"""Shared cases of the fp32 training tests (K19, tests/test_hip_train_fp32.py) and of the CPU measurement that sets their bounds
(tools/exp_train_fp32_bounds.py): the batch and weights of tests/test_hip_trainers.py, the float64 oracle step, and the error
measures.  Nothing here needs a GPU."""
import numpy as np
import torch

from oracle import losses as ol
from oracle.step import OracleSupervisedStep
from tests.synth import damp_residual, fill_by_name

K, NWIN, BINS, H, W, B = 11, 3, 5, 64, 96, 2             # tests/configs/finetune_dsec_synthetic.yaml, B = 2
WEIGHT_SEED = {'front_sensor_b': 300 + len('front_sensor_b'), 'back_end': 300 + len('back_end')}


def make_batch(seed=4):
    """(events [B, NWIN * BINS, H, W] fp32, ground truth [B, H, W] with one ignored band): the batch of test_hip_trainers.py"""
    torch.manual_seed(seed)
    ev = (torch.randn(B, NWIN * BINS, H, W) * (torch.rand(B, NWIN * BINS, H, W) > 0.7)).contiguous()
    torch.rand(B, 3, H, W)                                   # the reconstruction slot of that test: keeps the stream of draws
    gt = torch.randint(0, K, (B, H // 4, W // 4)).repeat_interleave(4, 1).repeat_interleave(4, 2)
    gt[0, :5] = 255
    return ev, gt


def fill_models(models, seed_offset=0):
    """fill_by_name + damp_residual with the seeds of test_hip_trainers.py; returns the sorted state_dict keys per model"""
    keys = {}
    for name, m in models.items():
        fill_by_name(m, WEIGHT_SEED[name] + seed_offset)
        damp_residual(m)
        keys[name] = sorted(m.state_dict().keys())
    return keys


def make_oracle(linear_probing, lr, keys, dtype=torch.float64, seed_offset=0):
    """OracleSupervisedStep (frame2voxel) filled like the product (keys: the product's state_dict keys per model), in `dtype`"""
    ref = OracleSupervisedStep("frame2voxel", K, NWIN, BINS, linear_probing, lr=lr)
    for name, m in ref.modules().items():
        fill_by_name(m, WEIGHT_SEED[name] + seed_offset, keys[name])
        damp_residual(m)
        m.to(dtype)
    return ref


def copy_weights(ref, state_dicts):
    """the product's (or another oracle's) current weights into the oracle, in the oracle's dtype; keys the oracle lacks are
    layers it does not restate"""
    for name, m in ref.modules().items():
        own = m.state_dict()
        dtype = next(m.parameters()).dtype
        new = {k: (v.detach().cpu().to(dtype) if v.dtype.is_floating_point else v.detach().cpu())
               for k, v in state_dicts[name].items() if k in own}
        assert set(new) == set(own), sorted(set(own) - set(new))
        m.load_state_dict(new)


def oracle_loss_and_grads(ref, ev, gt, weight=1.0):
    """loss and {parameter name: gradient} of the oracle's step on the batch, without stepping its optimiser"""
    dtype = next(ref.net.parameters()).dtype
    ref.net.train()
    ref.optim.zero_grad()
    loss = ol.task_loss(ref.logits((ev.to(dtype), gt)), gt, K) * weight
    loss.backward()
    return float(loss.detach()), {n: p.grad.detach().clone() for n, p in ref.net.named_parameters() if p.grad is not None}


def is_norm_bias(name):
    """a conv bias in front of an InstanceNorm: its gradient is analytically zero"""
    return name.startswith(('decoder_scale_1.', 'decoder_scale_2.', 'decoder_scale_3.', 'decoder_scale_4.')) and name.endswith('.bias')


def grad_errors(got, want):
    """{name: error} of gradients `got` against the float64 `want`: the L2 ratio |g - g64| / |g64|; a bias in front of an
    InstanceNorm max|db - db64| / max|dW64| of its conv.  Every element of every tensor of `want` is compared."""
    out = {}
    for n, g64 in want.items():
        g = np.asarray(got[n].detach().cpu().double().numpy())
        g64n = g64.double().numpy()
        assert g.shape == g64n.shape, n
        if is_norm_bias(n):
            out[n] = float(np.abs(g - g64n).max() / np.abs(want[n[:-len('bias')] + 'weight'].double().numpy()).max())
        else:
            out[n] = float(np.linalg.norm((g - g64n).ravel()) / np.linalg.norm(g64n.ravel()))
    return out


def relerr(a, b):
    return abs(float(a) - float(b)) / abs(float(b))
