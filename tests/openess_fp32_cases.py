"""Shared case of the joint OpenESS stage's fp32 tests (K23, tests/test_hip_openess_fp32.py) and of the CPU measurement that sets
their loss bounds (tools/exp_openess_fp32_bounds.py): the batch and weights of tests/test_hip_trainers.py::
test_openess_model_step_matches_oracle (64 x 96, B = 2, fill_by_name + damp_residual, dropout p = 0) and step 0 of
OracleOpenESSStep in any dtype from those weights.  Nothing here needs a GPU."""
import torch

from oracle.step import OracleOpenESSStep
from tests.synth import damp_residual, fill_by_name

K, HW, B, OUTPUT_STRIDE = 11, (64, 96), 2, 32
MODELS = ('model_recon', 'model_frame')
LOSS_KEYS = ('semseg_frame_loss', 'semseg_recon_loss', 'cons_feat_loss', 'cons_pred_loss', 'contrastive_nce_loss')
HEAD_PARAMS = ('classifier.ASPP.project.0.weight', 'classifier.classifier.0.weight', 'classifier.ASPP.convs.0.0.weight')


def batch():
    """(frame, None, recon, pseudo labels, superpixels) on the CPU; sample 0's superpixel ids reach into sample 1's range"""
    H, W = HW
    g = torch.Generator().manual_seed(8)
    frame, recon = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
    pl = torch.randint(0, K, (B, H // 4, W // 4), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2)
    pl[1, -6:] = 255
    sp = torch.randint(0, 45, (B, H // 8, W // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    assert int(sp[0].max()) >= 30
    return frame, None, recon, pl, sp


def seed_of(name):
    return 500 + len(name) + (7 if name == 'model_frame' else 0)


def prepare(module, name, reference_keys=None):
    """seeded weights by name, damped residual branches, dropout off (the two sides draw from different RNG streams)"""
    fill_by_name(module, seed_of(name), reference_keys)
    damp_residual(module)
    module.classifier.ASPP.project[3].p = 0.0
    return module


def oracle_step(reference_keys, dtype, contr=True):
    """OracleOpenESSStep in `dtype` from the shared weights; reference_keys: {model name: the product model's state_dict keys}"""
    ref = OracleOpenESSStep(K, contr, output_stride=OUTPUT_STRIDE)
    for name in MODELS:
        prepare(ref.modules()[name], name, sorted(reference_keys[name]))
        ref.modules()[name].to(dtype)
    return ref


_CACHE = {}


def oracle_losses(reference_keys, dtype, contr=True):
    """{loss key: float} of step 0 in `dtype` (computed once per dtype and shared)"""
    key = (dtype, contr)
    if key not in _CACHE:
        torch.set_num_threads(max(torch.get_num_threads(), 8))
        frame, _, recon, pl, sp = batch()
        with torch.no_grad():
            _, losses = oracle_step(reference_keys, dtype, contr).loss((frame.to(dtype), None, recon.to(dtype), pl, sp))
        _CACHE[key] = {k: float(v) for k, v in losses.items()}
    return _CACHE[key]
