"""Shared cases of the fp32 pre-training tests (K20: tests/test_hip_headpool_fp32.py, tests/test_hip_pretrain_fp32.py) and of the CPU
measurement that sets their bounds (tools/exp_pretrain_fp32_bounds.py): the head-pool inputs and their reference in any dtype, the
teacher head's convolution, the batch and weights of tests/test_hip_nets.py::test_pretrain_step_matches_oracle, the float64 oracle
step and the error measures.  Nothing here needs a GPU."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.step import OracleStep
from tests.synth import damp_residual, fill_by_name
from tests.train_fp32_cases import copy_weights, is_norm_bias, relerr  # noqa: F401  (re-exported)

# ------------------------------------------------------------------------------------------------------------ head-pool node
SCALE = 4
HEADPOOL_CASES = [(2, 256, 11, 16),      # the regular case
                  (1, 64, 7, 9),         # odd sizes, 64 channels
                  (2, 128, 5, 40),       # rows wider than one column tile (carry across iterations), 128 channels
                  (1, 64, 1, 9),         # a one-row map (degenerate vertical axis)
                  (2, 256, 3, 35)]       # a ragged last column tile
# name -> (B, C, h, w, sps, number of distinct raw ids, S or None = B * sps, zero 2 x 2 block)
HEADPOOL_VARIANTS = {'global_route': (1, 64, 7, 9, 300, 300, None, False),      # raw ids >= 256: straight to the global accumulators
                     'rows_beyond_S': (2, 64, 7, 9, 50, 37, 70, False),         # offset ids >= S are ignored
                     'zero_norm': (1, 64, 7, 9, 50, 37, None, True)}            # output pixels with zero norm: the clamp branch


def headpool_inputs(B, C, h, w, sps=50, nids=37, S=None, zero_block=False):
    """x [B, C, h, w], superpixels [B, 4h, 4w], sps, S, grad_k [S, C] built as test_upsampled_normalized_feature_pool builds them"""
    g = torch.Generator().manual_seed(C + w)
    x = torch.randn(B, C, h, w, generator=g)
    sp = torch.randint(0, nids, (B, SCALE * h, SCALE * w), generator=g)
    sp[0, :2] = sps - 1
    S = B * sps if S is None else S
    gk = torch.randn(S, C, generator=g)
    if zero_block:
        x[:, :, 2:4, 3:5] = 0.0
    return x, sp, sps, S, gk


def headpool_reference(x, sp, sps, S, gk, dtype):
    """(k, count, grad_x) of the reference ops in `dtype` (autograd): F.interpolate(align_corners=True), F.normalize, index_add_ over
    the pixels whose offset id lies in [0, S), / (count + 1e-6)"""
    B, C = x.shape[:2]
    xd = x.detach().to(dtype).requires_grad_(True)
    up = F.interpolate(xd, scale_factor=SCALE, mode="bilinear", align_corners=True)
    fn = F.normalize(up, p=2, dim=1).permute(0, 2, 3, 1).reshape(-1, C)
    ids = (sp + torch.arange(B, device=sp.device)[:, None, None] * sps).reshape(-1)
    keep = (ids >= 0) & (ids < S)
    ids, fn = ids[keep], fn[keep]
    sums = torch.zeros(S, C, dtype=dtype, device=x.device).index_add_(0, ids, fn)
    cnt = torch.zeros(S, dtype=dtype, device=x.device).index_add_(0, ids, torch.ones_like(ids, dtype=dtype))
    k = sums / (cnt[:, None] + 1e-6)
    k.backward(gk.to(dtype))
    return k.detach(), cnt, xd.grad


def max_ratio(a, ref):
    """max|a - ref| / max|ref|"""
    return float((a.double() - ref.double()).abs().max() / ref.double().abs().max())


def l2_ratio(a, ref):
    """|a - ref|_2 / |ref|_2 over the whole tensor"""
    return float((a.double() - ref.double()).norm() / ref.double().norm())


# ------------------------------------------------------------------------------------------------------- teacher head conv
HEAD_CONV = (2, 2048, 256, 16, 24)          # B, Cin, Cout, H, W: DilationFeatureExtractor.decoder[0] on a 2 x 16 x 24 map


def head_conv_inputs():
    B, Cin, Cout, H, W = HEAD_CONV
    g = torch.Generator().manual_seed(2048)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5
    b = torch.randn(Cout, generator=g)
    gy = torch.randn(B, Cout, H, W, generator=g)
    return x, w, b, gy


def head_conv_reference(x, w, b, gy, dtype):
    """(y, dx, dw, db) of F.conv2d in `dtype`"""
    xd, wd, bd = (t.detach().to(dtype).requires_grad_(True) for t in (x, w, b))
    y = F.conv2d(xd, wd, bd)
    y.backward(gy.to(dtype))
    return y.detach(), xd.grad, wd.grad, bd.grad


# -------------------------------------------------------------------------------------------------------------- the step
K, NWIN, BINS, H, W, B, SPS, LR = 11, 3, 5, 64, 96, 2, 25, 1e-4


def make_batch(seed=3, H=H, W=W):
    """(events, frame, pseudo-labels with one ignored band, superpixels, S) of test_pretrain_step_matches_oracle"""
    torch.manual_seed(seed)
    ev = (torch.randn(B, NWIN * BINS, H, W) * (torch.rand(B, NWIN * BINS, H, W) > 0.7)).contiguous()
    frame = torch.rand(B, 3, H, W)
    pl = torch.randint(0, K, (B, H, W))
    pl[0, :5] = 255
    sp = torch.randint(0, SPS, (B, H // 8, W // 8)).repeat_interleave(8, 1).repeat_interleave(8, 2)
    S = int((sp + torch.arange(B)[:, None, None] * SPS).max()) + 1
    return ev, frame, pl, sp, S


def fill_models(models):
    """fill_by_name(100 + len(name)) + damp_residual, as test_pretrain_step_matches_oracle; returns the sorted keys per model"""
    keys = {}
    for name, m in models.items():
        fill_by_name(m, 100 + len(name))
        damp_residual(m)
        keys[name] = sorted(m.state_dict().keys())
    return keys


def make_oracle(contr, keys, dtype=torch.float64, lr=LR):
    ref = OracleStep('frame2voxel', K, NWIN, BINS, contr, SPS, lr=lr)
    for name, m in ref.modules().items():
        fill_by_name(m, 100 + len(name), keys[name])
        damp_residual(m)
        m.to(dtype)
    return ref


def oracle_batch(ref, batch):
    ev, frame, pl, sp = batch[:4]
    dtype = next(ref.back_end.parameters()).dtype
    return (ev.to(dtype), None, frame.to(dtype), pl, sp)


TRAINED = ('back_end', 'model_frame')


def oracle_loss_and_grads(ref, batch):
    """({loss name: value}, total, {'<model>.<parameter>': gradient}) of the oracle's step on the batch, without stepping"""
    ref.opt_a.zero_grad()
    ref.opt_b.zero_grad()
    total, losses = ref.loss(oracle_batch(ref, batch))
    total.backward()
    grads = {f"{m}.{n}": p.grad.detach().clone() for m in TRAINED for n, p in ref.modules()[m].named_parameters() if p.grad is not None}
    return {k: float(v) for k, v in losses.items()}, float(total.detach()), grads


def oracle_step(ref, batch):
    losses, total = ref.train_step(oracle_batch(ref, batch))
    return {k: float(v) for k, v in losses.items()}, float(total)


def grad_errors(got, want):
    """{name: error} of gradients `got` against the float64 `want`, names '<model>.<parameter>': the L2 ratio |g - g64| / |g64|; a
    conv bias of the student in front of an InstanceNorm (analytically zero gradient) max|db - db64| / max|dW64| of its conv.
    Every element of every tensor of `want` is compared."""
    out = {}
    for n, g64 in want.items():
        g = np.asarray(got[n].detach().cpu().double().numpy())
        g64n = g64.double().numpy()
        assert g.shape == g64n.shape, n
        if n.startswith('back_end.') and is_norm_bias(n[len('back_end.'):]):
            out[n] = float(np.abs(g - g64n).max() / np.abs(want[n[:-len('bias')] + 'weight'].double().numpy()).max())
        else:
            out[n] = float(np.linalg.norm((g - g64n).ravel()) / np.linalg.norm(g64n.ravel()))
    return out


def is_student_norm_bias(n):
    return n.startswith('back_end.') and is_norm_bias(n[len('back_end.'):])
