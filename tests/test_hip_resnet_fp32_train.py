"""GPU tests of the fp32 backward of the dilated ResNet-50 backbone (K21: conv_wgrad_f32.hip, conv_f32.hip's stride-2 data
gradient, resnet_bwd_f32.hip and the fp32 autograd functions of openess_amd.hip), every gradient against float64 torch autograd on
the CPU.  The cases live in tests/resnet_fp32_cases.py.

Error measure: relerr = max|got - want| / max|want|.  The bound of a group is four times the largest relerr torch's OWN fp32 CPU
autograd reaches against float64 on that group's cases, with a floor of 1e-5 (the rule of K16 - K20).  Measured on the CPU by
tools/exp_resnet_fp32_bounds.py (CPU_FP32_RELERR below):

    group      torch fp32 CPU vs float64    bound
    wgrad      8.8e-07 (dW, db)             1e-5
    dgrad      4.0e-07                      1e-5
    bn         2.4e-06                      1e-5
    pool       9.7e-08                      1e-6  (set by the issue: a sum of at most four terms)
    blocks     9.8e-07                      1e-5
    backbone   1.21e-05                     4.84e-5

ReLU masks: every case with a ReLU conditions its seeded input (condition_relu_margin of the K18 test) and the test asserts, on
the float64 reference, that no ReLU input lies below 1e-4 of its layer's largest magnitude before it compares.  No element is
left out of any comparison."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import resnet_fp32_cases as rc
from tests.resnet_fp32_cases import relerr

pytestmark = pytest.mark.gpu

CPU_FP32_RELERR = {'wgrad': 8.8e-7, 'dgrad': 4.0e-7, 'bn': 2.44e-6, 'blocks': 9.8e-7, 'backbone': 1.211e-5}
BOUND = {k: max(4.0 * v, 1e-5) for k, v in CPU_FP32_RELERR.items()}
BOUND['pool'] = 1e-6
RELU_MARGIN = rc.RELU_MARGIN


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _np(t):
    return t.detach().cpu().numpy()


def _report(name, value, bound):
    print(f"[resnet_fp32_train] {name}: {value:.3e} (bound {bound:.1e})", flush=True)
    return value


def _slice_of_wide(t, fill=3.0):
    """t [B, C, H, W] as a channel slice of a wider channels_last buffer"""
    B, C, H, W = t.shape
    wide = torch.full((B, H, W, C + 12), fill, device="cuda")
    wide[..., 8:8 + C] = t.permute(0, 2, 3, 1).cuda()
    return wide[..., 8:8 + C].permute(0, 3, 1, 2)


def _layout(t, layout):
    if t is None:
        return None
    return {'nhwc': _cl, 'nchw': lambda v: v.cuda().contiguous(), 'slice': _slice_of_wide}[layout](t)


# ------------------------------------------------------------------------------------------------------------ convolution
def _conv_operands(i):
    (x, w, b, dy), _ = rc.conv_case(i)
    xd = _slice_of_wide(x) if i == rc.X_SLICE_CASE else _cl(x)
    gd = dy.cuda().contiguous() if i == rc.DY_NCHW_CASE else _cl(dy)
    return xd, gd


def _splits(lib, B, H, W, Cin, Cout, R, stride, pad, dil):
    need = lib.oess_conv2d_dilated_wgrad_f32_workspace_bytes(B, H, W, Cin, Cout, R, R, stride, pad, dil)
    return need // (4 * (R * R * Cin * Cout + Cout))


@pytest.mark.parametrize("i", range(len(rc.CONV_CASES)))
def test_dilated_wgrad_f32_matches_float64(i):
    from openess_amd import _lib, hip
    B, Cin, Cout, H, W, R, stride, pad, dil = rc.CONV_CASES[i]
    _, (_, dw64, db64) = rc.conv_case(i)
    xd, gd = _conv_operands(i)
    nsplit = _splits(_lib.load(), *rc.CONV_CASES[i])
    if i == rc.SPLIT_CASE:
        assert nsplit > 1                            # several pixel ranges
    dw, db = hip.conv2d_dilated_wgrad_f32(xd, gd, R, stride, pad, dil)
    assert dw.shape == dw64.shape and db.shape == db64.shape and dw.dtype == db.dtype == torch.float32
    e_w, e_b = relerr(_np(dw), dw64.numpy()), relerr(_np(db), db64.numpy())
    _report(f"wgrad {rc.CONV_CASES[i]} splits {nsplit} dW", e_w, BOUND['wgrad'])
    _report(f"wgrad {rc.CONV_CASES[i]} db", e_b, BOUND['wgrad'])
    assert e_w <= BOUND['wgrad'] and e_b <= BOUND['wgrad']
    if i == rc.CENTRE_TAP_CASE:                      # dilation 12 on a 3 x 4 map: every tap but the centre reads only padding
        off = dw.clone()
        off[:, :, 1, 1] = 0.0
        assert float(dw[:, :, 1, 1].abs().max()) > 0 and int((off != 0).sum()) == 0 and not bool(torch.signbit(off).any())
    dw2, none = hip.conv2d_dilated_wgrad_f32(xd, gd, R, stride, pad, dil, want_db=False)
    assert none is None and torch.equal(dw2, dw)
    dw3, db3 = hip.conv2d_dilated_wgrad_f32(xd, gd, R, stride, pad, dil)
    assert torch.equal(dw3, dw) and torch.equal(db3, db)


@pytest.mark.parametrize("shape", rc.K18_SHAPES)
def test_old_wgrad_entry_equals_the_new_one(shape):
    from openess_amd import _lib, hip
    B, Cin, Cout, H, W, R = shape
    lib = _lib.load()
    g = torch.Generator().manual_seed(sum(shape))
    x, dy = _cl(torch.randn(B, Cin, H, W, generator=g)), _cl(torch.randn(B, Cout, H, W, generator=g))
    pad = (R - 1) // 2
    old = lib.oess_conv2d_wgrad_f32_workspace_bytes(B, H, W, Cin, Cout, R, R, 1, pad, 1)
    assert old > 0 and old == lib.oess_conv2d_dilated_wgrad_f32_workspace_bytes(B, H, W, Cin, Cout, R, R, 1, pad, 1)
    dw0, db0 = hip.conv2d_wgrad_f32(x, dy, R)
    dw1, db1 = hip.conv2d_dilated_wgrad_f32(x, dy, R, 1, pad, 1)
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)


@pytest.mark.parametrize("i", [i for i in range(len(rc.CONV_CASES)) if i != rc.STEM_CASE])
def test_conv2d_dilated_f32_train_gradients_match_float64(i, monkeypatch):
    from openess_amd import hip
    B, Cin, Cout, H, W, R, stride, pad, dil = rc.CONV_CASES[i]
    (x, w, b, dy), (dx64, dw64, db64) = rc.conv_case(i)
    xd, gd = _conv_operands(i)
    xd = xd.detach().requires_grad_(True)
    wp, bp = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = hip.conv2d_dilated_f32_train(xd, wp, bp, stride=stride, pad=pad, dilation=dil)
    y64 = F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad, dilation=dil)
    assert relerr(_np(y), y64.numpy()) <= BOUND['dgrad']

    # every fresh output of the backward is carved out of a NaN-filled parent: an element the kernel does not write shows
    def nan_out(out, B_, C_, H_, W_, device):
        assert out is None
        parent = torch.full((B_, H_ + 2, W_ + 2, C_ + 4), float('nan'), dtype=torch.float32, device=device)
        return parent[:, 1:H_ + 1, 1:W_ + 1, :C_].permute(0, 3, 1, 2)
    monkeypatch.setattr(hip, "_f32_out", nan_out)
    dx, dw, db = torch.autograd.grad(y, [xd, wp, bp], gd)
    monkeypatch.undo()
    assert dx.shape == dx64.shape and dx.dtype == torch.float32 and not bool(torch.isnan(dx).any())
    assert _report(f"dgrad {rc.CONV_CASES[i]}", relerr(_np(dx), dx64.numpy()), BOUND['dgrad']) <= BOUND['dgrad']
    assert relerr(_np(dw), dw64.numpy()) <= BOUND['wgrad'] and relerr(_np(db), db64.numpy()) <= BOUND['wgrad']
    if i in rc.EVEN_1X1_CASES:                       # no window of a 1 x 1 stride-2 conv reads an odd row or column: exact zeros
        assert int((dx[:, :, 1::2] != 0).sum()) == 0 and int((dx[:, :, :, 1::2] != 0).sum()) == 0
        assert float(dx[:, :, 0::2, 0::2].abs().min()) > 0
    # a gradient nobody asks for is not computed
    y2 = hip.conv2d_dilated_f32_train(xd.detach(), wp, None, stride=stride, pad=pad, dilation=dil)
    dw2, = torch.autograd.grad(y2, [wp], gd)
    assert torch.equal(dw2, dw)


def test_stem_weight_gradient_through_autograd_and_cached_operands():
    """the 7 x 7 stem trains through conv2d_dilated_f32_train when x needs no gradient; a PackedWeightF32 keeps the operands"""
    from openess_amd import engine, hip
    B, Cin, Cout, H, W, R, stride, pad, dil = rc.CONV_CASES[rc.STEM_CASE]
    (x, w, b, dy), (_, dw64, _) = rc.conv_case(rc.STEM_CASE)
    wp = w.cuda().requires_grad_(True)
    pw = engine.PackedWeightF32()
    y = hip.conv2d_dilated_f32_train(x.cuda(), wp, None, stride=stride, pad=pad, dilation=dil, pw=pw)      # an NCHW image
    dw, = torch.autograd.grad(y, [wp], _cl(dy))
    assert relerr(_np(dw), dw64.numpy()) <= BOUND['wgrad']
    packed = pw.packed
    hip.conv2d_dilated_f32_train(x.cuda(), wp, None, stride=stride, pad=pad, dilation=dil, pw=pw)
    assert pw.packed is packed                       # same weight version: not packed again
    # the stride-2 data-gradient operand is cached per weight version
    w3 = torch.randn(8, 16, 3, 3, device="cuda", requires_grad=True)
    x3 = torch.randn(1, 16, 6, 6, device="cuda", requires_grad=True)
    pw3 = engine.PackedWeightF32()
    torch.autograd.grad(hip.conv2d_dilated_f32_train(x3, w3, None, stride=2, pad=1, pw=pw3).sum(), [x3])
    first = pw3.packed_dgrad_s2
    assert first is not None and torch.equal(first, hip.pack_conv_weight_f32_dgrad_s2(w3))
    torch.autograd.grad(hip.conv2d_dilated_f32_train(x3, w3, None, stride=2, pad=1, pw=pw3).sum(), [x3])
    assert pw3.packed_dgrad_s2 is first
    with torch.no_grad():
        w3.mul_(2.0)
    torch.autograd.grad(hip.conv2d_dilated_f32_train(x3, w3, None, stride=2, pad=1, pw=pw3).sum(), [x3])
    assert pw3.packed_dgrad_s2 is not first and torch.equal(pw3.packed_dgrad_s2, hip.pack_conv_weight_f32_dgrad_s2(w3))


# ------------------------------------------------------------------------------------------------------------ BatchNorm
def _bn_module(C, gamma, beta):
    bn = nn.BatchNorm2d(C, affine=gamma is not None).cuda().train()
    with torch.no_grad():
        if gamma is not None:
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
        bn.running_mean.copy_(torch.linspace(-1.0, 1.0, C))
        bn.running_var.copy_(torch.linspace(0.5, 2.0, C))
    return bn


def _bn_run(i, variant, affine=True, frozen=False):
    from openess_amd import hip
    (x, gamma, beta, res, dy, relu), want, margin = rc.bn_case(i, variant, affine)
    layout = rc.bn_layout(i, variant)
    C = x.shape[1]
    bn = _bn_module(C, gamma, beta)
    if frozen:
        bn.weight.requires_grad_(False)
        bn.bias.requires_grad_(False)
    xd = _layout(x, layout).detach().requires_grad_(True)
    rd = None if res is None else _layout(res, layout).detach().requires_grad_(True)
    gd = _layout(dy, layout)
    rm0, rv0, n0 = bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)
    y = hip.batch_norm_f32_train(xd, bn, relu=relu, residual=rd)
    rm1, rv1 = bn.running_mean.clone(), bn.running_var.clone()
    assert int(bn.num_batches_tracked) == n0 + 1 and not torch.equal(rm1, rm0) and not torch.equal(rv1, rv0)
    # the running statistics moved exactly one momentum step of torch's rule
    x64 = x.double()
    mean64, var64 = x64.mean((0, 2, 3)), x64.var((0, 2, 3), unbiased=True)
    assert relerr(_np(rm1), (0.9 * rm0.cpu().double() + 0.1 * mean64).numpy()) <= 1e-5
    assert relerr(_np(rv1), (0.9 * rv0.cpu().double() + 0.1 * var64).numpy()) <= 1e-5
    leaves = [xd] + ([bn.weight, bn.bias] if affine and not frozen else []) + ([rd] if rd is not None else [])
    got = torch.autograd.grad(y, leaves, gd, retain_graph=True)
    assert torch.equal(bn.running_mean, rm1) and torch.equal(bn.running_var, rv1) and int(bn.num_batches_tracked) == n0 + 1
    again = torch.autograd.grad(y, leaves, gd)
    for a, b_ in zip(got, again):
        assert torch.equal(a, b_)
    return (x, gamma, beta, res, dy, relu), want, margin, bn, xd, rd, y, got


@pytest.mark.parametrize("variant", rc.BN_VARIANTS)
@pytest.mark.parametrize("i", range(len(rc.BN_SHAPES)))
def test_batch_norm_f32_backward_matches_float64(i, variant):
    from openess_amd import hip
    (x, gamma, beta, res, dy, relu), want, margin, bn, xd, rd, y, got = _bn_run(i, variant)
    if relu:
        assert margin >= RELU_MARGIN, margin
    # the forward is batch_norm_train_f32's, bit for bit
    bn2 = _bn_module(x.shape[1], gamma, beta)
    assert torch.equal(y, hip.batch_norm_train_f32(xd.detach(), bn2, relu=relu, residual=None if rd is None else rd.detach()))
    assert torch.equal(bn2.running_mean, bn.running_mean) and torch.equal(bn2.running_var, bn.running_var)
    assert len(got) == len(want)
    names = ['dx', 'dgamma', 'dbeta'] + (['dres'] if res is not None else [])
    for n, a, b_ in zip(names, got, want):
        assert a.shape == b_.shape and a.dtype == torch.float32
        e = relerr(_np(a), b_.numpy())
        assert _report(f"bn bwd {rc.BN_SHAPES[i]} {variant} {rc.bn_layout(i, variant)} {n}", e, BOUND['bn']) <= BOUND['bn']


def test_batch_norm_f32_backward_without_affine_and_frozen():
    i, variant = 1, 'relu'
    _, want, margin, *_, got = _bn_run(i, variant, affine=False)
    assert margin >= RELU_MARGIN and len(got) == len(want) == 1
    assert _report("bn bwd no affine dx", relerr(_np(got[0]), want[0].numpy()), BOUND['bn']) <= BOUND['bn']
    # frozen gamma / beta still give dx: the bits of the trainable case, and no parameter gradient is computed
    *_, bn, xd, rd, y, got_frozen = _bn_run(i, variant, frozen=True)
    *_, got_full = _bn_run(i, variant)
    assert len(got_frozen) == 1 and torch.equal(got_frozen[0], got_full[0])
    assert bn.weight.grad is None and bn.bias.grad is None
    # a residual's gradient without a ReLU is the incoming gradient itself; with one it is masked
    from openess_amd import hip
    (x, gamma, beta, res, dy, relu), *_ = rc.bn_case(1, 'relu_residual')
    xd, rd, gd = _cl(x).requires_grad_(True), _cl(res).requires_grad_(True), _cl(dy)
    y = hip.batch_norm_f32_train(xd, _bn_module(x.shape[1], gamma, beta), relu=False, residual=rd)
    _, dres = torch.autograd.grad(y, [xd, rd], gd)
    assert torch.equal(dres, gd)
    y = hip.batch_norm_f32_train(xd, _bn_module(x.shape[1], gamma, beta), relu=True, residual=rd)
    dres, = torch.autograd.grad(y, [rd], gd)
    assert torch.equal(dres, torch.where(y > 0, gd, torch.zeros_like(gd)))


# ------------------------------------------------------------------------------------------------------------ max pool
@pytest.mark.parametrize("i", range(len(rc.POOL_SHAPES)))
def test_max_pool_f32_backward(i):
    from openess_amd import hip
    x, dy = rc.pool_case(i)
    assert float((x == 0).float().mean()) > 0.3                      # ties are the common case
    layout = ['nhwc', 'nchw', 'nhwc'][i]
    xd, gd = _layout(x, layout).requires_grad_(True), _layout(dy, layout)
    y = hip.max_pool_3x3s2_f32_train(xd)
    assert torch.equal(y, hip.max_pool_3x3s2_f32(xd.detach())) and torch.equal(y.cpu(), F.max_pool2d(x, 3, 2, 1))
    dx, = torch.autograd.grad(y, [xd], gd)
    assert dx.shape == x.shape and dx.dtype == torch.float32
    e = relerr(_np(dx), rc.pool_grad(x, dy, torch.float64).numpy())
    assert _report(f"pool bwd {rc.POOL_SHAPES[i]}", e, BOUND['pool']) <= BOUND['pool']
    # small-integer cotangent: every sum is exact, so the result is ATen's fp32 result bit for bit (the same winners)
    _, dyi = rc.pool_case(i, integer_dy=True)
    dxi, = torch.autograd.grad(hip.max_pool_3x3s2_f32_train(xd), [xd], _layout(dyi, layout))
    assert torch.equal(dxi.cpu(), rc.pool_grad(x, dyi, torch.float32))


# ------------------------------------------------------------------------------------------------------------ the blocks
def _check_grads(tag, names, got, want, bound):
    worst = 0.0
    for n, a, b_ in zip(names, got, want):
        assert a is not None and tuple(a.shape) == tuple(b_.shape), n
        e = relerr(_np(a), b_.numpy())
        worst = max(worst, e)
        assert e <= bound, (tag, n, e)
    return worst


@pytest.mark.parametrize("i", range(len(rc.BLOCK_CASES)))
def test_bottleneck_forward_fp32_autograd_gradients_match_float64(i):
    from openess_amd.models._resnet import Bottleneck, conv1x1
    kind, B, inplanes, planes, H, W, stride, dilation, down = rc.BLOCK_CASES[i]
    ref, x, dy, names, y64, want, margin = rc.block_case(i)
    assert margin >= RELU_MARGIN, margin
    ds = nn.Sequential(conv1x1(inplanes, planes * 4, stride), nn.BatchNorm2d(planes * 4)) if down else None
    net = Bottleneck(inplanes, planes, stride, ds, dilation=dilation)
    net.load_state_dict(ref.state_dict())
    net = net.cuda().train()
    twin = copy.deepcopy(net)
    xd = _cl(x).requires_grad_(True)
    y = net.forward_fp32_autograd(xd)
    assert torch.equal(y, twin.forward_train_fp32(xd.detach()))              # the forward's bits are the inference path's
    for (n, a), (_, b_) in zip(net.named_buffers(), twin.named_buffers()):
        assert torch.equal(a, b_), n
    assert relerr(_np(y), y64.numpy()) <= BOUND['blocks']
    params = dict(net.named_parameters())
    got = torch.autograd.grad(y, [xd] + [params[n] for n in names], _cl(dy))
    e_x = relerr(_np(got[0]), want[0].numpy())
    assert _report(f"block {kind} dX", e_x, BOUND['blocks']) <= BOUND['blocks']
    worst = _check_grads(f"block {kind}", names, got[1:], want[1:], BOUND['blocks'])
    _report(f"block {kind} parameters", worst, BOUND['blocks'])


# ------------------------------------------------------------------------------------------------------------ the backbone
def _mini_backbone(ref):
    from openess_amd.models._resnet import Bottleneck, ResNet
    net = ResNet(Bottleneck, rc.BACKBONE_LAYERS, replace_stride_with_dilation=rc.BACKBONE_DILATE)
    missing = net.load_state_dict(ref.state_dict(), strict=False)
    assert sorted(missing.missing_keys) == ['fc.bias', 'fc.weight'] and not missing.unexpected_keys
    return net.cuda().train()


def test_backbone_features_fp32_autograd_gradients_match_float64():
    from openess_amd.models._resnet import HipConv2d
    ref, x, dy, names, y64, want, margin = rc.backbone_case()
    assert margin >= RELU_MARGIN, margin
    net = _mini_backbone(ref)
    twin = copy.deepcopy(net)
    xd = x.cuda()
    # the bf16 path before: its output and its operand caches
    with torch.no_grad():
        y16 = net.features(xd).clone()
    convs = [m for m in net.modules() if isinstance(m, HipConv2d)]
    keys16 = [(m._pw.key, m._pw.packed, m._pw_folded.key) for m in convs]
    buffers = {n: b_.clone() for n, b_ in net.named_buffers()}
    twin.load_state_dict(net.state_dict())

    y = net.features_fp32_autograd(xd)
    assert y.dtype == torch.float32 and y.requires_grad
    assert torch.equal(y, twin.features_fp32(xd))                            # identical weights and buffers: identical bits
    for (n, a), (_, b_) in zip(net.named_buffers(), twin.named_buffers()):
        assert torch.equal(a, b_), n
    for n, b_ in net.named_buffers():                                        # one step of every BatchNorm, one batch counted
        if n.endswith('num_batches_tracked'):
            assert int(b_) == int(buffers[n]) + 1, n
    assert _report("backbone output", relerr(_np(y), y64.numpy()), BOUND['backbone']) <= BOUND['backbone']
    params = dict(net.named_parameters())
    assert set(names) == {n for n in params if not n.startswith('fc.')}
    got = torch.autograd.grad(y, [params[n] for n in names], _cl(dy), retain_graph=True)
    worst = _check_grads("backbone", names, got, want[1:], BOUND['backbone'])
    _report("backbone parameter gradients", worst, BOUND['backbone'])
    again = torch.autograd.grad(y, [params[n] for n in names], _cl(dy))
    for n, a, b_ in zip(names, got, again):
        assert torch.equal(a, b_), n
    # the bf16 forward and its caches are untouched by the fp32 forward + backward
    for m, (k, p, kf) in zip(convs, keys16):
        assert m._pw.key == k and m._pw.packed is p and m._pw_folded.key == kf
    with torch.no_grad():
        assert torch.equal(net.features(xd), y16)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_resnet_f32_train_functions_refuse_before_any_launch(monkeypatch):
    from openess_amd import hip
    from openess_amd.models._resnet import Bottleneck, conv_bn_f32_autograd
    x = torch.randn(1, 8, 6, 6, device="cuda")
    w = torch.randn(8, 8, 3, 3, device="cuda", requires_grad=True)
    w7 = torch.randn(8, 8, 7, 7, device="cuda", requires_grad=True)
    bn = nn.BatchNorm2d(8).cuda()
    blk = Bottleneck(8, 2).cuda()

    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(hip._lib, "load", boom)
    with pytest.raises(ValueError, match="fp32"):
        hip.conv2d_dilated_f32_train(x.bfloat16(), w, None, pad=1)
    with pytest.raises(ValueError, match="stride 2 together with dilation"):
        hip.conv2d_dilated_f32_train(x, w, None, stride=2, pad=2, dilation=2)
    with pytest.raises(ValueError, match="7 x 7"):                           # the stem with x.requires_grad
        hip.conv2d_dilated_f32_train(x.clone().requires_grad_(True), w7, None, stride=2, pad=3)
    with pytest.raises(ValueError, match="5 x 5"):
        hip.conv2d_dilated_f32_train(x, torch.randn(8, 8, 5, 5, device="cuda"), None, pad=2)
    with pytest.raises(ValueError, match="stride 3"):
        hip.conv2d_dilated_wgrad_f32(x, x, 3, 3, 1, 1)
    with pytest.raises(ValueError, match="fp32"):
        hip.conv2d_dilated_wgrad_f32(x.bfloat16(), x, 3, 1, 1, 1)
    with pytest.raises(ValueError, match="fp32"):
        hip.batch_norm_f32_train(x.bfloat16(), bn)
    with pytest.raises(NotImplementedError, match="conv_bn_f32"):
        hip.batch_norm_f32_train(x, bn.eval())
    with pytest.raises(NotImplementedError, match="conv_bn_f32"):
        conv_bn_f32_autograd(blk.conv1, blk.bn1.eval(), x)
    bn.train().momentum = None
    with pytest.raises(NotImplementedError, match="momentum"):
        hip.batch_norm_f32_train(x, bn)
    with pytest.raises(ValueError, match="fp32"):
        hip.max_pool_3x3s2_f32_train(x.bfloat16())
    with pytest.raises(ValueError, match="fp32"):
        blk.train().forward_fp32_autograd(x.bfloat16())


def test_resnet_bwd_f32_entry_points_refuse_geometry_on_the_host():
    from openess_amd import _lib
    lib = _lib.load()
    q = lib.oess_conv2d_dilated_wgrad_f32_workspace_bytes
    assert q(2, 33, 47, 64, 32, 3, 3, 2, 1, 1) > 0 and q(2, 19, 23, 3, 64, 7, 7, 2, 3, 1) > 0 and q(2, 3, 4, 256, 64, 3, 3, 1, 12, 12) > 0
    assert q(1, 9, 13, 6, 11, 1, 1, 2, 0, 1) == (6 * 11 + 11) * 4            # 5 x 7 = 35 output pixels: one range
    for bad in ((2, 33, 47, 64, 32, 5, 5, 1, 2, 1),          # R = 5
                (2, 33, 47, 64, 32, 3, 3, 3, 1, 1),          # stride 3
                (2, 33, 47, 64, 32, 3, 3, 1, 64, 64),        # (R - 1) dilation > 127
                (2, 33, 47, 64, 32, 7, 7, 1, 0, 22),         # the same for 7 x 7
                (2, 4, 47, 64, 32, 3, 3, 1, 0, 3),           # Ho < 1
                (2, 33, 47, 64, 32, 3, 1, 1, 1, 1),          # R != S
                (2, 33, 47, 64, 32, 3, 3, 1, -1, 1), (2, 33, 47, 64, 32, 3, 3, 1, 1, 0), (0, 33, 47, 64, 32, 3, 3, 1, 1, 1)):
        assert q(*bad) == 0, bad
        assert lib.oess_conv2d_dilated_wgrad_f32(None, None, *bad, None, None, None, 0, None) == -22
    assert lib.oess_conv2d_dgrad_s2_f32_packed_floats(8, 8, 5) == 0 and lib.oess_conv2d_dgrad_s2_f32_packed_floats(8, 8, 7) == 0
    assert lib.oess_conv2d_dgrad_s2_f32_packed_floats(3, 5, 3) == (16 + 16 + 16 + 16) * 32
    assert lib.oess_conv2d_dgrad_s2_f32_packed_floats(3, 5, 1) == 16 * 32
    assert lib.oess_conv2d_dgrad_s2_f32(None, 1, 8, 8, 8, None, 8, 3, 3, 1, None, None) == -22
    assert lib.oess_batch_norm_bwd_f32_workspace_bytes(0, 4, 4, 8) == 0 and lib.oess_batch_norm_bwd_f32_workspace_bytes(1, 4, 4, 8) > 0
    assert lib.oess_batch_norm_bwd_f32(None, None, None, 1, 4, 4, 8, None, None, 1e-5, None, 0, None, None, None, None, None, 0,
                                       None) == -22
    assert lib.oess_maxpool3x3s2_bwd_f32(None, None, 1, 4, 4, 8, None, None) == -22
