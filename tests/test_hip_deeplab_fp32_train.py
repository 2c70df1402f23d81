"""GPU tests of fp32 DeepLabv3-R50 training (K22: deeplab_bwd_f32.hip, the fp32-output pooling-branch backward of small_ops.hip,
hip.dropout_f32 / hip.aspp_pool_branch_f32, the forward_fp32_autograd methods of models/deeplabv3.py, forward_fp32_train and the
trainers' per-call precision), outputs and gradients against float64 torch autograd on the CPU.  The cases live in
tests/deeplab_fp32_train_cases.py.

Error measure: relerr = max|got - want| / max|want| per tensor.  The bound of a group is four times the largest relerr torch's OWN
fp32 CPU autograd reaches against float64 on that group's cases, with a floor of 1e-5 (the rule of K16 - K21).  Measured on the
CPU by tools/exp_deeplab_fp32_train_bounds.py (CPU_FP32_RELERR below); MI355X: the largest figure this file printed there:

    group      torch fp32 CPU vs float64                         bound      MI355X
    pool       3.58e-06 (dW of 3 x 2048 x 4 x 6)                 1.43e-5    6.66e-6 (dW, 2048 channels)
    head       1.64e-05 (ASPP.convs.4.2.weight, 2048 channels)   6.57e-5    6.12e-6
    model_out  1.07e-05 (logits behind the linear probe)         4.26e-5    1.33e-5 (logits behind the probe; plain 9.3e-6, feats 8.0e-6)
    model      4.61e-05 (classifier.ASPP.project.0.weight)       1.85e-4    6.06e-5

Dropout: the float64 reference multiplies by the mask the product draws, taken from hip.dropout_f32 on ones with the same seed
and a fresh counter on a second module; the keep decisions themselves are held to hip.dropout's (the bf16 kernel), bit for bit.

ReLU masks: every case with a ReLU conditions its seeded input (condition_relu_margin of the K18 test) and the test asserts, on
the float64 reference, that no ReLU input lies below 1e-4 of its layer's largest magnitude before it compares.  No element is
left out of any comparison."""
import copy
import ctypes
import math
import os

import pytest
import torch
import torch.nn as nn

from tests import deeplab_fp32_train_cases as dc
from tests.deeplab_fp32_train_cases import relerr
from tests.synth import damp_residual, fill_by_name

pytestmark = pytest.mark.gpu

CPU_FP32_RELERR = {'pool': 3.582e-6, 'head': 1.643e-5, 'model_out': 1.066e-5, 'model': 4.615e-5}
BOUND = {k: max(4.0 * v, 1e-5) for k, v in CPU_FP32_RELERR.items()}
RELU_MARGIN = dc.RELU_MARGIN
P = dc.DROP_P
CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _np(t):
    return t.detach().cpu().numpy()


def _report(name, value, bound):
    print(f"[deeplab_fp32_train] {name}: {value:.3e} (bound {bound:.2e})", flush=True)
    return value


def _slice_of_wide(t, fill=3.0, lead=8, tail=12):
    """t [B, C, H, W] as a channel slice of a wider channels_last buffer; also returns the parent"""
    B, C, H, W = t.shape
    wide = torch.full((B, H, W, lead + C + tail), fill, device="cuda")
    wide[..., lead:lead + C] = t.permute(0, 2, 3, 1).cuda()
    return wide[..., lead:lead + C].permute(0, 3, 1, 2), wide


def _fresh_owner():
    return nn.Dropout(P)


def _drawn_mask(shape, seed):
    """the mask of the FIRST dropout_f32 call of a fresh module under torch.manual_seed(seed), as float64 0 | 1 / (1 - p) on the CPU"""
    from openess_amd import hip
    torch.manual_seed(seed)
    y = hip.dropout_f32(torch.ones(shape, device="cuda"), P, True, owner=_fresh_owner())
    return (y != 0).double().cpu() / (1.0 - P)


def _check_grads(tag, names, got, want, bound):
    worst = 0.0
    for n, a, b_ in zip(names, got, want):
        if b_ is None:
            assert a is None, n
            continue
        assert a is not None and tuple(a.shape) == tuple(b_.shape) and a.dtype == torch.float32, n
        e = relerr(_np(a), b_.numpy())
        worst = max(worst, e)
        assert e <= bound, (tag, n, e)
    return worst


# ------------------------------------------------------------------------------------------------------------ (a) dropout
DROP_SHAPES = [(2, 8, 3, 5), (3, 256, 9, 13), (1, 264, 5, 7)]


def _drop_input(shape, layout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    x = x + 0.25 * torch.sign(x)                                 # no zeros, also after a bf16 cast: a zero of y is a dropped element
    if layout == 'nhwc':
        return _cl(x), None
    if layout == 'nchw':
        return x.cuda().contiguous(), None
    return _slice_of_wide(x)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("layout", ['nhwc', 'nchw', 'slice'])
@pytest.mark.parametrize("shape", DROP_SHAPES)
def test_dropout_f32_mask_is_the_bf16_kernels(shape, layout, p):
    from openess_amd import _lib, hip
    xd, parent = _drop_input(shape, layout, sum(shape))
    parent0 = None if parent is None else parent.clone()
    seed, count = 1234 + shape[1], 6
    scale = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32, device="cuda")

    def owner():
        m = nn.Dropout(p)
        m._oess_dropout_calls = count
        return m
    torch.manual_seed(seed)
    o32, o16 = owner(), owner()
    xg = xd.detach().requires_grad_(True)
    y = hip.dropout_f32(xg, p, True, owner=o32)
    y16 = hip.dropout(_cl(xd.detach().contiguous()).bfloat16(), p, True, owner=o16)
    assert o32._oess_dropout_calls == o16._oess_dropout_calls == count + 1
    assert y.dtype == torch.float32 and y.shape == xd.shape
    keep = y != 0
    assert torch.equal(keep, y16 != 0)                           # the bf16 kernel's keep decisions, element for element
    assert torch.equal(y, torch.where(keep, xd * scale, torch.zeros_like(xd)))
    assert not bool(torch.signbit(y[~keep]).any())               # a dropped value is +0.0
    if parent is not None:
        assert torch.equal(parent, parent0)
    # backward: the same pattern on the gradient
    gd = _drop_input(shape, layout, sum(shape) + 1)[0]
    gx, = torch.autograd.grad(y, [xg], gd)
    assert torch.equal(gx, torch.where(keep, gd * scale, torch.zeros_like(gd)))
    # the next call of the same module draws another mask; the same counter draws the same
    y2 = hip.dropout_f32(xd, p, True, owner=o32)
    assert o32._oess_dropout_calls == count + 2 and not torch.equal(y2 != 0, keep)
    o32._oess_dropout_calls = count
    assert torch.equal(hip.dropout_f32(xd, p, True, owner=o32), y.detach())
    assert hip.dropout_f32(xd, p, training=False) is xd and hip.dropout_f32(xd, 0.0) is xd
    if layout == 'slice':
        # the entry point in place on the slice: the same values, the parent untouched outside the slice
        B, C, H, W = shape
        v = _lib.F32View(xd.data_ptr(), xd.stride(0), xd.stride(2), xd.stride(3), xd.stride(1))
        rc_ = _lib.load().oess_dropout_f32(ctypes.byref(v), ctypes.byref(v), B, H, W, C, p, seed, (1 << 40) + count + 1, None)
        torch.cuda.synchronize()
        assert rc_ == 0 and torch.equal(xd, y.detach())
        assert torch.equal(parent[..., :8], parent0[..., :8]) and torch.equal(parent[..., 8 + C:], parent0[..., 8 + C:])


def test_dropout_f32_kept_fraction_and_refusals():
    from openess_amd import hip
    shape = DROP_SHAPES[1]
    n = math.prod(shape)
    for p in (0.1, 0.5):
        thr = int(p * 65536 + 0.5)
        torch.manual_seed(77)
        y = hip.dropout_f32(torch.ones(shape, device="cuda"), p, True, owner=nn.Dropout(p))
        frac = float((y != 0).double().mean())
        sigma = math.sqrt(p * (1 - p) / n)
        _report(f"dropout p={p} kept fraction - expected, in sigma", abs(frac - (1 - thr / 65536)) / sigma, 4.0)
        assert abs(frac - (1 - thr / 65536)) <= 4 * sigma
    x = torch.ones(2, 12, 3, 3, device="cuda")
    with pytest.raises(ValueError, match="C % 8"):
        hip.dropout_f32(x, 0.1)
    with pytest.raises(ValueError, match="fp32"):
        hip.dropout_f32(torch.ones(2, 8, 3, 3, device="cuda", dtype=torch.bfloat16), 0.1)


# ------------------------------------------------------------------------------------------------------------ (b) pooling branch
def _pool_modules(ref):
    conv = nn.Conv2d(ref[1].in_channels, dc.POOL_COUT, 1, bias=False)
    bn = nn.BatchNorm2d(dc.POOL_COUT)
    conv.load_state_dict(ref[1].state_dict())
    bn.load_state_dict(ref[2].state_dict())
    return conv.cuda(), bn.cuda().train()


@pytest.mark.parametrize("i", range(len(dc.POOL_CASES)))
def test_aspp_pool_branch_f32_matches_float64(i):
    from openess_amd import hip
    B, Cin, H, W = dc.POOL_CASES[i]
    ref, x, dy, y64, want, buffers64, margin = dc.pool_case(i)
    assert margin >= RELU_MARGIN, margin
    conv, bn = _pool_modules(ref)
    xs, parent = _slice_of_wide(x)
    parent0 = parent.clone()
    xd = xs.detach().requires_grad_(True)
    n0 = int(bn.num_batches_tracked)
    y = hip.aspp_pool_branch_f32(xd, conv, bn)
    assert y.shape == (B, dc.POOL_COUT, H, W) and y.dtype == torch.float32 and y.stride()[2:] == (0, 0)
    assert int(bn.num_batches_tracked) == n0 + 1 and torch.equal(parent, parent0)
    tag = f"pool {dc.POOL_CASES[i]}"
    assert _report(f"{tag} out", relerr(_np(y), y64.numpy()), BOUND['pool']) <= BOUND['pool']
    assert relerr(_np(bn.running_mean), buffers64['2.running_mean'].numpy()) <= 1e-6
    assert relerr(_np(bn.running_var), buffers64['2.running_var'].numpy()) <= 1e-6
    # the cotangent arrives as the last channel slice of the 1280-channel concat gradient
    gwide = torch.full((B, H, W, 1280), 7.0, device="cuda")
    gwide[..., 1024:] = dy.permute(0, 2, 3, 1).cuda()
    gd = gwide[..., 1024:].permute(0, 3, 1, 2)
    got = torch.autograd.grad(y, [xd, conv.weight, bn.weight, bn.bias], gd, retain_graph=True)
    assert got[0].stride()[2:] == (0, 0)                         # the [B, Cin, 1, 1] quotient, expanded
    for n, a, b_ in zip(['dx', 'dW', 'dgamma', 'dbeta'], got, want):
        assert tuple(a.shape) == tuple(b_.shape) and a.dtype == torch.float32, n
        assert _report(f"{tag} {n}", relerr(_np(a.contiguous()), b_.numpy()), BOUND['pool']) <= BOUND['pool']
    again = torch.autograd.grad(y, [xd, conv.weight, bn.weight, bn.bias], gd, retain_graph=True)
    for a, b_ in zip(got, again):
        assert torch.equal(a, b_)
    assert int(bn.num_batches_tracked) == n0 + 1                 # the backward counts no batch
    # a gradient nobody asks for is not returned: frozen parameters still give dx, a frozen producer still trains the branch
    dx_only, = torch.autograd.grad(y, [xd], gd, retain_graph=True)
    assert torch.equal(dx_only, got[0])
    conv2, bn2 = _pool_modules(ref)
    dW2, = torch.autograd.grad(hip.aspp_pool_branch_f32(xs.detach(), conv2, bn2), [conv2.weight], gd)
    assert torch.equal(dW2, got[1])


def test_aspp_pool_branch_f32_refusals():
    from openess_amd import hip
    ref = dc.pool_case(1)[0]
    conv, bn = _pool_modules(ref)
    n0 = int(bn.num_batches_tracked)
    for B in (1, 17):
        with pytest.raises(ValueError, match="2 <= B <= 16"):
            hip.aspp_pool_branch_f32(torch.zeros(B, 64, 3, 4, device="cuda"), conv, bn)
    with pytest.raises(NotImplementedError, match="eval-mode"):
        hip.aspp_pool_branch_f32(torch.zeros(3, 64, 3, 4, device="cuda"), conv, bn.eval())
    with pytest.raises(ValueError, match="fp32"):
        hip.aspp_pool_branch_f32(torch.zeros(3, 64, 3, 4, device="cuda", dtype=torch.bfloat16), conv, bn.train())
    assert int(bn.num_batches_tracked) == n0


# ------------------------------------------------------------------------------------------------------------ (c) the head
HEAD_SEED = 41


def _product_head(ref, i, text_path=None):
    from openess_amd.models.deeplabv3 import DeepLabHead
    B, Cin, H, W, rates = dc.HEAD_CASES[i]
    head = DeepLabHead(text_path, dc.K, Cin, dc.K, list(rates))
    head.load_state_dict(ref.state_dict())
    return head.cuda().train()


def _head_run(head, x, dy):
    """forward + backward of a fresh-counter head under HEAD_SEED: (logits, feat, dx, {name: grad})"""
    torch.manual_seed(HEAD_SEED)
    head.ASPP.project[3]._oess_dropout_calls = 0
    xd = _cl(x).requires_grad_(True)
    logits, feat = head.forward_fp32_autograd({'out': xd})
    for p in head.parameters():
        p.grad = None
    logits.backward(_cl(dy))
    return logits.detach(), feat.detach(), xd.grad, {n: p.grad for n, p in head.named_parameters()}


@pytest.mark.parametrize("i", range(len(dc.HEAD_CASES)))
def test_head_forward_fp32_autograd_matches_float64(i):
    B, Cin, H, W, rates = dc.HEAD_CASES[i]
    mask = _drawn_mask((B, 256, H, W), HEAD_SEED)
    assert 0.0 < float((mask == 0).double().mean()) < 0.2
    ref, x, dy, names, (logits64, feat64), want, margin = dc.head_case(i, mask)
    assert margin >= RELU_MARGIN, margin
    head = _product_head(ref, i)
    counters = {n: int(b_) for n, b_ in head.named_buffers() if n.endswith('num_batches_tracked')}
    logits, feat, dx, grads = _head_run(head, x, dy)
    tag = f"head {dc.HEAD_CASES[i]}"
    assert logits.dtype == feat.dtype == torch.float32 and logits.shape == (B, dc.K, H, W) and feat.shape == (B, 256, H, W)
    assert bool((feat[(mask == 0).cuda()] == 0).all())            # what the drawn mask drops is zero in the product's feature
    assert _report(f"{tag} logits", relerr(_np(logits), logits64.numpy()), BOUND['head']) <= BOUND['head']
    assert _report(f"{tag} feature", relerr(_np(feat), feat64.numpy()), BOUND['head']) <= BOUND['head']
    assert grads['pixel_feature.weight'] is None and want[1 + names.index('pixel_feature.weight')] is None
    assert grads['text_embeddings'] is not None
    worst = _check_grads(tag, ['x'] + names, [dx] + [grads[n] for n in names], want, BOUND['head'])
    _report(f"{tag} worst gradient", worst, BOUND['head'])
    for n, b_ in head.named_buffers():                           # every BatchNorm counted one batch
        if n.endswith('num_batches_tracked'):
            assert int(b_) == counters[n] + 1, n
    # the text embeddings as a buffer (text_embeddings_path=''): no gradient for them, the rest bit for bit
    head_b = _product_head(ref, i, text_path='')
    assert 'text_embeddings' not in dict(head_b.named_parameters()) and not head_b.text_embeddings.requires_grad
    logits_b, feat_b, dx_b, grads_b = _head_run(head_b, x, dy)
    assert head_b.text_embeddings.grad is None and grads_b['pixel_feature.weight'] is None
    assert torch.equal(logits_b, logits) and torch.equal(feat_b, feat) and torch.equal(dx_b, dx)
    for n, g in grads_b.items():
        assert (g is None and grads[n] is None) or torch.equal(g, grads[n]), n
    # eval-mode Dropout: the identity, no counter moved
    head.ASPP.project[3].eval()
    calls = head.ASPP.project[3]._oess_dropout_calls
    with torch.no_grad():
        _, feat_e = head.forward_fp32_autograd({'out': _cl(x)})
    assert head.ASPP.project[3]._oess_dropout_calls == calls and float((feat_e == 0).double().mean()) < 0.9
    kept = feat != 0
    assert relerr(_np(feat_e[kept] * (1.0 / (1.0 - P))), _np(feat[kept])) <= 1e-6


# ------------------------------------------------------------------------------------------------------------ (d) - (f) the model
MODEL_SEED = 43
_MODEL = {}


def _product_model(ref, **kw):
    from openess_amd.models._resnet import Bottleneck, ResNet
    from openess_amd.models.deeplabv3 import DeepLabHead, IntermediateLayerGetter, deeplabv3_resnet50
    net = deeplabv3_resnet50(dc.K, None, 16, '', **kw)
    net.backbone = IntermediateLayerGetter(ResNet(Bottleneck, [1, 1, 1, 2], replace_stride_with_dilation=[False, False, True]),
                                           {'layer4': 'out'})
    net.classifier = DeepLabHead(None, dc.K, 2048, dc.K, list(dc.MODEL_RATES))
    net.load_state_dict(ref.state_dict())
    # the constructor's freezing rules, for the modules put in after it ran
    if kw.get('if_linear_probing'):
        for p in list(net.backbone.parameters()) + list(net.classifier.parameters()):
            p.requires_grad = False
    if kw.get('if_finetuning') and kw.get('frozen_backbone'):
        for p in net.backbone.parameters():
            p.requires_grad = False
    return net.cuda().train()


def _model_run(net, x, dy, want_feats=False):
    torch.manual_seed(MODEL_SEED)
    net.classifier.ASPP.project[3]._oess_dropout_calls = 0
    for p in net.parameters():
        p.grad = None
    logits, feats = net.forward_fp32_train(x.cuda(), want_feats=want_feats)
    logits.backward(_cl(dy))
    return logits.detach(), feats, {n: p.grad for n, p in net.named_parameters()}


def _model_mask():
    if 'mask' not in _MODEL:
        _MODEL['mask'] = _drawn_mask(dc.model_mask_shape(), MODEL_SEED)
    return _MODEL['mask']


def _full_run():
    """the unfrozen model's forward + backward, once for the tests that compare against it"""
    if 'full' not in _MODEL:
        ref, x, dy, *_ = dc.model_case(_model_mask())
        net = _product_model(ref)
        state = copy.deepcopy(net.state_dict())
        _MODEL['full'] = (net, state) + _model_run(net, x, dy)
    return _MODEL['full']


def test_model_forward_fp32_train_matches_float64():
    from openess_amd.models._resnet import Bottleneck, ResNet
    ref, x, dy, names, (logits64, feats64), want, margin = dc.model_case(_model_mask())
    assert margin >= RELU_MARGIN, margin
    net, state, logits, feats, grads = _full_run()
    assert feats is None and logits.dtype == torch.float32 and logits.shape == (3, dc.K, 64, 96)
    assert _report("model logits", relerr(_np(logits), logits64.numpy()), BOUND['model_out']) <= BOUND['model_out']
    assert set(names) == set(grads) and grads['classifier.pixel_feature.weight'] is None
    worst = _check_grads("model", names, [grads[n] for n in names], want[1:], BOUND['model'])
    _report("model worst parameter gradient", worst, BOUND['model'])
    for n, b_ in net.named_buffers():                            # one step of every BatchNorm, one batch counted
        if n.endswith('num_batches_tracked'):
            assert int(b_) == int(state[n]) + 1, n
        elif n.endswith('running_mean'):
            assert not torch.equal(b_, state[n]), n
    # the backbone's feature: ResNet.features_fp32_autograd of the same weights, bit for bit
    twin = ResNet(Bottleneck, [1, 1, 1, 2], replace_stride_with_dilation=[False, False, True])
    missing = twin.load_state_dict({k[len('backbone.'):]: v for k, v in state.items() if k.startswith('backbone.')}, strict=False)
    assert sorted(missing.missing_keys) == ['fc.bias', 'fc.weight'] and not missing.unexpected_keys
    twin = twin.cuda().train()
    net2 = _product_model(ref)
    net2.load_state_dict(state)
    with torch.no_grad():
        assert torch.equal(net2.backbone.forward_fp32_autograd(x.cuda())['out'], twin.features_fp32_autograd(x.cuda()))
    # want_feats: the resized ASPP feature; the logits do not depend on it
    logits_f, feats_f, _ = _model_run(net2, x, dy, want_feats=True)
    assert torch.equal(logits_f, logits) and feats_f.shape == (3, 256, 64, 96) and feats_f.dtype == torch.float32
    assert _report("model feats", relerr(_np(feats_f), feats64.numpy()), BOUND['model_out']) <= BOUND['model_out']


def test_model_forward_fp32_train_repeats_bit_for_bit():
    ref, x, dy, *_ = dc.model_case(_model_mask())
    _, state, logits, _, grads = _full_run()
    net = _product_model(ref)
    net.load_state_dict(state)
    logits2, _, grads2 = _model_run(net, x, dy)
    assert torch.equal(logits2, logits)
    for n, g in grads.items():
        assert (g is None and grads2[n] is None) or torch.equal(g, grads2[n]), n
    # another dropout counter: another mask, other logits
    torch.manual_seed(MODEL_SEED)
    with torch.no_grad():
        assert not torch.equal(net.forward_fp32_train(x.cuda())[0], logits)


def test_model_linear_probe_form():
    mask = _model_mask()
    ref, x, dy, names, (logits64, _), want, margin = dc.model_case(mask, probe=True)
    assert margin >= RELU_MARGIN, margin
    net = _product_model(ref, if_linear_probing=True)
    state = copy.deepcopy(net.state_dict())
    logits, _, grads = _model_run(net, x, dy)
    assert _report("probe logits", relerr(_np(logits), logits64.numpy()), BOUND['model_out']) <= BOUND['model_out']
    assert {n for n, g in grads.items() if g is not None} == {'linear_probe.weight', 'linear_probe.bias'}
    for n in ('linear_probe.weight', 'linear_probe.bias'):
        e = relerr(_np(grads[n]), want[1 + names.index(n)].numpy())
        assert _report(f"probe {n}", e, BOUND['model']) <= BOUND['model']
    moved = [n for n, b_ in net.named_buffers() if n.endswith('running_var') and not torch.equal(b_, state[n])]
    assert len(moved) == sum(n.endswith('running_var') for n in state)          # the frozen network still runs in train mode


def test_model_frozen_backbone_form():
    ref, x, dy, *_ = dc.model_case(_model_mask())
    _, state, logits, _, grads = _full_run()
    net = _product_model(ref, if_finetuning=True, frozen_backbone=True)
    net.load_state_dict(state)
    logits2, _, grads2 = _model_run(net, x, dy)
    assert torch.equal(logits2, logits)
    for n, g in grads2.items():
        if n.startswith('backbone.'):
            assert g is None, n
        else:
            assert (g is None and grads[n] is None) or torch.equal(g, grads[n]), n
    assert sum(g is not None for g in grads2.values()) > 20


# ------------------------------------------------------------------------------------------------------------ (g) the trainers
def _trainer(form, tmp_path):
    import train
    from openess_amd.config.settings import Settings
    train.seed_everything()
    s = Settings(os.path.join(CFG, "finetune_dsec_synthetic.yaml"), generate_log=False)
    assert s.config_option == 'frame2recon'
    s.ckpt_dir = str(tmp_path)
    s.if_finetuning, s.if_linear_probing, s.if_supervised_only = form == 'finetune', form == 'probe', form == 'sup_only'
    trainer, loop = train.build_trainer(s)
    assert loop == 'training' and trainer.train_precision == 'bf16'
    keys = {name: sorted(m.state_dict()) for name, m in trainer.models_dict.items()}
    for name, m in trainer.models_dict.items():
        fill_by_name(m, 300 + len(name))
        damp_residual(m)
    return trainer, s, keys


@pytest.mark.parametrize("form", ['finetune', 'probe', 'sup_only'])
def test_frame2recon_train_step_in_fp32(form, tmp_path):
    from openess_amd import hip
    tr, s, keys = _trainer(form, tmp_path)
    hand, _, _ = _trainer(form, tmp_path)
    assert tr.scaler is None
    K, (H, W) = s.semseg_num_classes, s.img_size_b
    g = torch.Generator().manual_seed(9)
    img = torch.rand(3, 3, H, W, generator=g).cuda()
    gt = torch.randint(0, K, (3, H // 4, W // 4), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2)
    gt[0, :5] = 255                                              # an ignored band
    gt = gt.cuda()
    batch = (None, gt, img, gt, gt, None)
    net = tr.model_recon
    before = {n: t.detach().clone() for n, t in net.state_dict().items()}
    trainable = {n for n, p in net.named_parameters() if p.requires_grad}
    torch.manual_seed(5)
    losses, _, total = tr.train_step(batch, precision='fp32')
    assert set(losses) == {'semseg_recon_loss'} and torch.equal(losses['semseg_recon_loss'], total) and math.isfinite(float(total))
    # the same calls by hand on the twin
    torch.manual_seed(5)
    hand._set_modes()
    logits, feats = hand.model_recon.forward_fp32_train(img)
    assert feats is None and logits.dtype == torch.float32
    loss = hip.task_loss(logits, gt, K, 255, tuple(s.task_loss))[0] * s.weight_task_loss
    loss.backward()
    assert torch.equal(loss.detach(), total)
    n_grads = 0
    for (n, p), (_, q) in zip(net.named_parameters(), hand.model_recon.named_parameters()):
        assert (p.grad is None) == (q.grad is None) == (n not in trainable or n == 'classifier.pixel_feature.weight'), n
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad), n
            n_grads += 1
    assert n_grads == (2 if form == 'probe' else len(trainable) - 1)
    after = net.state_dict()
    for n, p in net.named_parameters():
        if p.grad is not None:
            assert not torch.equal(after[n], before[n]), n       # AdamW moved it
        else:
            assert torch.equal(after[n], before[n]), n
    # buffers: the network runs in train mode in every form, so every BatchNorm keeps stepping its statistics (the reference's
    # trainers do the same); a buffer no kernel writes (the text embeddings) stays
    for n, b_ in net.named_buffers():
        if n.endswith(('running_mean', 'running_var', 'num_batches_tracked')):
            assert not torch.equal(after[n], before[n]), n
        else:
            assert torch.equal(after[n], before[n]), n
    assert tr.scaler is None
    # a bf16 step afterwards runs
    losses16, _, total16 = tr.train_step(batch)
    assert set(losses16) == {'semseg_recon_loss'} and math.isfinite(float(total16))
    assert {name: sorted(m.state_dict()) for name, m in tr.models_dict.items()} == keys
