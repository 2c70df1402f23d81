"""Shared cases of the fp32 DeepLabv3-R50 training tests (K22, tests/test_hip_deeplab_fp32_train.py) and of the CPU measurement
that sets their bounds (tools/exp_deeplab_fp32_train_bounds.py): seeded fp32 inputs, the torch reference in any dtype (float64:
the reference; float32 on the CPU: the yardstick the bounds are four times of) and the ReLU margins.  Nothing here needs a GPU.
Builds on tests/resnet_fp32_cases.py (the mini backbone, randomize_bn, relerr, condition_relu_margin).

Dropout: the reference multiplies the ASPP feature by `mask`, a [B, 256, H, W] tensor of 0 and 1 / (1 - p), in place of
nn.Dropout.  The GPU tests hand in the mask the product draws (hip.dropout_f32 on ones with the same seed and counter); the
bounds tool, which has no GPU, hands in default_mask(): the figures depend on which elements are dropped only through the data."""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import nets as on
from tests import resnet_fp32_cases as rc
from tests.resnet_fp32_cases import RELU_MARGIN, condition_relu_margin, randomize_bn, relerr, relu_margin  # noqa: F401

K = 11                                   # classes
DROP_P = 0.1

# ------------------------------------------------------------------------------------------------------------ pooling branch
POOL_CASES = [(2, 64, 9, 13), (3, 64, 9, 13), (16, 64, 3, 4), (3, 2048, 4, 6)]          # (B, Cin, H, W), Cout = 256
POOL_COUT = 256


def _fp32_params(module):
    for p in module.parameters():
        p.data = p.data.float()
    return module


def _double(m):
    return copy.deepcopy(m).double().train()


def pool_forward(branch, x, pre):
    """oracle.nets.ASPP's pooling branch (AdaptiveAvgPool2d(1), 1 x 1 conv, BatchNorm, ReLU) broadcast over the map"""
    u = branch[2](branch[1](branch[0](x)))
    pre.append(u)
    return torch.relu(u).expand(-1, -1, x.shape[2], x.shape[3])


def grads_of(forward, ref, x, dy, dtype, want_x=True):
    """(outputs, gradients of [x] + named_parameters, None for a parameter the output does not depend on) of
    forward(copy of ref in dtype, x, pre); outputs and cotangents dy are tuples (a None cotangent: that output takes none)"""
    net = copy.deepcopy(ref).to(dtype).train()
    xx = x.to(dtype).requires_grad_(want_x)
    ys = forward(net, xx, [])
    ys = ys if isinstance(ys, tuple) else (ys,)
    dy = dy if isinstance(dy, tuple) else (dy,)
    pairs = [(y, g.to(dtype)) for y, g in zip(ys, dy) if g is not None]
    leaves = ([xx] if want_x else []) + [p for _, p in net.named_parameters()]
    grads = torch.autograd.grad([y for y, _ in pairs], leaves, [g for _, g in pairs], allow_unused=True)
    buffers = {n: b.detach().clone() for n, b in net.named_buffers()}
    return tuple(y.detach() for y in ys), (grads if want_x else (None,) + tuple(grads)), buffers


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def pool_case(i):
    """(fp32-parameter branch, conditioned fp32 x, dy, float64 output, float64 gradients (x, W, gamma, beta), float64 buffers
    after the step, ReLU margin)"""
    def make():
        B, Cin, H, W = POOL_CASES[i]
        torch.manual_seed(2600 + i)
        ref = on.ASPP(Cin, (2, 4, 12)).convs[4]
        randomize_bn(ref, torch.Generator().manual_seed(2610 + i))
        with torch.no_grad():
            ref[2].running_mean.copy_(torch.linspace(-1.0, 1.0, POOL_COUT))
            ref[2].running_var.copy_(torch.linspace(0.5, 2.0, POOL_COUT))
        ref = _fp32_params(ref).train()
        g = torch.Generator().manual_seed(2620 + i)
        x = torch.randn(B, Cin, H, W, generator=g) + 0.5 * torch.randn(B, Cin, 1, 1, generator=g)
        ref64 = _double(ref)

        def run(free):
            pre = []
            pool_forward(ref64, free[0], pre)
            return pre
        x, = condition_relu_margin(run, [x.double()], iters=200)
        margin = relu_margin(run([x]))
        x = x.float()
        dy = torch.randn(B, POOL_COUT, H, W, generator=g)
        (y64,), grads, buffers = grads_of(pool_forward, ref, x, dy, torch.float64)
        return ref, x, dy, y64, grads, buffers, margin
    return _cached(('pool', i), make)


# ------------------------------------------------------------------------------------------------------------ the head
HEAD_CASES = [(3, 64, 9, 13, (2, 4, 12)),        # rate 12 reaches the 9 x 13 map from one column only, rates 2 and 4 from many
              (3, 2048, 4, 6, (2, 3, 6))]        # rate 6 on a 4 x 6 map: the centre tap only


class RefHead(nn.Module):
    """oracle.nets.DeepLabHead for any input width, with the text embeddings as a Parameter (text_embeddings_path=None of the
    product); state_dict keys are the product's."""

    def __init__(self, cin, rates, classes=K):
        super().__init__()
        self.ASPP = on.ASPP(cin, rates)
        self.pixel_feature = nn.Conv2d(256, 512, 3, padding=1, bias=False)
        self.classifier = nn.Sequential(nn.Conv2d(256, 512, 3, padding=1, bias=False), nn.BatchNorm2d(512), nn.ReLU())
        self.text_embeddings = nn.Parameter(0.05 * torch.randn(classes, 512))


def head_forward(head, x, pre, mask):
    """(logits, ASPP feature after the dropout mask) of the head, recording every ReLU input in `pre`"""
    def cbr(conv, bn, t):
        u = bn(conv(t))
        pre.append(u)
        return torch.relu(u)
    a = head.ASPP
    res = [cbr(c[0], c[1], x) for c in a.convs[:4]] + [pool_forward(a.convs[4], x, pre)]
    feat = cbr(a.project[0], a.project[1], torch.cat(res, 1)) * mask.to(x.dtype)
    y = cbr(head.classifier[0], head.classifier[1], feat)
    return F.conv2d(y, head.text_embeddings[:, :, None, None]), feat


def default_mask(shape, seed=2700):
    """a seeded Bernoulli(1 - DROP_P) mask scaled by 1 / (1 - DROP_P), float64"""
    keep = torch.rand(shape, generator=torch.Generator().manual_seed(seed)) >= DROP_P
    return keep.double() / (1.0 - DROP_P)


def _mask_key(mask):
    return hash(mask.numpy().tobytes())


def head_case(i, mask=None):
    """(fp32-parameter head, conditioned fp32 x, (dlogits, dfeat=None), parameter names, float64 (logits, feat), float64
    gradients (x, then the parameters; None for pixel_feature.weight), ReLU margin); mask: [B, 256, H, W] of 0 and 1 / (1 - p)"""
    B, Cin, H, W, rates = HEAD_CASES[i]
    mask = default_mask((B, 256, H, W), 2700 + i) if mask is None else mask.double()

    def make():
        torch.manual_seed(2630 + i)
        ref = RefHead(Cin, rates)
        randomize_bn(ref, torch.Generator().manual_seed(2640 + i))
        ref = _fp32_params(ref).train()
        g = torch.Generator().manual_seed(2650 + i)
        x = torch.relu(torch.randn(B, Cin, H, W, generator=g))                  # what layer4 hands over: a post-ReLU map
        ref64 = _double(ref)

        def run(free):
            pre = []
            head_forward(ref64, free[0], pre, mask)
            return pre
        x, = condition_relu_margin(run, [x.double()], iters=400)
        margin = relu_margin(run([x]))
        x = x.float()
        dy = torch.randn(B, K, H, W, generator=g)
        fwd = lambda net, t, pre: head_forward(net, t, pre, mask)               # noqa: E731
        ys, grads, _ = grads_of(fwd, ref, x, (dy, None), torch.float64)
        return ref, x, dy, [n for n, _ in ref.named_parameters()], ys, grads, margin
    return _cached(('head', i, _mask_key(mask)), make)


def head_grads_fp32(i, mask=None):
    """torch's own fp32 CPU run of head_case(i, mask): ((logits, feat), gradients)"""
    B, Cin, H, W, rates = HEAD_CASES[i]
    mask = default_mask((B, 256, H, W), 2700 + i) if mask is None else mask.double()
    ref, x, dy, *_ = head_case(i, mask)
    ys, grads, _ = grads_of(lambda net, t, pre: head_forward(net, t, pre, mask), ref, x, (dy, None), torch.float32)
    return ys, grads


# ------------------------------------------------------------------------------------------------------------ the whole model
MODEL_INPUT, MODEL_RATES = (3, 3, 64, 96), (2, 3, 6)            # output stride 16: a 4 x 6 map under the head


class RefModel(nn.Module):
    """the mini dilated backbone (tests/resnet_fp32_cases.MiniResNet) under RefHead, [+ the K x K linear probe]; state_dict keys
    are the product's"""

    def __init__(self, probe=False):
        super().__init__()
        self.backbone = rc.MiniResNet()
        self.classifier = RefHead(2048, MODEL_RATES)
        if probe:
            self.linear_probe = nn.Conv2d(K, K, 1)


def model_forward(net, x, pre, mask):
    """(full-size logits, full-size ASPP feature) as deeplabv3_resnet50.forward composes them"""
    size = x.shape[-2:]
    logits, feat = head_forward(net.classifier, rc.backbone_forward(net.backbone, x, pre), pre, mask)
    logits = F.interpolate(logits, size=size, mode='bilinear', align_corners=False)
    if hasattr(net, 'linear_probe'):
        logits = net.linear_probe(logits)
    return logits, F.interpolate(feat, size=size, mode='bilinear', align_corners=False)


def backbone_only_forward(net, x):
    return rc.backbone_forward(net.backbone, x, [])


def _model_base(mask):
    def make():
        torch.manual_seed(2660)
        ref = RefModel(probe=True)                              # the probe's weights exist in both forms; only one form uses them
        randomize_bn(ref, torch.Generator().manual_seed(2661))
        ref = _fp32_params(ref).train()
        g = torch.Generator().manual_seed(2662)
        x = torch.rand(MODEL_INPUT, generator=g)
        ref64 = _double(ref)

        def run(free):
            pre = []
            model_forward(ref64, free[0], pre, mask)
            return pre
        x, = condition_relu_margin(run, [x.double()], iters=400)
        margin = relu_margin(run([x]))
        dy = torch.randn(MODEL_INPUT[0], K, MODEL_INPUT[2], MODEL_INPUT[3], generator=g)
        return ref, x.float(), dy, margin
    return _cached(('model_base', _mask_key(mask)), make)


def model_mask_shape():
    B, _, H, W = MODEL_INPUT
    return (B, 256, H // 16, W // 16)


def _plain(ref, probe):
    """ref with or without its linear probe"""
    if probe:
        return ref
    net = copy.deepcopy(ref)
    del net.linear_probe
    return net


def model_case(mask=None, probe=False, dtype=torch.float64):
    """(fp32-parameter model, conditioned fp32 image, dlogits, parameter names, (logits, feats) in dtype, gradients in dtype
    (None first: the image takes none; then the parameters), ReLU margin).  probe: the logits pass the K x K linear probe."""
    mask = default_mask(model_mask_shape(), 2710) if mask is None else mask.double()
    base, x, dy, margin = _model_base(mask)

    def make():
        ref = _plain(base, probe)
        ys, grads, _ = grads_of(lambda net, t, pre: model_forward(net, t, pre, mask), ref, x, (dy, None), dtype, want_x=False)
        return ref, x, dy, [n for n, _ in ref.named_parameters()], ys, grads, margin
    return _cached(('model', _mask_key(mask), probe, dtype), make)
