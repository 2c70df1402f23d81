"""Shared cases of the fp32 ResNet-50 backward tests (K21, tests/test_hip_resnet_fp32_train.py) and of the CPU measurement that
sets their bounds (tools/exp_resnet_fp32_bounds.py): seeded fp32 inputs, the torch reference in any dtype (float64: the
reference; float32 on the CPU: the yardstick the bounds are four times of) and the error measure.  Nothing here needs a GPU.

ReLU masks: every case with a ReLU conditions its seeded input (condition_relu_margin of the K18 test) so that, on the float64
side, no ReLU input lies below RELU_MARGIN of its layer's largest magnitude; the margin is returned and the tests assert it."""
import functools

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import nets as on
from tests.test_hip_semseg_fp32_train import RELU_MARGIN, condition_relu_margin, relu_margin

EPS = 1e-5


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ------------------------------------------------------------------------------------------------------------ convolution
# (B, Cin, Cout, H, W, R, stride, pad, dilation)
CONV_CASES = [(2, 32, 16, 9, 13, 3, 2, 1, 1), (1, 16, 33, 8, 12, 3, 2, 1, 1), (2, 64, 128, 7, 10, 1, 2, 0, 1),
              (2, 3, 64, 19, 23, 7, 2, 3, 1),          # the stem
              (2, 64, 32, 6, 10, 3, 1, 2, 2), (1, 128, 64, 5, 7, 3, 1, 4, 4),
              (2, 256, 64, 3, 4, 3, 1, 12, 12),        # only the centre tap touches the map
              (2, 64, 32, 33, 47, 3, 2, 1, 1),         # several pixel ranges
              (1, 16, 32, 6, 8, 1, 2, 0, 1),           # 1 x 1 stride 2 on an even map: odd rows and columns get no gradient
              (1, 16, 16, 8, 9, 3, 2, 0, 1)]           # pad 0: a last row beyond the last window
STEM_CASE, CENTRE_TAP_CASE, SPLIT_CASE, X_SLICE_CASE, DY_NCHW_CASE = 3, 6, 7, 0, 4
EVEN_1X1_CASES = (2, 8)
K18_SHAPES = [(2, 32, 16, 5, 7, 3), (2, 64, 32, 33, 47, 3), (1, 6, 11, 9, 13, 1)]        # (B, Cin, Cout, H, W, R): stride 1, 'same'


def conv_grads(x, w, b, dy, stride, pad, dilation, dtype, want_dx=True):
    """(dx | None, dw, db) of y = conv(x, w) + b with cotangent dy, by torch autograd in `dtype` on the CPU"""
    x, w, b = (t.to(dtype).requires_grad_(True) for t in (x, w, b))
    y = F.conv2d(x, w, b, stride=stride, padding=pad, dilation=dilation)
    g = torch.autograd.grad(y, [x, w, b] if want_dx else [w, b], dy.to(dtype))
    return g if want_dx else (None,) + tuple(g)


@functools.lru_cache(maxsize=None)
def conv_case(i):
    """fp32 inputs (x, w, b, dy) and the float64 gradients (dx, dw, db) of case i"""
    B, Cin, Cout, H, W, R, stride, pad, dil = CONV_CASES[i]
    g = torch.Generator().manual_seed(2100 + i)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, R, R, generator=g) / (Cin * R * R) ** 0.5
    b = torch.randn(Cout, generator=g)
    Ho, Wo = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1, (W + 2 * pad - dil * (R - 1) - 1) // stride + 1
    dy = torch.randn(B, Cout, Ho, Wo, generator=g)
    return (x, w, b, dy), conv_grads(x, w, b, dy, stride, pad, dil, torch.float64)


# ------------------------------------------------------------------------------------------------------------ BatchNorm
BN_SHAPES = [(2, 6, 7, 9), (2, 64, 5, 8), (1, 256, 3, 5), (2, 2048, 2, 3), (3, 64, 33, 47)]
BN_VARIANTS = ['plain', 'relu', 'relu_residual']
BN_LAYOUTS = ['nhwc', 'nchw', 'slice']
BN_OFFSET_SHAPE = 1                      # this shape's input sits on a per-channel offset of +50: cancellation


def bn_layout(i, variant):
    return BN_LAYOUTS[(i + BN_VARIANTS.index(variant)) % 3]


def bn_forward(x, gamma, beta, res, relu, pre=None):
    y = F.batch_norm(x, None, None, gamma, beta, True, 0.1, EPS)
    if res is not None:
        y = y + res
    if relu:
        if pre is not None:
            pre.append(y)
        y = torch.relu(y)
    return y


def bn_grads(x, gamma, beta, res, dy, relu, dtype):
    """gradients of (x, gamma, beta, residual) (those that exist, in this order) in `dtype`"""
    leaves = [t.to(dtype).requires_grad_(True) for t in (x, gamma, beta, res) if t is not None]
    it = iter(leaves)
    xx = next(it)
    gg = next(it) if gamma is not None else None
    bb = next(it) if beta is not None else None
    rr = next(it) if res is not None else None
    return torch.autograd.grad(bn_forward(xx, gg, bb, rr, relu), leaves, dy.to(dtype))


@functools.lru_cache(maxsize=None)
def bn_case(i, variant, affine=True):
    """fp32 inputs (x, gamma, beta, res, dy, relu), the float64 gradients and the ReLU margin (None without a ReLU)"""
    B, C, H, W = BN_SHAPES[i]
    g = torch.Generator().manual_seed(2200 + 10 * i + BN_VARIANTS.index(variant))
    x = torch.randn(B, C, H, W, generator=g) * (0.5 + torch.rand(1, C, 1, 1, generator=g))
    if i == BN_OFFSET_SHAPE:
        x = x + 50.0
    gamma = 0.5 + torch.rand(C, generator=g) if affine else None
    beta = 0.3 * torch.randn(C, generator=g) if affine else None
    res = torch.randn(B, C, H, W, generator=g) if variant == 'relu_residual' else None
    dy = torch.randn(B, C, H, W, generator=g)
    relu = variant != 'plain'
    margin = None
    if relu:
        dd = lambda t: None if t is None else t.double()                         # noqa: E731

        def run(free):
            pre = []
            bn_forward(free[0], dd(gamma), dd(beta), dd(res), True, pre)
            return pre
        x, = condition_relu_margin(run, [x.double()])
        margin = relu_margin(run([x]))
        x = x.float()
    return (x, gamma, beta, res, dy, relu), bn_grads(x, gamma, beta, res, dy, relu, torch.float64), margin


# ------------------------------------------------------------------------------------------------------------ max pool
POOL_SHAPES = [(2, 8, 7, 9), (1, 6, 8, 12), (2, 64, 33, 47)]


@functools.lru_cache(maxsize=None)
def pool_case(i, integer_dy=False):
    """a post-ReLU map with many exact zeros and repeated values (ties are the common case), and a cotangent"""
    B, C, H, W = POOL_SHAPES[i]
    g = torch.Generator().manual_seed(2300 + i)
    x = torch.relu(torch.randint(-3, 4, (B, C, H, W), generator=g).float() * 0.25)
    x = torch.where(torch.rand(B, C, H, W, generator=g) > 0.8, torch.relu(torch.randn(B, C, H, W, generator=g)), x)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randint(-4, 5, (B, C, Ho, Wo), generator=g).float() if integer_dy else torch.randn(B, C, Ho, Wo, generator=g)
    return x, dy


def pool_grad(x, dy, dtype):
    x = x.to(dtype).requires_grad_(True)
    return torch.autograd.grad(F.max_pool2d(x, 3, 2, 1), [x], dy.to(dtype))[0]


# ------------------------------------------------------------------------------------------------------------ the blocks
# (kind, B, inplanes, planes, H, W, stride, dilation, downsample)
BLOCK_CASES = [('plain', 2, 128, 32, 6, 10, 1, 1, False), ('stride2', 2, 64, 32, 9, 13, 2, 1, True),
               ('dilation2', 2, 64, 32, 6, 10, 1, 2, True), ('dilation4', 2, 256, 64, 5, 7, 1, 4, False)]


def randomize_bn(module, gen):
    """gamma in [0.5, 1.5], beta ~ 0.3 N on every BatchNorm (fp32-representable)"""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=gen))
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=gen))


def block_forward(blk, x, pre):
    """oracle.nets.Bottleneck.forward, recording every ReLU input in `pre`"""
    def relu(t):
        pre.append(t)
        return torch.relu(t)
    out = relu(blk.bn1(blk.conv1(x)))
    out = relu(blk.bn2(blk.conv2(out)))
    out = blk.bn3(blk.conv3(out))
    identity = x if blk.downsample is None else blk.downsample(x)
    return relu(out + identity)


def _fp32_params(module):
    for p in module.parameters():
        p.data = p.data.float()
    return module


def make_block(i, seed):
    kind, B, inplanes, planes, H, W, stride, dilation, down = BLOCK_CASES[i]
    torch.manual_seed(seed)
    ds = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4)) if down else None
    ref = on.Bottleneck(inplanes, planes, stride, ds, dilation)
    randomize_bn(ref, torch.Generator().manual_seed(seed + 1))
    return _fp32_params(ref).train()


def net_grads(forward, ref, x, dy, dtype):
    """y and the gradients (x, then the parameters in named_parameters order) of forward(ref copy in dtype, x)"""
    import copy
    net = copy.deepcopy(ref).to(dtype).train()
    xx = x.to(dtype).requires_grad_(True)
    y = forward(net, xx, [])
    grads = torch.autograd.grad(y, [xx] + [p for _, p in net.named_parameters()], dy.to(dtype))
    return y.detach(), grads


@functools.lru_cache(maxsize=None)
def block_case(i, seed=0):
    """(fp32-parameter oracle block, conditioned fp32 x, dy, parameter names, float64 output, float64 gradients, ReLU margin)"""
    kind, B, inplanes, planes, H, W, stride, dilation, down = BLOCK_CASES[i]
    ref = make_block(i, 2400 + 10 * i + 100 * seed)
    g = torch.Generator().manual_seed(2450 + 10 * i + 100 * seed)
    x = torch.randn(B, inplanes, H, W, generator=g)
    ref64 = _double_copy(ref)

    def run(free):
        pre = []
        block_forward(ref64, free[0], pre)
        return pre
    x, = condition_relu_margin(run, [x.double()], iters=200)
    margin = relu_margin(run([x]))
    x = x.float()
    with torch.no_grad():
        shape = block_forward(ref64, x.double(), []).shape
    dy = torch.randn(shape, generator=g)
    y64, grads = net_grads(block_forward, ref, x, dy, torch.float64)
    return ref, x, dy, [n for n, _ in ref.named_parameters()], y64, grads, margin


def _double_copy(m):
    import copy
    return copy.deepcopy(m).double().train()


# ------------------------------------------------------------------------------------------------------------ the backbone
BACKBONE_LAYERS, BACKBONE_DILATE, BACKBONE_INPUT = [1, 1, 1, 2], [False, False, True], (2, 3, 32, 48)


class MiniResNet(nn.Module):
    """oracle.nets.ResNet50 with BACKBONE_LAYERS blocks per layer: the reference of ResNet(Bottleneck, [1, 1, 1, 2],
    replace_stride_with_dilation=[False, False, True]); state_dict keys are the product's (without fc)."""

    def __init__(self):
        super().__init__()
        self.inplanes, self.dilation = 64, 1
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        make = on.ResNet50._make_layer
        self.layer1 = make(self, 64, BACKBONE_LAYERS[0])
        self.layer2 = make(self, 128, BACKBONE_LAYERS[1], 2, BACKBONE_DILATE[0])
        self.layer3 = make(self, 256, BACKBONE_LAYERS[2], 2, BACKBONE_DILATE[1])
        self.layer4 = make(self, 512, BACKBONE_LAYERS[3], 2, BACKBONE_DILATE[2])
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')


def backbone_forward(net, x, pre):
    t = net.bn1(net.conv1(x))
    pre.append(t)
    x = net.maxpool(torch.relu(t))
    for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
        for blk in layer:
            x = block_forward(blk, x, pre)
    return x


@functools.lru_cache(maxsize=None)
def backbone_case(seed=0):
    """(fp32-parameter reference, conditioned fp32 image, dy, parameter names, float64 output, float64 gradients, ReLU margin)"""
    torch.manual_seed(2500 + seed)
    ref = MiniResNet()
    randomize_bn(ref, torch.Generator().manual_seed(2501 + seed))
    ref = _fp32_params(ref).train()
    g = torch.Generator().manual_seed(2502 + seed)
    x = torch.rand(BACKBONE_INPUT, generator=g)
    ref64 = _double_copy(ref)

    def run(free):
        pre = []
        backbone_forward(ref64, free[0], pre)
        return pre
    x, = condition_relu_margin(run, [x.double()], iters=200)
    margin = relu_margin(run([x]))
    x = x.float()
    with torch.no_grad():
        shape = backbone_forward(ref64, x.double(), []).shape
    dy = torch.randn(shape, generator=g)
    y64, grads = net_grads(backbone_forward, ref, x, dy, torch.float64)
    return ref, x, dy, [n for n, _ in ref.named_parameters()], y64, grads, margin
