"""Mirror of models/_resnet.py (ResNet :117-209, Bottleneck :74-114, resnet50) with the convolutions
on the HIP MFMA kernel.  state_dict keys equal torchvision's / the reference's."""
from collections import OrderedDict
from typing import Callable, NamedTuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import engine, hip


class HipConv2d(nn.Conv2d):
    """nn.Conv2d (bias-free in ResNet) executed by the MFMA kernel; differentiable when its weight
    requires grad, plain inference otherwise."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self._pw = engine.PackedWeight()
        self._pw_folded = engine.PackedWeight()      # eval-mode BatchNorm folded in
        self._pw32 = engine.PackedWeightF32()        # the same in fp32 (conv_bn_f32)
        self._pw32_plain = engine.PackedWeightF32()  # fp32 without a fold (conv_bn_train_f32, the teacher's decoder)
        self._pw32_train = engine.PackedWeightF32()  # fp32 training operands (conv_bn_f32_autograd)

    def forward(self, x):
        if x.shape[1] % 8 or x.dtype != torch.bfloat16:
            x = engine.to_cl_bf16(x)
        elif x.stride(1) != 1:                       # e.g. torch.cat of an expanded tensor: make it NHWC
            x = x.contiguous(memory_format=torch.channels_last)
        k, s, p, d = self.kernel_size[0], self.stride[0], self.padding[0], self.dilation[0]
        if torch.is_grad_enabled() and (self.weight.requires_grad or x.requires_grad):
            return engine.conv2d_train(x, self.weight, self.bias, self._pw, k, s, p, d)
        pw = self._pw.get(self.weight, self.bias, None, cin_pad=x.shape[1])
        return engine.conv2d_infer(x, pw, self.out_channels, k, s, p, d)


class HipMaxPool2d(nn.MaxPool2d):
    """nn.MaxPool2d(3, stride=2, padding=1) of the stem on the HIP kernel (forward and backward; ATen's tie rule)."""

    def forward(self, x):
        if x.is_cuda and (self.kernel_size, self.stride, self.padding, self.dilation, self.ceil_mode) == (3, 2, 1, 1, False):
            if x.dtype != torch.bfloat16 or x.stride(1) != 1 or x.shape[1] % 8:
                x = engine.to_cl_bf16(x)
            return hip.max_pool_3x3s2(x)
        return super().forward(x)


def conv_bn_separable(conv, bn, x):
    """True where conv_bn(conv, bn, x) runs as conv + BatchNorm finalize + apply pass with scale / shift in memory in between:
    no autograd, train-mode BatchNorm, bias-free conv, and a map too large for the one-launch statistics + apply kernel
    (hip.conv_bn_train_separate_apply).  Only there does conv_bn take defer / residual_affine / want_output=False; every other
    route (autograd, eval-mode fold, small maps) has no apply pass of its own to move."""
    if torch.is_grad_enabled() and (conv.weight.requires_grad or x.requires_grad or bn.weight.requires_grad):
        return False
    if conv.bias is not None or not bn.training or not x.is_cuda:
        return False
    k, s, p, d = conv.kernel_size[0], conv.stride[0], conv.padding[0], conv.dilation[0]
    B, _, H, W = x.shape
    Ho, Wo = (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1
    return hip.conv_bn_train_separate_apply(B * Ho * Wo, conv.out_channels)


def conv_bn(conv, bn, x, relu=False, residual=None, out=None, skip_in=None, skip_out=None, defer=False, residual_affine=None,
            want_output=True):
    """conv -> BatchNorm2d [-> + residual] [-> ReLU] with nn.BatchNorm2d semantics for both bn.training states.
    No autograd needed (frozen teacher, validation): train-mode BN takes its batch statistics from the conv
    epilogue (no statistics pass); eval-mode BN is folded into the packed weights and the whole tail is the
    conv epilogue.  With autograd: MFMA conv + library BatchNorm.
    defer / residual_affine / want_output: the forms of hip.conv_bn_train_nhwc, legal where conv_bn_separable() holds."""
    if (defer or residual_affine is not None or not want_output) and not conv_bn_separable(conv, bn, x):
        raise ValueError("conv_bn: defer / residual_affine / want_output=False need the separate-apply route (conv_bn_separable)")
    needs_grad = torch.is_grad_enabled() and (conv.weight.requires_grad or x.requires_grad or bn.weight.requires_grad)
    if needs_grad and conv.bias is None and bn.training and bn.weight is not None and bn.running_mean is not None and \
            conv.out_channels % 8 == 0 and conv.out_channels <= 2048:
        # one autograd node: statistics from the conv epilogue (no statistics pass), fused BatchNorm backward
        if x.shape[1] % 8 or x.dtype != torch.bfloat16:
            x = engine.to_cl_bf16(x)
        elif x.stride(1) != 1:
            x = x.contiguous(memory_format=torch.channels_last)
        y = engine.conv_bn_train(x, conv, bn, conv._pw, relu=relu, residual=residual, skip_in=skip_in, skip_out=skip_out)
        if out is not None:
            out.copy_(y)
            return out
        return y
    if needs_grad or conv.bias is not None:
        y = engine.batch_norm_act(conv(x), bn, relu=relu, residual=residual)
        if out is not None:
            out.copy_(y)
            return out
        return y
    if x.shape[1] % 8 or x.dtype != torch.bfloat16:
        x = engine.to_cl_bf16(x)
    elif x.stride(1) != 1:
        x = x.contiguous(memory_format=torch.channels_last)
    if residual is not None and (residual.stride(1) != 1 or residual.dtype != torch.bfloat16):
        residual = residual.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    k, s, p, d = conv.kernel_size[0], conv.stride[0], conv.padding[0], conv.dilation[0]
    if bn.training:
        pw = conv._pw.get(conv.weight, None, None, cin_pad=x.shape[1])
        y = hip.conv_bn_train_nhwc(engine.nhwc(x), pw.packed, conv.out_channels, k, k, s, p, d, bn, relu=relu,
                                   residual=None if residual is None else engine.nhwc(residual),
                                   out=None if out is None else engine.nhwc(out), defer=defer, residual_affine=residual_affine,
                                   want_output=want_output)
        if y is None or defer:                       # nothing to read / hip.RawBN (NHWC) for residual_affine or the stem's pool
            return y
        return engine.from_nhwc(y)
    pw = conv._pw_folded.get(conv.weight, None, bn, cin_pad=x.shape[1])
    return engine.conv2d_infer(x, pw, conv.out_channels, k, s, p, d, relu=relu, residual=residual, out=out)


def fold_conv_bn_f64(conv, bn):
    """(weight, bias) in float64 of conv -> eval-mode BatchNorm2d as ONE conv: what PackedWeightF32.get rounds once to fp32."""
    return engine.fold_bn(conv.weight.detach().double(), None if conv.bias is None else conv.bias.detach().double(), bn)


def conv_bn_f32(conv, bn, x, relu=False, residual=None, out=None, pw=None):
    """conv -> eval-mode BatchNorm2d [-> + residual] [-> ReLU] in fp32, one launch (hip.conv2d_f32): the BatchNorm is folded into
    the weight and bias in float64 and rounded once; the operand is cached per parameter and running-statistic versions
    (engine.PackedWeightF32), so a training step between two validations re-packs it and an unchanged model does not.
    x, residual, out: logical [B, C, H, W] fp32 tensors, any strides.  pw: the cache of a conv that is not a HipConv2d."""
    if bn.training or bn.running_mean is None:
        raise NotImplementedError("fp32 inference folds BatchNorm's running statistics: train-mode BatchNorm is not built")
    op = (conv._pw32 if pw is None else pw).get(conv.weight, conv.bias, bn)
    (R, S), s, p, d = conv.kernel_size, conv.stride[0], conv.padding[0], conv.dilation[0]
    return hip.conv2d_f32(x, op.packed, op.bias, conv.out_channels, R, S, stride=s, pad=p, act='relu' if relu else None,
                          residual=residual, out=out, dilation=d)


def conv_f32(conv, x, relu=False, out=None):
    """The plain fp32 convolution (+ bias) of a HipConv2d through its un-folded operand cache."""
    op = conv._pw32_plain.get(conv.weight, conv.bias, None)
    (R, S), s, p, d = conv.kernel_size, conv.stride[0], conv.padding[0], conv.dilation[0]
    return hip.conv2d_f32(x, op.packed, op.bias, conv.out_channels, R, S, stride=s, pad=p, act='relu' if relu else None, out=out,
                          dilation=d)


def conv_bn_train_f32(conv, bn, x, relu=False, residual=None):
    """conv -> train-mode BatchNorm2d [-> + residual] [-> ReLU] in fp32 (the reference's frozen teacher stays in .train()): the
    plain convolution, then hip.batch_norm_train_f32 in place on its output: batch statistics, the running statistics moved one
    momentum step.  x, residual: logical [B, C, H, W] fp32 tensors, any strides.  No autograd."""
    if not bn.training:
        raise ValueError("conv_bn_train_f32 is the batch-statistics form: an eval-mode BatchNorm folds (conv_bn_f32)")
    y = conv_f32(conv, x)
    return hip.batch_norm_train_f32(y, bn, relu=relu, residual=residual, out=y)


def conv_bn_any_f32(conv, bn, x, relu=False, residual=None):
    """conv_bn_train_f32 or conv_bn_f32, as bn.training says: nn.BatchNorm2d's own rule."""
    return (conv_bn_train_f32 if bn.training else conv_bn_f32)(conv, bn, x, relu=relu, residual=residual)


def conv_bn_f32_autograd(conv, bn, x, relu=False, residual=None):
    """conv -> train-mode BatchNorm2d [-> + residual] [-> ReLU] in fp32 WITH autograd (K21): hip.conv2d_dilated_f32_train, then
    hip.batch_norm_f32_train.  The forward's bits are conv_bn_train_f32's.  An eval-mode BatchNorm is refused (conv_bn_f32)."""
    if not bn.training:
        raise NotImplementedError("conv_bn_f32_autograd is the batch-statistics form: an eval-mode BatchNorm folds (conv_bn_f32)")
    y = hip.conv2d_dilated_f32_train(x, conv.weight, conv.bias, stride=conv.stride[0], pad=conv.padding[0], dilation=conv.dilation[0],
                                     pw=conv._pw32_train)
    return hip.batch_norm_f32_train(y, bn, relu=relu, residual=residual)


class F32Layers(NamedTuple):
    """The per-layer functions of one mode of the fp32 network: what walk_f32 and Bottleneck.forward_f32 call."""
    conv_bn: Callable      # (conv, bn, x, relu=False, residual=None) -> y
    max_pool: Callable     # (x) -> y


F32_EVAL = F32Layers(conv_bn_f32, hip.max_pool_3x3s2_f32)                           # BatchNorm folded; no autograd
F32_AS_FLAGGED = F32Layers(conv_bn_any_f32, hip.max_pool_3x3s2_f32)                 # per BatchNorm as bn.training says; no autograd
F32_AUTOGRAD = F32Layers(conv_bn_f32_autograd, hip.max_pool_3x3s2_f32_train)        # train-mode BatchNorm with autograd (K21)


def walk_f32(net, x, layers, return_layers=()):
    """THE fp32 walk over a ResNet, or over the IntermediateLayerGetter that holds its first children: stem conv + BatchNorm +
    ReLU, max pool, then every block of layer1-4; ends at the classification head.  x fp32 [B, 3, H, W], any layout.  Returns
    (the last fp32 channels_last map, OrderedDict of the maps after the children named in return_layers, under their new names)."""
    out = OrderedDict()
    with engine.defer_bn_counters():                 # nothing is pending in eval mode: a no-op there
        for name, module in net.named_children():
            if name == 'conv1':
                x = layers.conv_bn(module, net.bn1, x, relu=True)
            elif name in ('bn1', 'relu'):
                continue
            elif name == 'maxpool':
                x = layers.max_pool(x)
            elif name in ('avgpool', 'fc'):
                break
            else:
                for block in module:
                    x = block.forward_f32(x, layers)
            if name in return_layers:
                out[return_layers[name]] = x
    return x, out


def conv3x3(in_planes, out_planes, stride=1, groups=1, dilation=1):
    assert groups == 1
    return HipConv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=dilation, bias=False, dilation=dilation)


def conv1x1(in_planes, out_planes, stride=1):
    return HipConv2d(in_planes, out_planes, kernel_size=1, stride=stride, bias=False)


class Bottleneck(nn.Module):
    expansion = 4
    # No autograd, train-mode BatchNorm, large maps (conv_bn_separable): the downsample branch's BatchNorm is applied inside the
    # block-end pass instead of by a pass of its own (False: two passes, A/B).  Same bits either way.
    fuse_downsample_bn = True
    # forward(x, want_output=False) on the same route: conv3 keeps its BatchNorm side effects but stores no result and the
    # block-end pass is not run (False: the whole block runs and its result is dropped, A/B).
    skip_dead_output = True

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64, dilation=1, norm_layer=None):
        super().__init__()
        norm_layer = norm_layer or nn.BatchNorm2d
        width = int(planes * (base_width / 64.)) * groups
        self.conv1 = conv1x1(inplanes, width)
        self.bn1 = norm_layer(width)
        self.conv2 = conv3x3(width, width, stride, groups, dilation)
        self.bn2 = norm_layer(width)
        self.conv3 = conv1x1(width, planes * self.expansion)
        self.bn3 = norm_layer(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def _one_node_path(self, x):
        """True when conv1 / conv3 of this block both take conv_bn's one-autograd-node path and x needs a gradient: only then
        can the skip connection's gradient ride in conv1's data-gradient epilogue (engine._ConvBNTrainFn skip_in / skip_out)."""
        if not (torch.is_grad_enabled() and x.requires_grad and x.is_cuda and x.dtype == torch.bfloat16 and x.stride(1) == 1 and
                x.shape[1] % 8 == 0):
            return False
        for conv, bn in ((self.conv1, self.bn1), (self.conv3, self.bn3)):
            if conv.bias is not None or not bn.training or bn.weight is None or bn.running_mean is None or conv.out_channels % 8 or \
                    conv.out_channels > 2048 or conv.stride[0] != 1:
                return False
        return True

    def forward(self, x, want_output=True):
        """want_output=False: the caller reads nothing of the result (a frozen network run for its running statistics); every
        BatchNorm of the block still moves as in a full forward.  Returns None then."""
        identity = x
        # no downsample: x feeds conv1 AND the residual add -> one shared hand-over slot instead of autograd's gradient sum
        skip = {} if (self.downsample is None and self._one_node_path(x)) else None
        # A gradient parked by conv3's node that conv1's node never collected (a backward over a subset of the graph) would be a
        # silently missing term: found at the block's next forward, it raises.
        last = getattr(self, '_skip_slot', None)
        if last is not None and 'g' in last:
            last.clear()
            raise RuntimeError("Bottleneck: the skip-connection gradient parked by the last backward pass was never consumed "
                               "(backward over a sub-graph that excluded the block's first conv)")
        self._skip_slot = skip
        out = conv_bn(self.conv1, self.bn1, x, relu=True, skip_in=skip)
        out = conv_bn(self.conv2, self.bn2, out, relu=True)
        separable = conv_bn_separable(self.conv3, self.bn3, out)
        dead = not want_output and self.skip_dead_output and separable
        if self.downsample is not None:
            if self.fuse_downsample_bn and separable and not dead and conv_bn_separable(self.downsample[0], self.downsample[1], x):
                raw = conv_bn(self.downsample[0], self.downsample[1], x, defer=True)
                return self._out(conv_bn(self.conv3, self.bn3, out, relu=True, residual_affine=raw), want_output)
            identity = conv_bn(self.downsample[0], self.downsample[1], x)
        if dead:
            return conv_bn(self.conv3, self.bn3, out, want_output=False)
        return self._out(conv_bn(self.conv3, self.bn3, out, relu=True, residual=identity, skip_out=skip), want_output)

    @staticmethod
    def _out(y, want_output):
        return y if want_output else None

    def forward_f32(self, x, layers):
        """The block in fp32 on one F32Layers set: three conv + BatchNorm steps, four with a downsample conv (the residual's
        producer); the residual add and the last ReLU ride in conv3's step."""
        out = layers.conv_bn(self.conv1, self.bn1, x, relu=True)
        out = layers.conv_bn(self.conv2, self.bn2, out, relu=True)
        identity = x if self.downsample is None else layers.conv_bn(self.downsample[0], self.downsample[1], x)
        return layers.conv_bn(self.conv3, self.bn3, out, relu=True, residual=identity)

    def forward_fp32(self, x):
        """Eval mode: every BatchNorm folded, one launch per conv."""
        return self.forward_f32(x, F32_EVAL)

    def forward_train_fp32(self, x):
        """Every BatchNorm in the form its own `training` flag asks for (conv_bn_any_f32).  No autograd."""
        return self.forward_f32(x, F32_AS_FLAGGED)

    def forward_fp32_autograd(self, x):
        """forward_train_fp32 with autograd (K21): the same bits forward, every BatchNorm in train mode; backward on the fp32
        kernels (weight, BatchNorm and data gradients)."""
        return self.forward_f32(x, F32_AUTOGRAD)


class ResNet(nn.Module):
    def __init__(self, block, layers, num_classes=1000, zero_init_residual=False, groups=1, width_per_group=64,
                 replace_stride_with_dilation=None, norm_layer=None):
        super().__init__()
        norm_layer = norm_layer or nn.BatchNorm2d
        self._norm_layer = norm_layer
        self.inplanes = 64
        self.dilation = 1
        if replace_stride_with_dilation is None:
            replace_stride_with_dilation = [False, False, False]
        if len(replace_stride_with_dilation) != 3:
            raise ValueError("replace_stride_with_dilation should be None or a 3-element tuple")
        self.groups = groups
        self.base_width = width_per_group
        self.conv1 = HipConv2d(3, self.inplanes, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = norm_layer(self.inplanes)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = HipMaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2, dilate=replace_stride_with_dilation[0])
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2, dilate=replace_stride_with_dilation[1])
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2, dilate=replace_stride_with_dilation[2])
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * block.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, Bottleneck):
                    nn.init.constant_(m.bn3.weight, 0)

    def _make_layer(self, block, planes, blocks, stride=1, dilate=False):
        norm_layer = self._norm_layer
        downsample = None
        previous_dilation = self.dilation
        if dilate:
            self.dilation *= stride
            stride = 1
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(conv1x1(self.inplanes, planes * block.expansion, stride),
                                       norm_layer(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample, self.groups, self.base_width, previous_dilation, norm_layer)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, groups=self.groups, base_width=self.base_width,
                                dilation=self.dilation, norm_layer=norm_layer))
        return nn.Sequential(*layers)

    # No autograd, train-mode BatchNorm, large maps (conv_bn_separable): bn1 + ReLU are applied by the max pool to each tap as it
    # loads, the normalised stem map is never written (False: apply pass, then the plain pool, A/B).  Same bits either way.
    fuse_stem_pool = True

    def stem(self, x):
        mp = self.maxpool
        if self.fuse_stem_pool and isinstance(mp, HipMaxPool2d) and conv_bn_separable(self.conv1, self.bn1, x) and \
                (mp.kernel_size, mp.stride, mp.padding, mp.dilation, mp.ceil_mode) == (3, 2, 1, 1, False):
            raw = conv_bn(self.conv1, self.bn1, x, defer=True)
            return hip.max_pool_3x3s2_affine_relu(engine.from_nhwc(raw.y), raw.scale.view(-1), raw.shift.view(-1))
        x = conv_bn(self.conv1, self.bn1, x, relu=True)
        return self.maxpool(x)

    def features(self, x, want_output=True):
        """want_output=False: the call is made for the train-mode BatchNorm updates alone (nobody reads the layer4 map): the last
        block skips what only its result needs (Bottleneck.forward) and None comes back."""
        with engine.defer_bn_counters():             # 53 num_batches_tracked bumps -> one multi-tensor add
            x = self.stem(x)
            x = self.layer1(x)
            x = self.layer2(x)
            x = self.layer3(x)
            if want_output:
                return self.layer4(x)
            for block in self.layer4[:-1]:
                x = block(x)
            return self.layer4[-1](x, want_output=False)

    def features_fp32(self, x):
        """features() in fp32: x fp32 [B, 3, H, W], any layout -> the fp32 channels_last layer4 map.  Per BatchNorm the folded
        (eval) or the batch-statistics (train) form.  No autograd."""
        return walk_f32(self, x, F32_AS_FLAGGED)[0]

    def features_fp32_autograd(self, x):
        """features_fp32 with autograd (K21): every BatchNorm in train mode; the same bits forward, the gradients of every
        parameter on the fp32 backward kernels."""
        return walk_f32(self, x, F32_AUTOGRAD)[0]

    def forward(self, x):
        x = self.features(x)
        x = torch.flatten(self.avgpool(x.float()), 1)
        return self.fc(x)


def resnet50(pretrained=False, progress=True, **kwargs):
    if pretrained:
        raise NotImplementedError("no network access: load weights with load_state_dict")
    return ResNet(Bottleneck, [3, 4, 6, 3], **kwargs)
