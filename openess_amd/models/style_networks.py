"""Host-side mirror of models/style_networks.py: SemSegE2VID task decoder (reference :9-198),
ReLUINSConv2d (:252-263), INSResBlock (:266-289).  Same constructor arguments, state_dict keys and
return values; the convolutions run on the HIP MFMA kernel (forward + data gradient).

Deviation that changes no result (documented in DESIGN.md): decoder_ch256 -> decoder_ch512 ->
conv2d(text_embeddings) are three linear maps with nothing in between (style_networks.py:161-163),
so the logits are computed as ONE 1x1 conv with the composed operator T*W512*W256 (and composed
bias); the 512-channel full-resolution tensor (4.6 GB fp32 at DSEC B=8) is never materialised.
Autograd differentiates the composition, so every parameter receives the same gradient.
"""
from typing import Callable, NamedTuple

import torch
import torch.nn as nn
import torch.nn.functional as f

from .. import engine, hip


def gaussian_weights_init(m):
    classname = m.__class__.__name__
    if classname.find('Conv') != -1 and classname.find('Conv') == 0:
        m.weight.data.normal_(0.0, 0.02)


class _HipConv2d(nn.Conv2d):
    """nn.Conv2d whose forward runs the MFMA kernel (class name starts with '_Hip' on purpose: the
    reference's gaussian_weights_init only touches classes whose name STARTS with 'Conv')."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self._pw = engine.PackedWeight()
        self._pw32 = engine.PackedWeightF32()
        self._pw32_train = engine.PackedWeightF32()

    def forward_f32(self, x, act=None, out=None):
        """fp32 inference (K15): act(conv(x) + bias) on the f32-input MFMA kernel, operand cached per parameter versions."""
        pw = self._pw32.get(self.weight, self.bias)
        return hip.conv2d_f32(x, pw.packed, pw.bias, self.out_channels, self.kernel_size[0], self.kernel_size[1], self.stride[0],
                              self.padding[0], act=act, out=out)

    def forward_f32_train(self, x):
        """fp32 training (K18): conv(x) + bias under autograd, forward and backward on the f32-input MFMA kernels."""
        return hip.conv2d_f32_train(x, self.weight, self.bias, self.stride[0], self.padding[0], self.dilation[0], pw=self._pw32_train)

    def forward(self, x, out_f32=False):
        return engine.conv2d_train(x, self.weight, self.bias, self._pw, self.kernel_size[0], self.stride[0],
                                   self.padding[0], self.dilation[0], out_f32=out_f32)


def _conv(n_in, n_out, kernel_size, stride=1, padding=0, bias=True):
    m = _HipConv2d(n_in, n_out, kernel_size=kernel_size, stride=stride, padding=padding, bias=bias)
    m.weight.data.normal_(0.0, 0.02)          # == gaussian_weights_init applied by the reference blocks
    return m


def _conv_norm_f32(conv, norm, x, relu=False, residual=None):
    """conv -> InstanceNorm2d [+ residual] [+ ReLU] in fp32, inference (K15): the norm in place on the conv's output."""
    y = conv.forward_f32(x)
    return hip.instance_norm_f32(y, relu=relu, residual=residual, eps=norm.eps, out=y)


def _conv_norm_f32_train(conv, norm, x, relu=False, residual=None):
    """The same step under autograd (K18), not in place."""
    return hip.instance_norm_f32_train(conv.forward_f32_train(x), relu=relu, residual=residual, eps=norm.eps)


class F32Layers(NamedTuple):
    """The per-layer functions of one mode of the fp32 decoder: what SemSegE2VID._decoder_f32 and its blocks call."""
    conv_norm: Callable            # (conv, norm, x, relu=False, residual=None) -> y
    upsample_concat: Callable      # (x, skip=None) -> y


F32_EVAL = F32Layers(_conv_norm_f32, hip.upsample2x_concat_f32)
F32_TRAIN = F32Layers(_conv_norm_f32_train, hip.upsample2x_concat_f32_train)


def _instance_norm(x, relu, residual=None):
    # nn.InstanceNorm2d defaults: affine=False, no running stats, eps=1e-5; fused [+ residual] [+ ReLU]
    return hip.instance_norm(x, relu=relu, residual=residual)


class ReLUINSConv2d(nn.Module):
    def __init__(self, n_in, n_out, kernel_size, stride, padding=0):
        super().__init__()
        self.model = nn.Sequential(_conv(n_in, n_out, kernel_size, stride, padding, bias=True),
                                   nn.InstanceNorm2d(n_out, affine=False), nn.ReLU(inplace=True))

    def forward(self, x):
        return _instance_norm(self.model[0](x), relu=True)

    def _forward_f32(self, x, layers):
        return layers.conv_norm(self.model[0], self.model[1], x, relu=True)

    def forward_f32(self, x):
        return self._forward_f32(x, F32_EVAL)

    def forward_f32_train(self, x):
        return self._forward_f32(x, F32_TRAIN)


class INSResBlock(nn.Module):
    def __init__(self, inplanes, planes, stride=1, dropout=0.0):
        super().__init__()
        model = [_conv(inplanes, planes, 3, stride, 1), nn.InstanceNorm2d(planes), nn.ReLU(inplace=True),
                 _conv(planes, planes, 3, 1, 1), nn.InstanceNorm2d(planes)]
        if dropout > 0:
            model += [nn.Dropout(p=dropout)]
        self.model = nn.Sequential(*model)

    def forward(self, x):
        out = _instance_norm(self.model[0](x), relu=True)
        if len(self.model) > 5:
            return self.model[5](_instance_norm(self.model[3](out), relu=False)) + x
        return _instance_norm(self.model[3](out), relu=False, residual=x)      # out += residual (:287)

    def _forward_f32(self, x, layers):
        y = layers.conv_norm(self.model[0], self.model[1], x, relu=True)
        return layers.conv_norm(self.model[3], self.model[4], y, residual=x)

    def forward_f32(self, x):
        return self._forward_f32(x, F32_EVAL)

    def forward_f32_train(self, x):
        if len(self.model) > 5:
            raise NotImplementedError("forward_f32_train has no dropout (INSResBlock(dropout > 0))")
        return self._forward_f32(x, F32_TRAIN)


def compose_head_f64(w256, b256, w512, b512, text):
    """decoder_ch256 -> decoder_ch512 -> conv2d(text_embeddings) as one 1x1 operator, composed in float64:
    (T W512 W256 [K, C, 1, 1], T b512 + T W512 b256 [K])."""
    w1, w2, t = w256.detach().double().flatten(1), w512.detach().double().flatten(1), text.detach().double()
    tw2 = t @ w2
    return (tw2 @ w1)[:, :, None, None], t @ b512.detach().double() + tw2 @ b256.detach().double()


def skip_concat(x1, x2):
    return torch.cat([x1, x2], dim=1)


def skip_sum(x1, x2):
    return x1 + x2


class SemSegE2VID(nn.Module):
    def __init__(self, input_c, output_c, skip_connect=False, skip_type='sum', input_index_map=False,
                 text_embeddings_path='', if_linear_probing=False, materialize_ch256=True):
        super().__init__()
        if not skip_connect or input_index_map:
            raise NotImplementedError("every shipped config uses skip_connect_task: True (style_networks.py:34)")
        self.skip_connect = skip_connect
        self.skip_type = skip_type
        self.apply_skip_connection = skip_sum if skip_type == 'sum' else skip_concat
        self.materialize_ch256 = materialize_ch256
        tch = input_c
        text_categories = output_c
        self.text_embeddings_path = text_embeddings_path
        if text_embeddings_path is None:
            self.text_embeddings = nn.Parameter(torch.zeros(text_categories, 512))
            nn.init.normal_(self.text_embeddings, mean=0.0, std=0.01)
        else:
            self.register_buffer('text_embeddings', torch.randn(text_categories, 512))
            if text_embeddings_path:
                # the reference hard-codes map_location='cuda' (style_networks.py:31)
                loaded = torch.load(text_embeddings_path, map_location='cpu')
                self.text_embeddings[:, :] = loaded[:, :]
        layers = [INSResBlock(tch, tch) for _ in range(5)]
        layers += [ReLUINSConv2d(tch, tch // 2, kernel_size=3, stride=1, padding=1)]
        self.decoder_scale_1 = nn.Sequential(*layers)
        self.decoder_scale_2 = nn.Sequential(ReLUINSConv2d(tch, tch // 2, 3, 1, 1), ReLUINSConv2d(tch // 2, tch // 4, 3, 1, 1))
        tch = tch // 2
        self.decoder_scale_3 = nn.Sequential(ReLUINSConv2d(tch, tch // 2, 3, 1, 1), ReLUINSConv2d(tch // 2, tch // 2, 3, 1, 1))
        tch = tch // 2
        self.decoder_scale_4 = nn.Sequential(ReLUINSConv2d(tch, tch // 2, 3, 1, 1))
        tch = tch // 2
        # decoder_scale_5 exists in the reference's state_dict but is never used in the skip path (:61-63, :167)
        self.decoder_scale_5 = nn.Sequential(nn.Conv2d(tch, output_c, kernel_size=1, stride=1, padding=0))
        self.decoder_ch256 = nn.Sequential(_HipConv2d(tch, 256, kernel_size=1, stride=1, padding=0))
        self.decoder_ch512 = nn.Sequential(nn.Conv2d(256, 512, kernel_size=1, stride=1, padding=0))
        self.if_linear_probing = if_linear_probing
        if if_linear_probing:
            for mod in (self.decoder_scale_1, self.decoder_scale_2, self.decoder_scale_3, self.decoder_scale_4,
                        self.decoder_ch256, self.decoder_ch512):
                for p in mod.parameters():
                    p.requires_grad = False
            self.linear_probe = nn.Conv2d(text_categories, text_categories, 1)
        self._pw_head = engine.PackedWeight()
        self._pw32_head, self._pw32_probe = engine.PackedWeightF32(), engine.PackedWeightF32()
        self._pw32_head_train = engine.PackedWeightF32()

    def update_skip_dict(self, skips, x, sz_in):
        rem, scale = sz_in % x.shape[3], sz_in // x.shape[3]
        assert rem == 0
        skips[scale] = x

    def _composed_head(self):
        """T*W512*W256 and its bias (fp32, differentiable)."""
        w1 = self.decoder_ch256[0].weight.flatten(1)              # 256 x 32
        b1 = self.decoder_ch256[0].bias
        w2 = self.decoder_ch512[0].weight.flatten(1)              # 512 x 256
        b2 = self.decoder_ch512[0].bias
        t = self.text_embeddings.float()                          # K x 512
        tw2 = t @ w2
        return (tw2 @ w1)[:, :, None, None], t @ b2 + tw2 @ b1

    def _decoder(self, input_dict):
        """THE bf16 decoder walk of forward and head_features: (out with the keys 8, 4 and 2, the decoder_scale_4 map)."""
        sz_in = input_dict[1].shape[3]
        x = input_dict[8]
        out = {8: x}
        concat = self.skip_type != 'sum'
        x = self.decoder_scale_1(x)
        # nearest x2 + skip concat written into one NHWC buffer (no separate interpolate / cat tensors)
        x = hip.upsample2x_concat(x, input_dict[4]) if concat else hip.upsample2x_concat(x) + input_dict[4]
        x = self.decoder_scale_2(x)
        self.update_skip_dict(out, x, sz_in)
        x = hip.upsample2x_concat(x, input_dict[2]) if concat else hip.upsample2x_concat(x) + input_dict[2]
        x = self.decoder_scale_3(x)
        self.update_skip_dict(out, x, sz_in)
        x = hip.upsample2x_concat(x)
        return out, self.decoder_scale_4(x)

    @torch.no_grad()
    def head_features(self, input_dict, precision='bf16'):
        """The decoder_scale_4 map [B, 32, H, W], the operand of the composed head: bf16 from forward's pieces
        ('bf16'), fp32 from forward_fp32's ('fp32', under check_fp32's rules).  With compose_vocabulary's operator the logits of
        ANY vocabulary follow from it; neither method touches text_embeddings or the cached packed operands."""
        if precision not in ('bf16', 'fp32'):
            raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
        if precision == 'fp32':
            self.check_fp32()
            return self._decoder_f32('head_features', input_dict, F32_EVAL)[1]
        return self._decoder(input_dict)[1]

    @torch.no_grad()
    def compose_vocabulary(self, text):
        """(fp32 [P, 32], fp32 [P]): decoder_ch256 -> decoder_ch512 -> text [P, 512] as one operator, composed in float64
        (compose_head_f64) and rounded once -- forward_fp32's head for any vocabulary.  A linear probe is tied to the trained
        classes: refused."""
        if self.if_linear_probing:
            raise NotImplementedError("compose_vocabulary: the linear probe's K x K conv is tied to the trained classes")
        if not torch.is_tensor(text) or text.ndim != 2 or text.shape[1] != self.decoder_ch512[0].out_channels or text.shape[0] < 1:
            raise ValueError(f"compose_vocabulary takes text embeddings [P, {self.decoder_ch512[0].out_channels}]")
        c256, c512 = self.decoder_ch256[0], self.decoder_ch512[0]
        w, b = compose_head_f64(c256.weight, c256.bias, c512.weight, c512.bias, text.to(c256.weight.device))
        return w.flatten(1).float().contiguous(), b.float().contiguous()

    def forward(self, input_dict):
        sz_in = input_dict[1].shape[3]
        out, x = self._decoder(input_dict)
        # 'pooled': the 256-channel map only feeds the superpixel mean, which commutes with the 1x1 convolution (hip.PointwiseFeature)
        if self.materialize_ch256 == 'pooled':
            x_ch256 = hip.PointwiseFeature(x, self.decoder_ch256[0])
        else:
            x_ch256 = self.decoder_ch256[0](x) if self.materialize_ch256 else None
        wf, bf = self._composed_head()
        ver = tuple(p._version for p in (self.decoder_ch256[0].weight, self.decoder_ch256[0].bias,
                                         self.decoder_ch512[0].weight, self.decoder_ch512[0].bias, self.text_embeddings))
        logits = engine.conv2d_train(x, wf, bf, self._pw_head, 1, out_f32=True, ver=ver)
        if self.if_linear_probing:
            logits = hip.linear_probe(logits, self.linear_probe)
        self.update_skip_dict(out, logits, sz_in)
        return out, x_ch256

    @staticmethod
    def check_fp32_config(skip_type='concat', materialize_ch256=True, train=False):
        """check_fp32's refusals that follow from the constructor arguments alone, for a caller that must refuse before it
        builds anything (the trainers' train_precision: fp32).  train=True: the rules of forward_fp32_train, which has the
        'pooled' form (the fp32 hip.PointwiseFeature); inference has no consumer for it."""
        if skip_type != 'concat':
            raise NotImplementedError(f"forward_fp32 runs skip_type='concat' (every shipped config), not {skip_type!r}")
        if materialize_ch256 == 'pooled' and not train:
            raise NotImplementedError("forward_fp32 has no 'pooled' form of x_ch256 (a pre-training option of the bf16 path)")

    def check_fp32(self, train=False):
        """The configurations forward_fp32 runs: skip_type 'concat' (with 'sum' the reference's own channel counts do not fit:
        ReLUINSConv2d(256, ...) would receive 128 channels), no dropout in an INSResBlock; raises otherwise, before any launch."""
        self.check_fp32_config(self.skip_type, self.materialize_ch256, train=train)
        for m in self.modules():
            if isinstance(m, nn.Dropout) and m.p > 0:
                raise NotImplementedError("forward_fp32 has no dropout (INSResBlock(dropout > 0))")

    def _head_f32(self):
        c256, c512 = self.decoder_ch256[0], self.decoder_ch512[0]
        params = (c256.weight, c256.bias, c512.weight, c512.bias, self.text_embeddings)
        return self._pw32_head.get_composed(params, lambda: compose_head_f64(*params))

    def _decoder_f32(self, name, input_dict, layers):
        """THE fp32 decoder walk of forward_fp32 and forward_fp32_train (`name`: the one called): decoder_scale_1 to 4 over the
        latents on one F32Layers set.  Returns (out with the keys 8, 4 and 2, the decoder_scale_4 map)."""
        for k in (1, 2, 4, 8):
            if input_dict[k].dtype != torch.float32:
                raise ValueError(f"{name} takes the fp32 latents of the fp32 E2VID path")
        sz_in = input_dict[1].shape[3]
        x = input_dict[8]
        out = {8: x}
        for layer in self.decoder_scale_1:
            x = layer._forward_f32(x, layers)
        x = layers.upsample_concat(x, input_dict[4])
        for layer in self.decoder_scale_2:
            x = layer._forward_f32(x, layers)
        self.update_skip_dict(out, x, sz_in)
        x = layers.upsample_concat(x, input_dict[2])
        for layer in self.decoder_scale_3:
            x = layer._forward_f32(x, layers)
        self.update_skip_dict(out, x, sz_in)
        x = layers.upsample_concat(x)
        return out, self.decoder_scale_4[0]._forward_f32(x, layers)

    def forward_fp32(self, input_dict):
        """fp32 inference (K15): forward() in the reference's arithmetic.  input_dict: the fp32 latents {1, 2, 4, 8} of
        UNetRecurrent.forward_fp32 (logical NCHW, any strides; read where they are).  Returns (out, x_ch256) as forward():
        out[1] the fp32 logits at input size, out[2], out[4] the decoder features, x_ch256 fp32 or None."""
        self.check_fp32()
        with torch.no_grad():
            out, x = self._decoder_f32('forward_fp32', input_dict, F32_EVAL)
            x_ch256 = self.decoder_ch256[0].forward_f32(x) if self.materialize_ch256 else None
            pw = self._head_f32()
            K = self.text_embeddings.shape[0]
            logits = hip.conv2d_f32(x, pw.packed, pw.bias, K, 1, 1)
            if self.if_linear_probing:
                pp = self._pw32_probe.get(self.linear_probe.weight, self.linear_probe.bias)
                logits = hip.conv2d_f32(logits, pp.packed, pp.bias, K, 1, 1)
            self.update_skip_dict(out, logits, input_dict[1].shape[3])
        return out, x_ch256

    def forward_fp32_train(self, input_dict):
        """fp32 training (K18): forward_fp32 under autograd.  Same inputs, refusals and return structure; every layer is an fp32
        autograd function of hip (conv2d_f32_train, instance_norm_f32_train, upsample2x_concat_f32_train), so the decoder's
        parameters (and text_embeddings when it is a parameter) receive fp32 gradients; latents that need no gradient (the frozen
        encoder's) get none computed.  The head is conv2d_f32_train on the operator of _composed_head(), composed in fp32 by
        autograd (forward_fp32 composes it in float64 and rounds once: the logits agree within the fp32 bound, not bit for bit).
        With if_linear_probing the frozen decoder runs under no_grad and only hip.linear_probe trains.
        materialize_ch256='pooled' returns x_ch256 as the fp32 hip.PointwiseFeature."""
        self.check_fp32(train=True)
        frozen = self.if_linear_probing
        with torch.no_grad() if frozen else torch.enable_grad():
            out, x = self._decoder_f32('forward_fp32_train', input_dict, F32_TRAIN)
            if self.materialize_ch256 == 'pooled':      # pre-training (K20): the superpixel mean commutes with the 1x1 conv
                x_ch256 = hip.PointwiseFeature(x, self.decoder_ch256[0])
            else:
                x_ch256 = self.decoder_ch256[0].forward_f32_train(x) if self.materialize_ch256 else None
            wf, bf = self._composed_head()
            ver = tuple(p._version for p in (self.decoder_ch256[0].weight, self.decoder_ch256[0].bias,
                                             self.decoder_ch512[0].weight, self.decoder_ch512[0].bias, self.text_embeddings))
            logits = hip.conv2d_f32_train(x, wf, bf, pw=self._pw32_head_train, ver=ver)
        if frozen:
            logits = hip.linear_probe(logits, self.linear_probe)
        self.update_skip_dict(out, logits, input_dict[1].shape[3])
        return out, x_ch256
