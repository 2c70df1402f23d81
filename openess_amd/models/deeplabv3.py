"""Mirror of models/deeplabv3.py: deeplabv3_resnet50 (:128-189), DeepLabHead (:86-125), ASPP (:319-348),
ASPPConv (:295-302), ASPPPooling (:305-316), IntermediateLayerGetter (:21-83).  Same state_dict keys."""
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import engine, hip
from . import _resnet as resnet
from ._resnet import HipConv2d, conv_bn, conv_bn_f32, conv_bn_f32_autograd


class IntermediateLayerGetter(nn.ModuleDict):
    def __init__(self, model, return_layers):
        if not set(return_layers).issubset([name for name, _ in model.named_children()]):
            raise ValueError("return_layers are not present in model")
        orig = return_layers
        return_layers = dict(return_layers)
        layers = OrderedDict()
        for name, module in model.named_children():
            layers[name] = module
            if name in return_layers:
                del return_layers[name]
            if not return_layers:
                break
        super().__init__(layers)
        self.return_layers = orig

    def forward(self, x):
        out = OrderedDict()
        x = engine.to_cl_bf16(x)
        for name, module in self.named_children():
            if name == 'conv1':
                x = conv_bn(module, self['bn1'], x, relu=True)
                continue
            if name in ('bn1', 'relu'):
                continue
            x = module(x)
            if name in self.return_layers:
                out[self.return_layers[name]] = x
        return out

    def forward_fp32(self, x):
        """forward() in fp32 (eval mode): x fp32 [B, 3, H, W], any layout; the same OrderedDict of fp32 channels_last maps."""
        return resnet.walk_f32(self, x, resnet.F32_EVAL, self.return_layers)[1]

    def forward_fp32_autograd(self, x):
        """forward() in fp32 with autograd and every BatchNorm in train mode (K22): ResNet.features_fp32_autograd's own walk, so
        its bits.  x fp32 [B, 3, H, W], any layout."""
        return resnet.walk_f32(self, x, resnet.F32_AUTOGRAD, self.return_layers)[1]


class _ConvBNReLU(nn.Sequential):
    def forward(self, x, out=None):
        return conv_bn(self[0], self[1], x, relu=True, out=out)

    def forward_f32(self, x, layers, **kw):
        """kw: out=, for the eval set only (a branch's channel slice of ASPP's concat buffer)."""
        return layers.conv_bn(self[0], self[1], x, relu=True, **kw)

    def forward_fp32(self, x, out=None):
        return self.forward_f32(x, resnet.F32_EVAL, out=out)

    def forward_fp32_autograd(self, x):
        return self.forward_f32(x, resnet.F32_AUTOGRAD)


class ASPPConv(_ConvBNReLU):
    def __init__(self, in_channels, out_channels, dilation):
        super().__init__(HipConv2d(in_channels, out_channels, 3, padding=dilation, dilation=dilation, bias=False),
                         nn.BatchNorm2d(out_channels), nn.ReLU(inplace=True))


class ASPPPooling(nn.Sequential):
    def __init__(self, in_channels, out_channels):
        super().__init__(nn.AdaptiveAvgPool2d(1), nn.Conv2d(in_channels, out_channels, 1, bias=False),
                         nn.BatchNorm2d(out_channels), nn.ReLU(inplace=True))
        self._pw32 = engine.PackedWeightF32()

    def forward_fp32(self, x, out):
        """Global average pool (fixed-order fp32 sums), the 1 x 1 conv + BatchNorm + ReLU on the B x 1 x 1 map, then the
        broadcast (bilinear from 1 x 1) into `out`, the branch's channel slice of the concat buffer."""
        y = conv_bn_f32(self[1], self[2], hip.global_avg_pool_f32(x), relu=True, pw=self._pw32)
        out.copy_(y.expand(-1, -1, x.shape[2], x.shape[3]))
        return out

    def forward_fp32_autograd(self, x):
        """The branch in fp32 with autograd and a train-mode BatchNorm (K22), one node: the [B, Cout, 1, 1] row expanded with
        stride 0 over the map."""
        return hip.aspp_pool_branch_f32(x, self[1], self[2])

    def forward(self, x, out=None):
        size = x.shape[-2:]
        bn = self[2]
        if bn.training and x.is_cuda and x.dtype == torch.bfloat16 and x.stride(1) == 1 and x.shape[1] % 8 == 0 and \
                x.shape[1] <= 2048 and 2 <= x.shape[0] <= 16 and bn.running_mean is not None:
            # train mode: pooling, B-row GEMV, BatchNorm over the B pooled vectors and ReLU on the HIP kernels, one autograd node
            y = hip.aspp_pool_branch(x, self[1], bn)
            if out is not None:
                out.copy_(y)
                return out
            return y
        if x.is_cuda and x.dtype == torch.bfloat16 and x.stride(1) == 1 and x.shape[1] % 8 == 0 and x.shape[1] <= 2048:
            y = hip.global_avg_pool(x)                                     # AdaptiveAvgPool2d(1) without an fp32 copy of the map
        else:
            y = x.float().mean(dim=(2, 3), keepdim=True)
        y = torch.matmul(y.flatten(1), self[1].weight.flatten(1).t())[:, :, None, None]   # B x C x 1 x 1: a GEMV, not a conv
        y = F.relu(self[2](y))
        y = y.to(x.dtype).expand(-1, -1, size[0], size[1])                 # bilinear from 1x1 == broadcast
        if out is not None:
            out.copy_(y)
            return out
        return y


class ASPP(nn.Module):
    def __init__(self, in_channels, atrous_rates):
        super().__init__()
        out_channels = 256
        modules = [_ConvBNReLU(HipConv2d(in_channels, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels),
                               nn.ReLU(inplace=True))]
        rate1, rate2, rate3 = tuple(atrous_rates)
        modules += [ASPPConv(in_channels, out_channels, rate1), ASPPConv(in_channels, out_channels, rate2),
                    ASPPConv(in_channels, out_channels, rate3), ASPPPooling(in_channels, out_channels)]
        self.convs = nn.ModuleList(modules)
        self.project = nn.Sequential(HipConv2d(5 * out_channels, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels),
                                     nn.ReLU(inplace=True), nn.Dropout(0.1))

    def forward(self, x):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            res = torch.cat([conv(x) for conv in self.convs], dim=1)
        else:
            # no autograd: every branch writes its channel slice of ONE NHWC concat buffer (conv output, BatchNorm apply in
            # place on the slice) -- no torch.cat pass over the 5 x 256 channels
            B, _, H, W = x.shape
            oc = self.convs[0][0].out_channels
            res = engine.empty_cl(B, oc * len(self.convs), H, W, x.device)
            for i, conv in enumerate(self.convs):
                conv(x, out=res[:, i * oc:(i + 1) * oc])
        y = conv_bn(self.project[0], self.project[1], res, relu=True)
        drop = self.project[3]
        if drop.training and drop.p > 0 and y.is_cuda and y.dtype == torch.bfloat16 and y.stride(1) == 1 and y.shape[1] % 8 == 0:
            return hip.dropout(y, drop.p, True, owner=drop)            # Philox mask recomputed in the backward pass (nn.Dropout(0.1), :343)
        return drop(y)

    def forward_fp32(self, x):
        B, _, H, W = x.shape
        oc = self.convs[0][0].out_channels
        res = engine.empty_cl(B, oc * len(self.convs), H, W, x.device, dtype=torch.float32)
        for i, conv in enumerate(self.convs):
            conv.forward_fp32(x, out=res[:, i * oc:(i + 1) * oc])
        return conv_bn_f32(self.project[0], self.project[1], res, relu=True)          # Dropout: the identity in eval mode

    def forward_fp32_autograd(self, x):
        """forward() in fp32 with autograd (K22): the five branches, one concatenation pass (along the dense channel axis of
        the NHWC maps, so the 1280-channel map and the slices of its gradient are channels_last), the projection and the Philox
        dropout of hip.dropout on the module's own counter."""
        res = torch.cat([conv.forward_fp32_autograd(x).permute(0, 2, 3, 1) for conv in self.convs], dim=3).permute(0, 3, 1, 2)
        y = conv_bn_f32_autograd(self.project[0], self.project[1], res, relu=True)
        drop = self.project[3]
        return hip.dropout_f32(y, drop.p, drop.training, owner=drop)


class DeepLabHead(nn.Module):
    def __init__(self, text_embeddings_path, text_categories, in_channels, num_classes, aspp_dilate=[12, 24, 36]):
        super().__init__()
        self.ASPP = ASPP(in_channels, aspp_dilate)
        self.pixel_feature = nn.Conv2d(256, 512, 3, padding=1, bias=False)     # unused in the reference too (:94)
        self.classifier = nn.Sequential(HipConv2d(256, 512, 3, padding=1, bias=False), nn.BatchNorm2d(512),
                                        nn.ReLU(inplace=True))
        self._init_weight()
        self.text_embeddings_path = text_embeddings_path
        if text_embeddings_path is None:
            self.text_embeddings = nn.Parameter(torch.zeros(text_categories, 512))
            nn.init.normal_(self.text_embeddings, mean=0.0, std=0.01)
        else:
            self.register_buffer('text_embeddings', torch.randn(text_categories, 512))
            if text_embeddings_path:
                loaded = torch.load(text_embeddings_path, map_location='cpu')   # reference: map_location='cuda'
                self.text_embeddings[:, :] = loaded[:, :]
        self._pw_text = engine.PackedWeight()
        self._pw_text32 = engine.PackedWeightF32()
        self._pw_text32_train = engine.PackedWeightF32()      # fp32 training operands (forward_fp32_autograd)
        self._vocab_text = None                               # the run-time vocabulary the two operands below were packed from
        self._pw_vocab, self._pw_vocab32 = engine.PackedWeight(), engine.PackedWeightF32()

    def _vocabulary(self, text):
        """Operand caches of a run-time vocabulary (K36), apart from those of the registered text_embeddings: fresh ones whenever
        another matrix arrives.  text: fp32 [P, 512] on the module's device."""
        te = self.text_embeddings
        if (not torch.is_tensor(text) or text.ndim != 2 or text.shape[1] != te.shape[1] or text.shape[0] < 1
                or text.dtype != torch.float32 or text.device != te.device):
            raise ValueError(f"text_embeddings must be a float32 [P, {te.shape[1]}] matrix on {te.device}")
        if text is not self._vocab_text:
            self._vocab_text = text
            self._pw_vocab, self._pw_vocab32 = engine.PackedWeight(), engine.PackedWeightF32()
        return text.detach()

    def forward_fp32(self, feature, text=None):
        """text: a run-time vocabulary [P, 512] in place of text_embeddings (K36); None: the registered matrix and its operand."""
        feature = self.ASPP.forward_fp32(feature['out'])
        x = conv_bn_f32(self.classifier[0], self.classifier[1], feature, relu=True)
        if text is not None:
            te = self._vocabulary(text)
            op = self._pw_vocab32.get_composed([te], lambda: (te.double()[:, :, None, None], None))
            return hip.conv2d_f32(x, op.packed, None, te.shape[0], 1, 1), feature
        te = self.text_embeddings
        op = self._pw_text32.get_composed([te], lambda: (te.detach().double()[:, :, None, None], None))
        return hip.conv2d_f32(x, op.packed, None, te.shape[0], 1, 1), feature

    def forward_fp32_autograd(self, feature):
        """forward() in fp32 with autograd (K22): (logits, ASPP feature) at the backbone's resolution.  The text embeddings are
        the 1 x 1 classifier's weight as they are: a Parameter gets its gradient, a buffer gets none."""
        feature = self.ASPP.forward_fp32_autograd(feature['out'])
        x = conv_bn_f32_autograd(self.classifier[0], self.classifier[1], feature, relu=True)
        te = self.text_embeddings
        logits = hip.conv2d_dilated_f32_train(x, te[:, :, None, None], None, pw=self._pw_text32_train, ver=te._version)
        return logits, feature

    def forward(self, feature, text=None):
        feature = self.ASPP(feature['out'])
        x = conv_bn(self.classifier[0], self.classifier[1], feature, relu=True)
        if text is not None:                                  # a run-time vocabulary (K36): its own operand, no autograd
            te = self._vocabulary(text)
            with torch.no_grad():
                return engine.conv2d_train(x, te[:, :, None, None], None, self._pw_vocab, 1, ver=te._version), feature
        logits = engine.conv2d_train(x, self.text_embeddings[:, :, None, None].float(), None, self._pw_text, 1,
                                     ver=self.text_embeddings._version)
        return logits, feature

    def _init_weight(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)


class deeplabv3_resnet50(nn.Module):
    feats_fp32 = False
    lazy_feats = False            # see forward()

    def __init__(self, num_classes, text_embeddings_path, output_stride, pretrained_backbone, if_linear_probing=False,
                 if_finetuning=False, frozen_backbone=False):
        super().__init__()
        if output_stride == 8:
            replace_stride_with_dilation, aspp_dilate = [False, True, True], [12, 24, 36]
        else:
            replace_stride_with_dilation, aspp_dilate = [False, False, True], [6, 12, 18]
        backbone = resnet.resnet50(replace_stride_with_dilation=replace_stride_with_dilation)
        classifier = DeepLabHead(text_embeddings_path, num_classes, 2048, num_classes, aspp_dilate)
        self.backbone = IntermediateLayerGetter(backbone, return_layers={'layer4': 'out'})
        self.classifier = classifier
        if pretrained_backbone != '':
            pretrained = torch.load(pretrained_backbone, map_location='cpu')
            self.load_state_dict(pretrained['model_recon'], strict=True)
        self.if_linear_probing = if_linear_probing
        if if_linear_probing:
            for p in self.backbone.parameters():
                p.requires_grad = False
            for p in self.classifier.parameters():
                p.requires_grad = False
            self.linear_probe = nn.Conv2d(num_classes, num_classes, 1)
        self.if_finetuning = if_finetuning
        if if_finetuning and frozen_backbone:
            for p in self.backbone.parameters():
                p.requires_grad = False
            for p in self.classifier.parameters():
                p.requires_grad = True

    def check_fp32(self):
        """Raises NotImplementedError for what forward_fp32 does not run: it is the eval-mode network (BatchNorm folded from its
        running statistics, Dropout the identity)."""
        for name, m in self.named_modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm) and (m.training or m.running_mean is None or m.running_var is None):
                raise NotImplementedError(f"forward_fp32 folds BatchNorm's running statistics into the convs: {name or 'the model'} "
                                          "is in train mode (batch statistics); call .eval() first")
            if isinstance(m, nn.Dropout) and m.training and m.p > 0:
                raise NotImplementedError(f"forward_fp32 is inference only: dropout {name} is in train mode; call .eval() first")

    def check_fp32_train(self):
        """Raises NotImplementedError for what forward_fp32_train does not run: it is the train-mode network, every BatchNorm on
        batch statistics with a running-statistics step."""
        for name, m in self.named_modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                what = ("is in eval mode (running statistics): call .train() first, or use forward_fp32" if not m.training else
                        "keeps no running statistics" if m.running_mean is None or m.running_var is None else
                        "has momentum=None (cumulative moving average)" if m.momentum is None else None)
                if what is not None:
                    raise NotImplementedError(f"forward_fp32_train runs every BatchNorm on batch statistics with a momentum step: "
                                              f"{name or 'the model'} {what}")

    def forward_fp32_train(self, x, want_feats=False):
        """forward() of the train-mode network in fp32 with autograd: (logits, feats).  logits: fp32 at the input
        size, through the linear probe when the model has one.  feats: the ASPP feature resized to the input size, formed only
        when asked for (256 channels at full resolution), otherwise None; want_feats='lazy' returns it as hip.UpsampledFeature
        over the fp32 feature at the network's stride instead (nothing of the full resolution is formed).  Frozen parameters record nothing: a node whose inputs
        need no gradient keeps no graph, the first trainable convolution skips its data gradient.  No buffer, operand or state
        is shared with forward(), except the Dropout module's mask counter (one mask sequence for both)."""
        self.check_fp32_train()
        return self._forward_fp32('forward_fp32_train', x, True, want_feats)

    @torch.no_grad()
    def forward_fp32(self, x):
        """forward() of the eval-mode network in fp32 on the f32-input MFMA kernels: (logits, feats), both fp32 at
        the input size.  No buffer, operand or state is shared with forward()."""
        self.check_fp32()
        return self._forward_fp32('forward_fp32', x, False, True)

    @torch.no_grad()
    def logits_at_stride(self, x, precision='bf16', text_embeddings=None):
        """The eval-mode network up to the classifier's output, fp32 [B, K, H / stride, W / stride]: what forward() ('bf16') and
        forward_fp32() ('fp32') resize to the input size, from their own pieces and so with their bits.  Neither the
        full-resolution logits nor the 256-channel feature map at the input size are formed: hip.segment_render /
        hip.argmax_labels with size=x.shape[-2:] blend these logits exactly as the resize does.
        text_embeddings (K36): a float32 [P, 512] matrix on the device; the logits are then [B, P, ...] against IT, from operands
        of its own (the registered buffer and its cached operands are not touched).  None is the path above, bit for bit.
        Refused: a train-mode module (check_fp32's rule, in both precisions), and a linear probe, which sits behind the resize."""
        if precision not in ('bf16', 'fp32'):
            raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
        if self.if_linear_probing:
            raise NotImplementedError("logits_at_stride: the linear probe acts on the full-resolution logits (behind the resize); "
                                      "use forward / forward_fp32 and the same-size render")
        self.check_fp32()
        if precision == 'fp32':
            if x.dtype != torch.float32 or x.ndim != 4:
                raise ValueError("logits_at_stride takes a float32 [B, 3, H, W] image batch")
            return self.classifier.forward_fp32(self.backbone.forward_fp32(x), text_embeddings)[0]
        with engine.defer_bn_counters():
            return self.classifier(self.backbone(x), text_embeddings)[0].float()

    def _forward_fp32(self, name, x, train, want_feats):
        """What forward_fp32 (`name`, train=False) and forward_fp32_train share: the input check, the network in its mode, the two
        resizes to the input size and the linear probe."""
        if x.dtype != torch.float32 or x.ndim != 4:
            raise ValueError(f"{name} takes a float32 [B, 3, H, W] image batch")
        input_shape = x.shape[-2:]
        if train:
            with engine.defer_bn_counters():
                logist, feats = self.classifier.forward_fp32_autograd(self.backbone.forward_fp32_autograd(x))
        else:
            logist, feats = self.classifier.forward_fp32(self.backbone.forward_fp32(x))
        logist = hip.bilinear_resize(logist, size=input_shape, align_corners=False)
        if isinstance(want_feats, str):
            if want_feats != 'lazy':
                raise ValueError(f"want_feats must be False, True or 'lazy', got {want_feats!r}")
            # the consumers pool the map over superpixels and take its L1 distance to another one (OpenESSModel): both work on
            # the map at the network's stride (hip.UpsampledFeature.pool, hip.upsampled_l1_mean)
            feats = hip.UpsampledFeature(feats, input_shape, align_corners=False)
        else:
            feats = hip.bilinear_resize(feats, size=input_shape, align_corners=False) if want_feats else None
        if self.if_linear_probing:
            logist = hip.linear_probe(logist, self.linear_probe)
        return logist, feats

    def forward(self, x):
        input_shape = x.shape[-2:]
        with engine.defer_bn_counters():              # one multi-tensor add for all BatchNorm step counters
            features = self.backbone(x)
            logist, feats = self.classifier(features)
        logist = hip.bilinear_resize(logist.float(), size=input_shape, align_corners=False)      # deeplabv3.py:183
        # deeplabv3.py:184.  feats_fp32: the full-resolution 256-channel map leaves in fp32 (interpolated from the bf16 OS16 map
        # without a second rounding): what the superpixel pooling / InfoNCE / L1 consistency losses consume
        if self.lazy_feats and torch.is_grad_enabled():
            # the consumer only pools the features over superpixels (PretrainStep, frame2recon + contrastive): hip.UpsampledFeature
            # multiplies the OS16 map with the pooling matrix instead of forming the full-resolution tensor
            feats = hip.UpsampledFeature(feats.float() if self.feats_fp32 else feats, input_shape, align_corners=False)
        else:
            feats = hip.bilinear_resize(feats.float() if self.feats_fp32 else feats, size=input_shape, align_corners=False)
        if self.if_linear_probing:
            logist = hip.linear_probe(logist, self.linear_probe)
        return logist, feats
