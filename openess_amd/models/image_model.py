"""Mirror of models/image_model.py:DilationFeatureExtractor (:90-143) and
models/modules/resnet_encoder.py:ResNetEncoder (:8-38): frozen dilated ResNet-50 (output stride 4),
trainable 1x1 decoder, x4 bilinear (align_corners=True), L2 normalisation over channels."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import engine, hip
from ._resnet import Bottleneck, HipConv2d, ResNet, conv_f32


class ResNetEncoder(ResNet):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        del self.fc
        del self.avgpool

    def forward(self, x, want_output=True):
        return self.features(x, want_output=want_output)

    def load_state_dict(self, state_dict, **kwargs):
        state_dict.pop("fc.bias", None)
        state_dict.pop("fc.weight", None)
        return super().load_state_dict(state_dict, **kwargs)


# image_weights names -> (key of the state dict inside the file | None for the file itself, prefix kept and removed | None for
# every key, prefix dropped although it starts with the kept one | None): the key rules of models/image_model.py:46-74
IMAGE_WEIGHTS = {
    'imagenet': (None, None, None),                 # plain torchvision ResNet-50 (fc.* dropped by ResNetEncoder.load_state_dict)
    'dino': (None, None, None),
    'moco_v1': ('state_dict', 'module.encoder_q.', 'module.encoder_q.fc'),
    'moco_v2': ('state_dict', 'module.encoder_q.', 'module.encoder_q.fc'),
    'moco_coco': ('state_dict', 'module.encoder_q.', 'module.encoder_q.fc'),
    'swav': (None, 'module.', 'module.pro'),
    'deepcluster_v2': (None, 'module.', 'module.pro'),
    'obow': ('network', None, None),
    'pixpro': ('model', 'module.encoder.', None),
}


def adapt_weights(architecture, path):
    """The ResNet-50 state dict of the self-supervised checkpoint `path` in the layout `architecture` names (IMAGE_WEIGHTS), on
    the CPU.  The file is local: the reference downloads it to weights/<architecture>.pt (image_model.py:38-42), nothing here
    fetches anything."""
    if architecture not in IMAGE_WEIGHTS:
        raise ValueError(f"image_weights: {architecture!r} is none of {sorted(IMAGE_WEIGHTS)}")
    inner, keep, drop = IMAGE_WEIGHTS[architecture]
    weights = torch.load(path, map_location='cpu')
    if inner is not None:
        weights = weights[inner]
    if keep is None:
        return dict(weights)
    # (the reference writes k.replace(keep, ""); on keys that start with `keep` and hold it once that is the prefix removed)
    return {k.replace(keep, ""): v for k, v in weights.items()
            if k.startswith(keep) and not (drop is not None and k.startswith(drop))}


class DilationFeatureExtractor(nn.Module):
    def __init__(self, image_weights=None, preprocessing=None, weights_path=None):
        """image_weights: None / '' / 'none' / 'random' load nothing; a name of IMAGE_WEIGHTS loads the frozen encoder (strict)
        from `weights_path`, or -- None -- from weights/<image_weights>.pt under the working directory.  A file that does not
        exist is an error here: training.pretrained.teacher_path is where a missing file is tolerated."""
        super().__init__()
        self.encoder = ResNetEncoder(block=Bottleneck, layers=[3, 4, 6, 3], replace_stride_with_dilation=[True, True, True])
        if image_weights not in (None, '', 'none', 'random'):
            self.encoder.load_state_dict(adapt_weights(image_weights, weights_path or f"weights/{image_weights}.pt"))
        for p in self.encoder.parameters():
            p.requires_grad = False
        self.decoder = nn.Sequential(HipConv2d(2048, 256, 1), nn.Upsample(scale_factor=4, mode="bilinear", align_corners=True))
        self.preprocessing = preprocessing
        self.normalize_feature = True
        # True: the differentiable path returns hip.UpsampledNormalizedFeature (x, 4) for a consumer that only pools the features
        # over superpixels (PretrainStep with the contrastive loss); its .materialize() is the tensor this module returns otherwise
        self.lazy_features = False
        self._pw32_head_train = engine.PackedWeightF32()     # operands of head_fp32_train, per version of the head's parameters

    def forward(self, x):
        return self.head(self.encode(x))

    def encode(self, x, want_output=True):
        """The frozen part (preprocessing + dilated ResNet-50, train-mode BatchNorm side effects included): depends on no trainable
        weight, so a training loop may run it for the NEXT batch while the current one is still in its backward pass.
        want_output=False: the caller reads no features and runs the encoder for those side effects alone (pixel distillation);
        every running statistic and batch counter moves as ever, the last block's result is not produced, None comes back."""
        if self.preprocessing:
            x = self.preprocessing(x)
        x = engine.to_cl_bf16(x)
        with torch.no_grad():                      # encoder params are frozen (image_model.py:113-114)
            return self.encoder(x, want_output=want_output)

    def head(self, x):
        """The trainable 1x1 decoder + x4 bilinear + L2 normalisation on the encoder's output."""
        x = self.decoder[0](x)
        if torch.is_grad_enabled() and x.requires_grad:
            # differentiable path (contrastive loss active)
            if self.normalize_feature and x.dtype == torch.bfloat16 and x.shape[1] % 64 == 0 and x.shape[1] <= 512:
                if self.lazy_features:
                    return hip.UpsampledNormalizedFeature(x, 4)
                return hip.bilinear_l2norm_train(x, 4)            # one fused forward kernel + (L2 adjoint, bilinear adjoint)
            x = hip.bilinear_resize(x, scale_factor=4, align_corners=True)
            return hip.l2_normalize(x) if self.normalize_feature else x
        return hip.bilinear_l2norm(x, 4, self.normalize_feature)

    @torch.no_grad()
    def forward_fp32(self, x):
        """forward() in fp32, the reference's own arithmetic, on the f32-input MFMA kernels: x fp32 [B, 3, H, W]
        -> fp32 [B, 256, H, W] unit-norm features.  Inference only (no autograd: the trainable head's backward stays bf16).
        Every BatchNorm runs in the form its `training` flag asks for: in train mode (how the reference leaves its frozen
        encoder) one call moves every running statistic one momentum step, as one forward() does; in eval mode the folded
        convs of K16.  No buffer, operand or workspace is shared with forward()."""
        return self.head_fp32(self.encode_fp32(x))

    @torch.no_grad()
    def encode_fp32(self, x):
        if self.preprocessing:
            x = self.preprocessing(x)
        if x.dtype != torch.float32 or x.ndim != 4:
            raise ValueError("forward_fp32 takes a float32 [B, 3, H, W] image batch")
        return self.encoder.features_fp32(x)

    @torch.no_grad()
    def head_fp32(self, x):
        x = conv_f32(self.decoder[0], x)
        x = hip.bilinear_resize(x, scale_factor=4, align_corners=True)
        return hip.l2_normalize(x) if self.normalize_feature else x

    def head_fp32_train(self, x):
        """The trainable head under autograd in fp32 (K20): hip.conv2d_f32_train on decoder[0], then -- with lazy_features --
        hip.UpsampledNormalizedFeature(x, 4), whose pool() is the fused fp32 head-pool node (no full-resolution tensor), or
        without it the materialised fp32 chain bilinear_resize -> l2_normalize.  x: the fp32 output of encode_fp32."""
        if x.dtype != torch.float32:
            raise ValueError("head_fp32_train takes the float32 output of encode_fp32")
        conv = self.decoder[0]
        x = hip.conv2d_f32_train(x, conv.weight, conv.bias, conv.stride[0], conv.padding[0], conv.dilation[0], pw=self._pw32_head_train)
        if self.normalize_feature:
            feat = hip.UpsampledNormalizedFeature(x, 4)
            return feat if self.lazy_features else feat.materialize()
        return hip.bilinear_resize(x, scale_factor=4, align_corners=True)
