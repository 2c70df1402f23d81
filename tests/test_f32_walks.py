"""The fp32 mirrors walk each network ONCE: ResNet / IntermediateLayerGetter through _resnet.walk_f32, SemSegE2VID through
_decoder_f32, every block through one body, each on the layer set of its mode.  Host only: a recording layer set stands in for
the kernels, so what is pinned here is the order of the layers, their flags and which layer set every public name hands over."""
from collections import OrderedDict

import pytest
import torch

from openess_amd import hip
from openess_amd.models import _resnet, deeplabv3
from openess_amd.models import style_networks as sn
from openess_amd.models._resnet import Bottleneck, ResNet


class Recorder:
    """A layer set's functions that launch nothing: they append (conv, norm, relu, residual is None) by module name and return a
    CPU tensor of the layer's output shape."""

    def __init__(self, net):
        self.names = {id(m): n for n, m in net.named_modules()}
        self.seen = []

    def conv_norm(self, conv, norm, x, relu=False, residual=None):
        self.seen.append((self.names[id(conv)], self.names[id(norm)], relu, residual is None))
        (k, _), s, p, d = conv.kernel_size, conv.stride[0], conv.padding[0], conv.dilation[0]
        B, Cin, H, W = x.shape
        assert Cin == conv.in_channels
        y = torch.zeros(B, conv.out_channels, (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1)
        assert residual is None or residual.shape == y.shape
        return y

    def max_pool(self, x):
        self.seen.append('maxpool')
        B, C, H, W = x.shape
        return torch.zeros(B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)

    def upsample_concat(self, x, skip=None):
        self.seen.append(('upsample2x', None if skip is None else skip.shape[1]))
        B, C, H, W = x.shape
        assert skip is None or (skip.shape[0], skip.shape[2], skip.shape[3]) == (B, 2 * H, 2 * W)
        return torch.zeros(B, C + (0 if skip is None else skip.shape[1]), 2 * H, 2 * W)

    def resnet_layers(self):
        return _resnet.F32Layers(self.conv_norm, self.max_pool)

    def decoder_layers(self):
        return sn.F32Layers(self.conv_norm, self.upsample_concat)


# stem, max pool, then conv1, conv2, the downsample conv (the residual's producer) and conv3 (+ residual, ReLU) of every block
RESNET_WALK = [
    ('conv1', 'bn1', True, True),
    'maxpool',
    ('layer1.0.conv1', 'layer1.0.bn1', True, True),
    ('layer1.0.conv2', 'layer1.0.bn2', True, True),
    ('layer1.0.downsample.0', 'layer1.0.downsample.1', False, True),
    ('layer1.0.conv3', 'layer1.0.bn3', True, False),
    ('layer2.0.conv1', 'layer2.0.bn1', True, True),
    ('layer2.0.conv2', 'layer2.0.bn2', True, True),
    ('layer2.0.downsample.0', 'layer2.0.downsample.1', False, True),
    ('layer2.0.conv3', 'layer2.0.bn3', True, False),
    ('layer3.0.conv1', 'layer3.0.bn1', True, True),
    ('layer3.0.conv2', 'layer3.0.bn2', True, True),
    ('layer3.0.downsample.0', 'layer3.0.downsample.1', False, True),
    ('layer3.0.conv3', 'layer3.0.bn3', True, False),
    ('layer4.0.conv1', 'layer4.0.bn1', True, True),
    ('layer4.0.conv2', 'layer4.0.bn2', True, True),
    ('layer4.0.downsample.0', 'layer4.0.downsample.1', False, True),
    ('layer4.0.conv3', 'layer4.0.bn3', True, False),
]

# five residual blocks (conv + norm + ReLU, conv + norm + residual) and a conv at 1/8, then two convs after each x2 + skip
DECODER_WALK = [
    ('decoder_scale_1.0.model.0', 'decoder_scale_1.0.model.1', True, True),
    ('decoder_scale_1.0.model.3', 'decoder_scale_1.0.model.4', False, False),
    ('decoder_scale_1.1.model.0', 'decoder_scale_1.1.model.1', True, True),
    ('decoder_scale_1.1.model.3', 'decoder_scale_1.1.model.4', False, False),
    ('decoder_scale_1.2.model.0', 'decoder_scale_1.2.model.1', True, True),
    ('decoder_scale_1.2.model.3', 'decoder_scale_1.2.model.4', False, False),
    ('decoder_scale_1.3.model.0', 'decoder_scale_1.3.model.1', True, True),
    ('decoder_scale_1.3.model.3', 'decoder_scale_1.3.model.4', False, False),
    ('decoder_scale_1.4.model.0', 'decoder_scale_1.4.model.1', True, True),
    ('decoder_scale_1.4.model.3', 'decoder_scale_1.4.model.4', False, False),
    ('decoder_scale_1.5.model.0', 'decoder_scale_1.5.model.1', True, True),
    ('upsample2x', 16),
    ('decoder_scale_2.0.model.0', 'decoder_scale_2.0.model.1', True, True),
    ('decoder_scale_2.1.model.0', 'decoder_scale_2.1.model.1', True, True),
    ('upsample2x', 8),
    ('decoder_scale_3.0.model.0', 'decoder_scale_3.0.model.1', True, True),
    ('decoder_scale_3.1.model.0', 'decoder_scale_3.1.model.1', True, True),
    ('upsample2x', None),
    ('decoder_scale_4.0.model.0', 'decoder_scale_4.0.model.1', True, True),
]


@pytest.fixture(scope="module")
def nets():
    torch.manual_seed(0)
    net = ResNet(Bottleneck, [1, 1, 1, 1], replace_stride_with_dilation=[False, True, True])
    getter = deeplabv3.IntermediateLayerGetter(net, OrderedDict([('layer2', 'mid'), ('layer4', 'out')]))
    dec = sn.SemSegE2VID(32, 5, skip_connect=True, skip_type='concat', text_embeddings_path=None)
    return net, getter, dec


def _latents():
    return {1: torch.zeros(1, 4, 16, 24), 2: torch.zeros(1, 8, 8, 12), 4: torch.zeros(1, 16, 4, 6), 8: torch.zeros(1, 32, 2, 3)}


def test_layer_sets_hold_the_functions_of_their_mode():
    for got, want in ((_resnet.F32_EVAL, (_resnet.conv_bn_f32, hip.max_pool_3x3s2_f32)),
                      (_resnet.F32_AS_FLAGGED, (_resnet.conv_bn_any_f32, hip.max_pool_3x3s2_f32)),
                      (_resnet.F32_AUTOGRAD, (_resnet.conv_bn_f32_autograd, hip.max_pool_3x3s2_f32_train)),
                      (sn.F32_EVAL, (sn._conv_norm_f32, hip.upsample2x_concat_f32)),
                      (sn.F32_TRAIN, (sn._conv_norm_f32_train, hip.upsample2x_concat_f32_train))):
        assert len(got) == len(want) and all(g is w for g, w in zip(got, want))


def test_resnet_walk_visits_the_written_sequence(nets):
    net, getter, _ = nets
    rec = Recorder(net)
    y, kept = _resnet.walk_f32(net, torch.zeros(1, 3, 32, 32), rec.resnet_layers())
    assert rec.seen == RESNET_WALK
    assert y.shape == (1, 2048, 4, 4) and not kept            # layer3 and layer4 dilated: the stride stays 8


def test_getter_walk_is_the_resnet_walk_and_returns_its_keys_in_order(nets):
    net, getter, _ = nets
    rec = Recorder(getter)
    y, kept = _resnet.walk_f32(getter, torch.zeros(1, 3, 32, 32), rec.resnet_layers(), getter.return_layers)
    assert rec.seen == RESNET_WALK
    assert list(kept) == ['mid', 'out'] and kept['mid'].shape == (1, 512, 4, 4) and kept['out'] is y


@pytest.mark.parametrize("which, public", [("F32_EVAL", ("forward_fp32",)), ("F32_AS_FLAGGED", ("features_fp32",)),
                                           ("F32_AUTOGRAD", ("features_fp32_autograd", "forward_fp32_autograd"))])
def test_public_resnet_names_walk_the_same_sequence_on_their_layer_set(nets, monkeypatch, which, public):
    """Only the named set is replaced by the recorder; the other two stay the real ones and would need a GPU."""
    net, getter, _ = nets
    rec = Recorder(net)
    monkeypatch.setattr(_resnet, which, rec.resnet_layers())
    x = torch.zeros(1, 3, 32, 32)
    for name in public:
        rec.seen.clear()
        if hasattr(net, name):
            assert getattr(net, name)(x).shape == (1, 2048, 4, 4)
        else:
            assert list(getattr(getter, name)(x)) == ['mid', 'out']
        assert rec.seen == RESNET_WALK, name


@pytest.mark.parametrize("name, which", [("forward_fp32", "F32_EVAL"), ("forward_train_fp32", "F32_AS_FLAGGED"),
                                         ("forward_fp32_autograd", "F32_AUTOGRAD")])
def test_bottleneck_names_share_one_body(monkeypatch, name, which):
    blk = Bottleneck(256, 64)                                  # no downsample conv: the input itself is the residual
    rec = Recorder(blk)
    monkeypatch.setattr(_resnet, which, rec.resnet_layers())
    assert getattr(blk, name)(torch.zeros(1, 256, 5, 7)).shape == (1, 256, 5, 7)
    assert rec.seen == [('conv1', 'bn1', True, True), ('conv2', 'bn2', True, True), ('conv3', 'bn3', True, False)]


@pytest.mark.parametrize("name, which, kw", [("forward_fp32", "F32_EVAL", dict(out=None)), ("forward_fp32_autograd", "F32_AUTOGRAD", {})])
def test_conv_bn_relu_names_share_one_body(monkeypatch, name, which, kw):
    m = deeplabv3.ASPPConv(16, 8, 3)
    rec, seen_kw = Recorder(m), []

    def conv_bn(conv, bn, x, relu=False, **k):                 # out=: what only the eval set is handed
        seen_kw.append(k)
        return rec.conv_norm(conv, bn, x, relu)
    monkeypatch.setattr(_resnet, which, _resnet.F32Layers(conv_bn, rec.max_pool))
    assert getattr(m, name)(torch.zeros(1, 16, 5, 7), **kw).shape == (1, 8, 5, 7)
    assert rec.seen == [('0', '1', True, True)] and seen_kw == [kw]


def test_decoder_walk_visits_the_written_sequence(nets):
    dec = nets[2]
    rec, lat = Recorder(dec), _latents()
    out, x = dec._decoder_f32('forward_fp32', lat, rec.decoder_layers())
    assert rec.seen == DECODER_WALK
    assert list(out) == [8, 4, 2] and out[8] is lat[8] and out[4].shape == (1, 8, 4, 6) and out[2].shape == (1, 8, 8, 12)
    assert x.shape == (1, 4, 16, 24)


class _Reached(Exception):
    pass


@pytest.mark.parametrize("name, which", [("forward_fp32", "F32_EVAL"), ("forward_fp32_train", "F32_TRAIN")])
def test_decoder_entry_points_reach_the_walk_with_their_layer_set(nets, monkeypatch, name, which):
    dec = nets[2]

    def spy(self, called, input_dict, layers):
        raise _Reached(called, layers)
    monkeypatch.setattr(sn.SemSegE2VID, "_decoder_f32", spy)
    with pytest.raises(_Reached) as e:
        getattr(dec, name)(_latents())
    assert e.value.args[0] == name and e.value.args[1] is getattr(sn, which)


@pytest.mark.parametrize("name, which", [("forward_f32", "F32_EVAL"), ("forward_f32_train", "F32_TRAIN")])
def test_decoder_block_names_share_one_body(nets, monkeypatch, name, which):
    dec = nets[2]
    rec = Recorder(dec)
    monkeypatch.setattr(sn, which, rec.decoder_layers())
    x = torch.zeros(1, 32, 2, 3)
    assert getattr(dec.decoder_scale_1[0], name)(x).shape == x.shape
    assert getattr(dec.decoder_scale_1[5], name)(x).shape == (1, 16, 2, 3)
    assert rec.seen == DECODER_WALK[:2] + [DECODER_WALK[10]]
    with pytest.raises(NotImplementedError, match="no dropout"):
        sn.INSResBlock(8, 8, dropout=0.5).forward_f32_train(torch.zeros(1, 8, 2, 3))
