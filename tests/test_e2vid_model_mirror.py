"""CPU-side checks of the E2VID model mirror's host plumbing: the one eval-mode BatchNorm fold (engine.fold_bn) against the
formula written out here, and the state_dict names the reference's checkpoints load by."""
import pytest
import torch
import torch.nn as nn

from oracle.step import E2VID_LIGHTWEIGHT_CONFIG


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("has_bias", [False, True])
@pytest.mark.parametrize("transposed", [False, True])
def test_fold_bn_is_the_formula(transposed, has_bias, dtype):
    """scale = gamma / sqrt(var + eps), w * scale over the output-channel dimension, (b0 - mean) * scale + beta, in the dtype of
    the weight handed in: exact equality, the helper is this formula."""
    from openess_amd import engine
    torch.manual_seed(7)
    Cin, Cout = 6, 10
    w = torch.randn((Cin, Cout, 5, 5) if transposed else (Cout, Cin, 3, 3)).to(dtype)      # ConvTranspose2d / Conv2d weight
    b = torch.randn(Cout).to(dtype) if has_bias else None
    bn = nn.BatchNorm2d(Cout).eval()
    with torch.no_grad():
        bn.weight.normal_(), bn.bias.normal_(), bn.running_mean.normal_(), bn.running_var.uniform_(0.1, 3.0)
    scale = bn.weight.detach().to(dtype) / torch.sqrt(bn.running_var.detach().to(dtype) + bn.eps)
    w_ref = w * (scale[None, :, None, None] if transposed else scale[:, None, None, None])
    b_ref = ((torch.zeros_like(scale) if b is None else b) - bn.running_mean.detach().to(dtype)) * scale + bn.bias.detach().to(dtype)
    w_out, b_out = engine.fold_bn(w, b, bn, 1 if transposed else 0)
    assert w_out.dtype == dtype and b_out.dtype == dtype
    assert torch.equal(w_out, w_ref) and torch.equal(b_out, b_ref)
    w_same, b_same = engine.fold_bn(w, b, None)                                              # nothing to fold
    assert w_same is w and b_same is b


def test_param_versions_follow_every_tensor():
    from openess_amd import engine
    conv, bn = nn.Conv2d(4, 8, 3), nn.BatchNorm2d(8)
    keys = [engine.param_versions(conv.weight, conv.bias, bn)]
    with torch.no_grad():
        for t in (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var):
            t.add_(1.0)
            keys.append(engine.param_versions(conv.weight, conv.bias, bn))
    assert len(set(keys)) == len(keys)
    assert engine.param_versions(conv.weight) == (conv.weight._version, None, None)


_BN = ['weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked']
_IN = ['running_mean', 'running_var', 'num_batches_tracked']                   # InstanceNorm2d(track_running_stats=True): no affine


def _norm_keys(prefix, names):
    return [f'{prefix}.{n}' for n in names]


@pytest.mark.parametrize("cls_name, conv", [("ConvLayer", "conv2d"), ("TransposedConvLayer", "transposed_conv2d"),
                                            ("UpsampleConvLayer", "conv2d")])
def test_layer_state_dict_keys(cls_name, conv):
    from openess_amd.e2vid.model import submodules
    cls = getattr(submodules, cls_name)
    assert list(cls(8, 16, 5, padding=2, norm=None).state_dict()) == [f'{conv}.weight', f'{conv}.bias']
    assert list(cls(8, 16, 5, padding=2, norm='BN').state_dict()) == [f'{conv}.weight'] + _norm_keys('norm_layer', _BN)
    assert list(cls(8, 16, 5, padding=2, norm='IN').state_dict()) == [f'{conv}.weight', f'{conv}.bias'] + _norm_keys('norm_layer', _IN)


@pytest.mark.parametrize("use_upsample_conv", [False, True])
def test_unet_recurrent_state_dict_keys(use_upsample_conv):
    """The names (and order) the reference's E2VID_lightweight checkpoints are loaded by, strictly."""
    from openess_amd.e2vid.model.unet import UNetRecurrent
    c = E2VID_LIGHTWEIGHT_CONFIG
    net = UNetRecurrent(num_input_channels=c['num_bins'], num_output_channels=1, skip_type=c['skip_type'],
                        recurrent_block_type=c['recurrent_block_type'], activation='sigmoid', num_encoders=c['num_encoders'],
                        base_num_channels=c['base_num_channels'], num_residual_blocks=c['num_residual_blocks'], norm=c['norm'],
                        use_upsample_conv=use_upsample_conv)
    expected = ['head.conv2d.weight', 'head.conv2d.bias']
    for i in range(3):
        expected += [f'encoders.{i}.conv.conv2d.weight'] + _norm_keys(f'encoders.{i}.conv.norm_layer', _BN)
        expected += [f'encoders.{i}.recurrent_block.Gates.weight', f'encoders.{i}.recurrent_block.Gates.bias']
    for i in range(2):
        expected += [f'resblocks.{i}.conv1.weight'] + _norm_keys(f'resblocks.{i}.bn1', _BN) + _norm_keys(f'resblocks.{i}.bn2', _BN)
        expected += [f'resblocks.{i}.conv2.weight']
    dec = 'conv2d' if use_upsample_conv else 'transposed_conv2d'
    for i in range(3):
        expected += [f'decoders.{i}.{dec}.weight'] + _norm_keys(f'decoders.{i}.norm_layer', _BN)
    expected += ['pred.conv2d.weight'] + _norm_keys('pred.norm_layer', _BN)
    assert list(net.state_dict()) == expected
    # Conv2d keeps [Cout, Cin, k, k], ConvTranspose2d [Cin, Cout, k, k]: the dimension the BatchNorm scale is folded over
    assert tuple(net.state_dict()[f'decoders.0.{dec}.weight'].shape) == ((128, 256, 5, 5) if use_upsample_conv else (256, 128, 5, 5))
