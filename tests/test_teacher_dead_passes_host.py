"""Host side of the frozen teacher's removed BatchNorm passes (EXPERIMENTS.md R6-13): the eligibility rule, the argument checks of
the three new entry points (they return before any launch) and the switches.  No GPU."""
import pytest
import torch


def test_separate_apply_rule_is_the_small_map_threshold():
    from openess_amd import hip
    assert hip.BN_FUSED_MAX_TILES == 320
    assert not hip.conv_bn_train_separate_apply(1, 64)
    assert not hip.conv_bn_train_separate_apply(320 * 128, 256)            # 320 tiles: the one-launch statistics + apply kernel
    assert hip.conv_bn_train_separate_apply(320 * 128 + 1, 256)            # 321 tiles
    assert hip.conv_bn_train_separate_apply(2 * 144 * 144, 2048)           # 41 472 pixels = 324 tiles (2 x 3 x 576 x 576 at stride 4)
    assert hip.conv_bn_train_separate_apply(8 * 110 * 160, 64)             # the flagship's teacher maps
    assert not hip.conv_bn_train_separate_apply(2 * 16 * 24, 256)          # 2 x 3 x 64 x 96 at stride 4
    # a small map with a channel count the one-launch kernel does not take runs separate passes today, but is not eligible either
    assert not hip.conv_bn_train_separate_apply(100, 72)


def test_conv_bn_separable_needs_the_no_autograd_train_mode_route():
    from openess_amd.models import _resnet
    conv, bn = _resnet.conv1x1(64, 256), torch.nn.BatchNorm2d(256)
    x = torch.zeros(8, 64, 110, 160)
    assert not _resnet.conv_bn_separable(conv, bn, x)                      # a CPU tensor: nothing of the HIP path applies
    with pytest.raises(ValueError):
        _resnet.conv_bn(conv, bn, x, defer=True)
    with pytest.raises(ValueError):
        _resnet.conv_bn(conv, bn, x, want_output=False)

    class OnGpu:                                                           # what the rule reads of the tensor
        is_cuda, requires_grad, shape = True, False, (8, 64, 110, 160)
    for p in list(conv.parameters()) + list(bn.parameters()):
        p.requires_grad = False
    assert _resnet.conv_bn_separable(conv, bn, OnGpu)
    OnGpu.shape = (2, 64, 16, 24)
    assert not _resnet.conv_bn_separable(conv, bn, OnGpu)                  # small map
    OnGpu.shape = (8, 64, 110, 160)
    bn.eval()
    assert not _resnet.conv_bn_separable(conv, bn, OnGpu)                  # eval mode folds
    bn.train()
    conv.weight.requires_grad = True
    assert not _resnet.conv_bn_separable(conv, bn, OnGpu)                  # autograd
    with torch.no_grad():
        assert _resnet.conv_bn_separable(conv, bn, OnGpu)
    # the stem: 7 x 7 stride 2 pad 3 -> 288 x 288 x 2 = 1 296 tiles; at 64 x 96 -> 24 tiles
    stem = _resnet.HipConv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
    stem.weight.requires_grad = False
    bn1 = torch.nn.BatchNorm2d(64)
    with torch.no_grad():
        OnGpu.shape = (2, 8, 576, 576)
        assert _resnet.conv_bn_separable(stem, bn1, OnGpu)
        OnGpu.shape = (2, 8, 64, 96)
        assert not _resnet.conv_bn_separable(stem, bn1, OnGpu)


def test_switches_default_on():
    from openess_amd.models import _resnet, image_model
    assert _resnet.Bottleneck.fuse_downsample_bn and _resnet.Bottleneck.skip_dead_output and _resnet.ResNet.fuse_stem_pool
    assert image_model.ResNetEncoder.fuse_stem_pool


def test_new_entry_points_validate_on_the_host():
    from openess_amd import _lib, hip
    lib = _lib.load()
    assert lib.oess_norm_apply2_nhwc_bf16(None, 64, None, None, None, 64, None, None, 1, 10, 64, None, 64, None) == -22
    assert lib.oess_maxpool3x3s2_affine_relu_fwd_nhwc_bf16(None, 64, 1, 8, 8, 64, None, None, None, 64, None) == -22
    assert lib.oess_conv2d_stats_only_bf16(None, 256, 1, 256, 512, 256, None, 256, None, None) == -22
    # the store-free kernel exists where the storing call's plan is the w128 GEMM (host query; 256 CUs assumed without a GPU)
    assert hip.conv2d_route((1, 256, 512, 256), None, False, 256, 1, 1, tile_stats=True) == hip.ROUTE_CONV1X1_W128
    assert hip.conv2d_route((1, 255, 512, 256), None, False, 256, 1, 1, tile_stats=True) != hip.ROUTE_CONV1X1_W128
    # K = 64 (layer1's 64 -> 256 convs) is below the rule's K >= 256: those layers keep their storing kernel, only the apply goes
    assert hip.conv2d_route((1, 256, 512, 64), None, False, 256, 1, 1, tile_stats=True) != hip.ROUTE_CONV1X1_W128
    assert hip.conv2d_route((8, 110, 160, 512), None, False, 2048, 1, 1, tile_stats=True) == hip.ROUTE_CONV1X1_W128     # the last conv3
    assert lib.oess_conv2d_route_name(hip.ROUTE_CONV1X1_W128) == b"conv1x1_w128_kernel"
