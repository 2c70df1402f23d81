"""Host-side checks of the fp32 DeepLabv3-R50 inference path (K16): the model's fp32 entry points and what they refuse, the
float64 BatchNorm fold, the operand cache keyed by parameter AND running-statistic versions, the argument checks of the new
C entry points, and the frame2recon wiring of the trainer and of tools/eval_precision.py.  No GPU."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL, ENOMEM = -22, -12


def _net(**kw):
    from openess_amd.models.deeplabv3 import deeplabv3_resnet50
    return deeplabv3_resnet50(num_classes=11, text_embeddings_path=None, output_stride=16, pretrained_backbone='', **kw)


def test_fp32_entry_points_exist_and_refuse_train_mode():
    net = _net()
    assert callable(net.forward_fp32) and callable(net.check_fp32)
    net.train()
    with pytest.raises(NotImplementedError, match="train mode"):
        net.check_fp32()
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        net.forward_fp32(torch.zeros(1, 3, 32, 32))
    net.eval()
    net.check_fp32()
    net.backbone.layer3[2].bn2.train()               # one BatchNorm left in train mode is named
    with pytest.raises(NotImplementedError, match=r"backbone\.layer3\.2\.bn2"):
        net.check_fp32()
    net.eval()
    net.classifier.ASPP.project[3].train()
    with pytest.raises(NotImplementedError, match="dropout"):
        net.check_fp32()
    net.eval()
    with pytest.raises(ValueError, match="float32"):
        net.forward_fp32(torch.zeros(1, 3, 32, 32, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # eval mode, fp32 input: the kernels refuse CPU tensors
        net.forward_fp32(torch.zeros(1, 3, 32, 32))


@pytest.mark.parametrize("Cout,Cin,k,dil,bias", [(64, 3, 7, 1, False), (32, 48, 3, 12, False), (24, 16, 1, 1, True)])
def test_batchnorm_fold_in_float64(Cout, Cin, k, dil, bias):
    """conv -> BatchNorm2d.eval() against the folded conv, both in float64, on random running statistics: relerr <= 1e-12 (the
    bound of compose_head_f64's test); the cached fp32 operand is that fold rounded once."""
    from openess_amd import hip
    from openess_amd.models._resnet import HipConv2d, fold_conv_bn_f64
    g = torch.Generator().manual_seed(Cout + k)
    conv = HipConv2d(Cin, Cout, k, padding=dil * (k // 2), dilation=dil, bias=bias)
    bn = torch.nn.BatchNorm2d(Cout).eval()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
        if bias:
            conv.bias.copy_(torch.randn(Cout, generator=g))
        bn.weight.copy_(torch.randn(Cout, generator=g))
        bn.bias.copy_(torch.randn(Cout, generator=g))
        bn.running_mean.copy_(torch.randn(Cout, generator=g) * 3)
        bn.running_var.copy_(torch.rand(Cout, generator=g) * 4 + 0.01)
    x = torch.randn(2, Cin, 9, 11, generator=g, dtype=torch.float64)
    w64, b64 = fold_conv_bn_f64(conv, bn)
    assert w64.dtype == b64.dtype == torch.float64
    import copy
    c64, bn64 = copy.deepcopy(conv).double(), copy.deepcopy(bn).double()
    with torch.no_grad():
        want = bn64(F.conv2d(x, c64.weight, c64.bias, 1, conv.padding, conv.dilation))
        got = F.conv2d(x, w64, b64, 1, conv.padding, conv.dilation)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"[deeplab_fp32] fold {Cout}x{Cin}x{k}x{k}: {err:.3e} (bound 1e-12)")
    assert err <= 1e-12
    op = conv._pw32.get(conv.weight, conv.bias, bn)
    assert torch.equal(op.packed, hip.pack_conv_weight_f32(w64.float())) and torch.equal(op.bias, b64.float())


def test_operand_cache_repacks_on_parameter_and_running_statistic_updates_only(monkeypatch):
    from openess_amd import hip
    net = _net().eval()
    calls = []
    real = hip.pack_conv_weight_f32
    monkeypatch.setattr(hip, "pack_conv_weight_f32", lambda w: (calls.append(tuple(w.shape)), real(w))[1])
    conv, bn = net.backbone.conv1, net.backbone.bn1
    get = lambda: conv._pw32.get(conv.weight, conv.bias, bn)     # noqa: E731  (what conv_bn_f32 asks for)
    op = get()
    assert calls == [(64, 3, 7, 7)] and op.packed.shape == (160, 64) and op.bias.shape == (64,)
    get(), get()
    assert len(calls) == 1                                        # nothing moved: no re-pack
    with torch.no_grad():
        conv.weight.mul_(2.0)                                     # an optimiser step: in place, the version counter moves
    get(), get()
    assert len(calls) == 2
    with torch.no_grad():
        bn.bias.add_(1.0)
    get()
    assert len(calls) == 3
    bias_before = get().bias.clone()
    with torch.no_grad():
        bn.running_mean.add_(1.0)                                 # a running statistic alone
    assert len(calls) == 3 and not torch.equal(get().bias, bias_before) and len(calls) == 4
    packed_before = get().packed.clone()
    bn.train()
    bn(torch.randn(2, 64, 5, 5) * 3)                              # what a training step does to the running statistics
    bn.eval()
    assert not torch.equal(get().packed, packed_before) and len(calls) == 5
    get()
    assert len(calls) == 5
    net.load_state_dict(net.state_dict())                         # copies in place: one re-pack
    get(), get()
    assert len(calls) == 6
    # the text-embedding operand of the head: composed from the parameter, the same rule
    head = net.classifier
    te = head.text_embeddings
    text = lambda: head._pw_text32.get_composed([te], lambda: (te.detach().double()[:, :, None, None], None))   # noqa: E731
    text(), text()
    assert len(calls) == 7 and calls[-1] == (11, 512, 1, 1)
    with torch.no_grad():
        te.mul_(0.5)
    text(), text()
    assert len(calls) == 8


def _views():
    from openess_amd import _lib
    buf = (ctypes.c_float * 4096)()
    addr = ctypes.addressof(buf)
    addr += (-addr) % 16
    return buf, addr, _lib.F32View(addr, 1024, 128, 16, 1), _lib.F32View(None, 1024, 128, 16, 1)


def test_dilated_conv_entry_validates_arguments_on_the_host():
    from openess_amd import _lib
    lib = _lib.load()
    buf, addr, ok, null = _views()
    r = ctypes.byref
    conv = lib.oess_conv2d_dilated_fwd_f32

    def call(vin=r(ok), vout=r(ok), B=1, H=8, W=8, Cin=16, w=addr, Cout=16, R=3, S=3, stride=1, pad=1, dil=1, act=0, res=None):
        return conv(vin, None, B, H, W, Cin, 0, w, None, Cout, R, S, stride, pad, dil, act, res, vout, None)

    assert call(vin=None) == EINVAL and call(vin=r(null)) == EINVAL              # null views
    assert call(vout=None) == EINVAL and call(vout=r(null)) == EINVAL
    assert call(res=r(null)) == EINVAL and call(w=None) == EINVAL
    assert call(dil=0) == EINVAL and call(dil=-2) == EINVAL                      # dilation < 1
    assert call(dil=64, pad=64) == EINVAL                                        # tap offset 2 * 64 = 128 > signed char
    assert call(R=7, S=7, dil=22, pad=66) == EINVAL                              # 6 * 22 = 132
    assert call(R=8, S=8, pad=3) == EINVAL and call(R=7, S=8, pad=3) == EINVAL   # R * S > 49
    assert call(R=5, S=10, pad=2) == EINVAL                                      # 50 taps
    assert call(H=4, W=4, dil=6, pad=0) == EINVAL                                # output extent < 1
    assert call(H=12, W=4, dil=6, pad=0) == EINVAL                               # one of the two extents
    assert call(R=7, S=7, H=6, W=6, pad=0) == EINVAL
    assert call(pad=-1) == EINVAL and call(stride=3) == EINVAL and call(act=3) == EINVAL
    # the K14 entry keeps its limits: 25 taps, pad < R
    old = lib.oess_conv2d_fwd_f32
    assert old(r(ok), None, 1, 8, 8, 3, 0, addr, None, 16, 7, 7, 2, 3, 0, None, r(ok), None) == EINVAL
    assert old(r(ok), None, 1, 8, 8, 16, 0, addr, None, 16, 3, 3, 1, 3, 0, None, r(ok), None) == EINVAL
    # packing: the 7 x 7 stem has a size, what the entry refuses has none
    assert lib.oess_conv2d_f32_packed_floats(64, 3, 7, 7) == 160 * 64
    assert lib.oess_conv2d_f32_packed_floats(256, 2048, 3, 3) == 9 * 2048 * 256
    assert lib.oess_conv2d_f32_packed_floats(64, 3, 8, 8) == 0 and lib.oess_conv2d_f32_packed_floats(64, 3, 7, 8) == 0


def test_pooling_entries_validate_arguments_on_the_host():
    from openess_amd import _lib
    lib = _lib.load()
    buf, addr, ok, null = _views()
    r = ctypes.byref
    pool = lib.oess_maxpool3x3s2_fwd_f32
    assert pool(None, 1, 4, 4, 4, r(ok), None) == EINVAL and pool(r(null), 1, 4, 4, 4, r(ok), None) == EINVAL
    assert pool(r(ok), 1, 4, 4, 4, None, None) == EINVAL and pool(r(ok), 1, 4, 4, 4, r(null), None) == EINVAL
    for B, H, W, C in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0)):
        assert pool(r(ok), B, H, W, C, r(ok), None) == EINVAL
    need = lib.oess_global_avg_pool_f32_workspace_bytes
    assert need(8, 28, 40, 2048) >= 8 * 2048 * 4 and need(0, 28, 40, 2048) == 0 and need(1, 4, 4, 0) == 0
    gap = lib.oess_global_avg_pool_fwd_f32
    assert gap(None, 1, 4, 4, 4, addr, addr, 1 << 20, None) == EINVAL
    assert gap(r(null), 1, 4, 4, 4, addr, addr, 1 << 20, None) == EINVAL
    assert gap(r(ok), 1, 4, 4, 4, None, addr, 1 << 20, None) == EINVAL
    assert gap(r(ok), 1, 4, 4, 4, addr, None, 1 << 20, None) == EINVAL
    assert gap(r(ok), 1, 4, 4, 4, addr, addr + 4, 1 << 20, None) == EINVAL       # workspace not 16-byte aligned
    for B, H, W, C in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0)):
        assert gap(r(ok), B, H, W, C, addr, addr, 1 << 20, None) == EINVAL
    assert gap(r(ok), 1, 4, 4, 4, addr, addr, 16, None) == ENOMEM


def test_wrappers_refuse_cpu_tensors():
    from openess_amd import hip
    x = torch.zeros(1, 16, 6, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.max_pool_3x3s2_f32(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.global_avg_pool_f32(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.conv2d_f32(x, torch.zeros(144, 32), None, 16, 3, 3, pad=2, dilation=2)


def test_eval_precision_tool_builds_frame2recon_without_the_refused_key(monkeypatch):
    """Host logic of tools/eval_precision.py: frame2recon is a choice, and the settings it hands to the trainer do not carry the
    key the frame2recon trainers refuse at construction; the event networks still get eval_precision: fp32."""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import eval_precision as tool
    import train
    from openess_amd.training._supervised import SupervisedTrainer
    seen = []
    monkeypatch.setattr(train, "build_trainer", lambda s: (seen.append(s), ("trainer", None))[1])
    trainer, s = tool.build(tool.DEFAULT, config_option='frame2recon')
    assert trainer == "trainer" and seen[-1] is s and s.config_option == 'frame2recon' and s.eval_precision == 'bf16'
    monkeypatch.setattr(SupervisedTrainer.__mro__[1], "__init__", lambda self, settings, train=True: None)
    SupervisedTrainer(s)                                         # the construction check passes (everything after it is stubbed)
    s.eval_precision = 'fp32'
    with pytest.raises(NotImplementedError, match="DeepLabv3") as e:
        SupervisedTrainer(s)
    assert "val_logits" in str(e.value) and "tools/eval_precision.py" in str(e.value) and "not wired" in str(e.value)
    _, s2 = tool.build(tool.DEFAULT, config_option='recon2voxel')
    assert s2.eval_precision == 'fp32'
    with pytest.raises(SystemExit):
        tool.main(["--config-option", "teacher"])


def test_val_logits_dispatches_frame2recon_fp32_and_restores_modes():
    """val_logits(batch, 'fp32') of a frame2recon trainer calls forward_fp32 on the eval-mode model and puts every module's
    train / eval flag back, also when the forward raises (here: a CPU model, whose kernels refuse)."""
    from types import SimpleNamespace
    from openess_amd.training._supervised import SupervisedTrainer
    tr = SupervisedTrainer.__new__(SupervisedTrainer)
    tr.settings, tr.eval_precision = SimpleNamespace(config_option='frame2recon'), 'bf16'
    net = _net().train()
    net.backbone.layer1.eval()                                   # a mixed state must come back as it was
    tr.models_dict = {'model_recon': net}
    modes = [m.training for m in net.modules()]
    seen = {}
    real = net.forward_fp32
    net.forward_fp32 = lambda x: (seen.update(training=net.training, bn=net.backbone.bn1.training), real(x))[1]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.val_logits((None, None, torch.zeros(1, 3, 32, 32)), precision='fp32')
    assert seen == {'training': False, 'bn': False}
    assert [m.training for m in net.modules()] == modes and net.training and not net.backbone.layer1.training
    with pytest.raises(ValueError, match="precision"):
        tr.val_logits((None, None, None), precision='fp16')
