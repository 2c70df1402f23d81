"""Host-side checks of the fp32 SemSegE2VID evaluation path (K15): the `eval_precision` setting, the float64 head
composition, the per-layer operand cache, and the argument checks of the new entry points.  No GPU."""
import ctypes
import os

import pytest
import torch
import yaml

CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs", "finetune_dsec_synthetic.yaml")


def _settings(tmp_path, **clip):
    from openess_amd.config.settings import Settings
    cfg = yaml.load(open(CFG), yaml.Loader)
    cfg['clip'].update(clip)
    path = tmp_path / "settings.yaml"
    path.write_text(yaml.dump(cfg))
    return Settings(str(path), generate_log=False)


def test_settings_eval_precision_values(tmp_path):
    assert _settings(tmp_path).eval_precision == 'bf16'
    assert _settings(tmp_path, eval_precision='bf16').eval_precision == 'bf16'
    assert _settings(tmp_path, eval_precision='fp32').eval_precision == 'fp32'
    for bad in ('fp16', 'FP32', 32, True):
        with pytest.raises(ValueError, match="eval_precision"):
            _settings(tmp_path, eval_precision=bad)


def test_frame2recon_trainer_refuses_fp32_at_construction(tmp_path):
    from openess_amd.training.finetune_trainer import OpenESSFineTuneModel
    from openess_amd.training.linear_probe_trainer import OpenESSLinearProbeModel
    s = _settings(tmp_path, eval_precision='fp32', config_option='frame2recon')
    for cls in (OpenESSFineTuneModel, OpenESSLinearProbeModel):
        with pytest.raises(NotImplementedError, match="DeepLabv3"):
            cls(settings=s)
    s.eval_precision = 'half'            # a value set past the YAML check is refused by the trainer as well
    with pytest.raises(ValueError, match="eval_precision"):
        OpenESSFineTuneModel(settings=s)


def test_composed_head_equals_the_three_maps_in_float64():
    from openess_amd.models.style_networks import compose_head_f64
    g = torch.Generator().manual_seed(3)
    w1, b1 = torch.randn(256, 32, 1, 1, generator=g), torch.randn(256, generator=g)
    w2, b2 = torch.randn(512, 256, 1, 1, generator=g), torch.randn(512, generator=g)
    t = torch.randn(11, 512, generator=g)
    W, b = compose_head_f64(w1, b1, w2, b2, t)
    assert W.dtype == b.dtype == torch.float64 and W.shape == (11, 32, 1, 1) and b.shape == (11,)
    x = torch.randn(2, 32, 5, 7, generator=g).double()
    F = torch.nn.functional
    want = F.conv2d(F.conv2d(F.conv2d(x, w1.double(), b1.double()), w2.double(), b2.double()), t.double()[:, :, None, None])
    got = F.conv2d(x, W, b)
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-12


def test_operand_cache_repacks_on_parameter_update_only(monkeypatch):
    from openess_amd import hip
    from openess_amd.models.style_networks import SemSegE2VID
    net = SemSegE2VID(256, 11, skip_connect=True, skip_type='concat', text_embeddings_path=None, if_linear_probing=True)
    calls = []
    real = hip.pack_conv_weight_f32
    monkeypatch.setattr(hip, "pack_conv_weight_f32", lambda w: (calls.append(tuple(w.shape)), real(w))[1])
    conv = net.decoder_scale_4[0].model[0]
    pw = conv._pw32.get(conv.weight, conv.bias)
    assert calls == [(32, 64, 3, 3)] and pw.packed.shape == (9 * 64, 32) and torch.equal(pw.bias, conv.bias.detach())
    assert torch.equal(pw.packed[:, :32], conv.weight.detach().permute(2, 3, 1, 0).reshape(-1, 32))
    conv._pw32.get(conv.weight, conv.bias)
    assert len(calls) == 1
    head = net._head_f32()
    assert len(calls) == 2 and calls[1] == (11, 32, 1, 1) and head.packed.shape == (32, 32)
    net._head_f32()
    assert len(calls) == 2
    before = head.packed.clone()
    with torch.no_grad():
        net.decoder_ch512[0].bias.add_(1.0)          # what an optimiser step does: in place, the version counter moves
        conv.weight.mul_(2.0)
    assert torch.equal(net._head_f32().packed, before) and len(calls) == 3      # the bias moved: weight equal, bias not
    assert not torch.equal(net._head_f32().bias, torch.zeros(11))
    conv._pw32.get(conv.weight, conv.bias)
    assert len(calls) == 4
    net.load_state_dict(net.state_dict())            # load_state_dict copies in place: everything repacks once
    conv._pw32.get(conv.weight, conv.bias), net._head_f32()
    conv._pw32.get(conv.weight, conv.bias), net._head_f32()
    assert len(calls) == 6


def test_new_entry_points_validate_arguments_on_the_host():
    from openess_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    addr = ctypes.addressof(buf)
    addr += (-addr) % 16
    ok = _lib.F32View(addr, 32, 16, 4, 1)
    null = _lib.F32View(None, 32, 16, 4, 1)
    r = ctypes.byref
    assert lib.oess_instance_norm_f32_workspace_bytes(2, 33, 47, 256) >= 2 * 256 * 2 * 4
    assert lib.oess_instance_norm_f32_workspace_bytes(0, 33, 47, 256) == 0
    assert lib.oess_instance_norm_f32_workspace_bytes(1, 4, 6, 0) == 0
    norm = lib.oess_instance_norm_fwd_f32
    assert norm(None, 1, 2, 2, 4, 1e-5, 0, None, r(ok), addr, 1 << 20, None) == -22
    assert norm(r(null), 1, 2, 2, 4, 1e-5, 0, None, r(ok), addr, 1 << 20, None) == -22
    assert norm(r(ok), 1, 2, 2, 4, 1e-5, 0, None, None, addr, 1 << 20, None) == -22
    assert norm(r(ok), 1, 2, 2, 4, 1e-5, 0, r(null), r(ok), addr, 1 << 20, None) == -22
    assert norm(r(ok), 1, 2, 2, 4, 1e-5, 0, None, r(ok), None, 1 << 20, None) == -22
    for B, H, W, C in ((0, 2, 2, 4), (1, 0, 2, 4), (1, 2, 0, 4), (1, 2, 2, 0)):
        assert norm(r(ok), B, H, W, C, 1e-5, 0, None, r(ok), addr, 1 << 20, None) == -22
    assert norm(r(ok), 1, 2, 2, 4, 1e-5, 2, None, r(ok), addr, 1 << 20, None) == -22
    assert norm(r(ok), 1, 2, 2, 4, -1.0, 0, None, r(ok), addr, 1 << 20, None) == -22
    assert norm(r(ok), 1, 2, 2, 4, 1e-5, 0, None, r(ok), addr, 16, None) == -12          # OESS_ENOMEM: workspace too small
    up = lib.oess_upsample_nearest2x_concat_f32
    assert up(None, 1, 2, 2, 4, None, 0, r(ok), None) == -22
    assert up(r(null), 1, 2, 2, 4, None, 0, r(ok), None) == -22
    assert up(r(ok), 1, 2, 2, 4, None, 0, None, None) == -22
    assert up(r(ok), 1, 2, 2, 4, r(null), 4, r(ok), None) == -22
    assert up(r(ok), 1, 2, 2, 4, None, 4, r(ok), None) == -22            # channels of a skip that is not there
    assert up(r(ok), 1, 2, 2, 4, r(ok), 0, r(ok), None) == -22
    for B, H, W, C in ((0, 2, 2, 4), (1, 0, 2, 4), (1, 2, 0, 4), (1, 2, 2, 0)):
        assert up(r(ok), B, H, W, C, None, 0, r(ok), None) == -22


def test_wrappers_refuse_cpu_tensors():
    from openess_amd import hip
    x = torch.zeros(1, 4, 2, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.instance_norm_f32(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.upsample2x_concat_f32(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.upsample2x_concat_f32(x, torch.zeros(1, 4, 4, 4))


def test_check_fp32_refuses_what_is_not_built():
    from openess_amd.models.style_networks import INSResBlock, SemSegE2VID
    net = SemSegE2VID(256, 11, skip_connect=True, skip_type='sum', text_embeddings_path=None)
    with pytest.raises(NotImplementedError, match="concat"):
        net.check_fp32()
    with pytest.raises(NotImplementedError, match="concat"):
        net.forward_fp32({k: torch.zeros(1, 1, 1, 1) for k in (1, 2, 4, 8)})
    net = SemSegE2VID(256, 11, skip_connect=True, skip_type='concat', text_embeddings_path=None)
    net.check_fp32()
    net.decoder_scale_1[0] = INSResBlock(256, 256, dropout=0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        net.check_fp32()
