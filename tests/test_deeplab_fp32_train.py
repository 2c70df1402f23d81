"""Host-side checks of the fp32 DeepLabv3-R50 training path (K22): the new C entry points and what they refuse, the model's
forward_fp32_train / check_fp32_train and what they refuse before any launch, that the K16 inference entry points behave as
before, and the per-call `precision` argument of the stage-2/3 trainers' step (frame2recon in fp32 is reached through it alone:
the YAML key keeps refusing at construction).  No GPU."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CFG = os.path.join(HERE, "configs", "finetune_dsec_synthetic.yaml")
EINVAL = -22
NEW_ENTRIES = ("oess_dropout_f32", "oess_aspp_pool_bwd_f32o")


def _net(**kw):
    from openess_amd.models.deeplabv3 import deeplabv3_resnet50
    return deeplabv3_resnet50(num_classes=11, text_embeddings_path=None, output_stride=16, pretrained_backbone='', **kw)


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_new_entries_are_declared_exported_and_bound():
    from openess_amd import _lib
    header = open(os.path.join(ROOT, "include", "oess.h")).read()
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(lib, name).restype is ctypes.c_int
    assert lib.oess_abi_version() == 13 and "#define OESS_ABI_VERSION 13" in header
    # the fp32-output form takes the arguments of the bf16-output one
    assert len(_lib.SIGNATURES["oess_aspp_pool_bwd_f32o"][1]) == len(_lib.SIGNATURES["oess_aspp_pool_bwd_f32"][1])


def _views():
    from openess_amd import _lib
    buf = (ctypes.c_float * 4096)()
    addr = ctypes.addressof(buf)
    addr += (-addr) % 16
    return buf, addr, _lib.F32View(addr, 1024, 128, 16, 1), _lib.F32View(None, 1024, 128, 16, 1)


def test_dropout_f32_entry_refuses_on_the_host():
    from openess_amd import _lib
    lib = _lib.load()
    buf, addr, ok, null = _views()
    r = ctypes.byref
    drop = lib.oess_dropout_f32

    def call(x=r(ok), y=r(ok), B=1, H=8, W=8, C=16, p=0.1):
        return drop(x, y, B, H, W, C, p, 1, 2, None)

    assert call(x=None) == EINVAL and call(x=r(null)) == EINVAL and call(y=None) == EINVAL and call(y=r(null)) == EINVAL
    assert call(C=12) == EINVAL and call(C=4) == EINVAL and call(C=17) == EINVAL             # C % 8
    assert call(p=1.0) == EINVAL and call(p=-0.1) == EINVAL and call(p=1.5) == EINVAL and call(p=float('nan')) == EINVAL
    for B, H, W, C in ((0, 8, 8, 16), (1, 0, 8, 16), (1, 8, 0, 16), (1, 8, 8, 0), (-1, 8, 8, 16)):
        assert call(B=B, H=H, W=W, C=C) == EINVAL


def test_aspp_pool_bwd_f32o_entry_refuses_on_the_host():
    from openess_amd import _lib
    lib = _lib.load()
    buf, a, _, _ = _views()
    bwd = lib.oess_aspp_pool_bwd_f32o

    def call(B=3, Cin=64, Cout=256, **null):
        names = ('grad_z', 'pooled', 'w', 'gamma', 'y_pre', 'stat', 'z', 'dy', 'gw', 'gg', 'gb', 'gp')
        p = {n: (None if null.get(n) else a) for n in names}
        return bwd(p['grad_z'], p['pooled'], 1.0, p['w'], p['gamma'], p['y_pre'], p['stat'], p['z'], B, Cin, Cout, p['dy'], p['gw'],
                   p['gg'], p['gb'], p['gp'], None)

    for n in ('grad_z', 'pooled', 'w', 'gamma', 'y_pre', 'stat', 'z', 'dy', 'gw', 'gg', 'gb'):
        assert call(**{n: True}) == EINVAL, n                                    # grad_pooled alone may be null (frozen producer)
    assert call(B=1) == EINVAL and call(B=17) == EINVAL and call(B=0) == EINVAL
    assert call(Cin=0) == EINVAL and call(Cout=0) == EINVAL and call(Cin=-4) == EINVAL
    # the bf16-output entry refuses the same
    assert lib.oess_aspp_pool_bwd_f32(None, None, 1.0, None, None, None, None, None, 8, 2048, 256, None, None, None, None, None, None) == EINVAL


# ------------------------------------------------------------------------------------------------------------ hip.py
def test_hip_functions_refuse_before_any_launch(monkeypatch):
    from openess_amd import hip

    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(hip._lib, "load", boom)
    x = torch.zeros(3, 64, 4, 6)
    conv, bn = torch.nn.Conv2d(64, 256, 1, bias=False), torch.nn.BatchNorm2d(256)
    assert hip.dropout_f32(x, 0.1, training=False) is x and hip.dropout_f32(x, 0.0) is x
    with pytest.raises(ValueError, match="fp32"):
        hip.dropout_f32(x.bfloat16(), 0.1)
    with pytest.raises(ValueError, match="C % 8"):
        hip.dropout_f32(x[:, :12], 0.1)
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        hip.dropout_f32(x, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.dropout_f32(x, 0.1)
    with pytest.raises(ValueError, match="fp32"):
        hip.aspp_pool_branch_f32(x.bfloat16(), conv, bn)
    with pytest.raises(ValueError, match="2 <= B <= 16"):
        hip.aspp_pool_branch_f32(x[:1], conv, bn)
    with pytest.raises(ValueError, match="2 <= B <= 16"):
        hip.aspp_pool_branch_f32(torch.zeros(17, 64, 2, 2), conv, bn)
    with pytest.raises(ValueError, match="Cin % 4"):
        hip.aspp_pool_branch_f32(x[:, :62], torch.nn.Conv2d(62, 256, 1, bias=False), bn)
    with pytest.raises(NotImplementedError, match="eval-mode"):
        hip.aspp_pool_branch_f32(x, conv, torch.nn.BatchNorm2d(256).eval())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.aspp_pool_branch_f32(x, conv, bn)
    assert int(bn.num_batches_tracked) == 0


# ------------------------------------------------------------------------------------------------------------ the model
def test_forward_fp32_train_refusals_and_the_inference_entry_points_unchanged(monkeypatch):
    from openess_amd import hip
    net = _net().train()
    for name in ('forward_fp32_train', 'check_fp32_train'):
        assert callable(getattr(net, name))
    for mod in (net.backbone, net.classifier, net.classifier.ASPP, net.classifier.ASPP.convs[0], net.classifier.ASPP.convs[4],
                net.backbone.layer1[0]):
        assert callable(mod.forward_fp32_autograd)
    net.check_fp32_train()

    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(hip._lib, "load", boom)
    img = torch.zeros(2, 3, 32, 32)
    with pytest.raises(ValueError, match="float32"):
        net.forward_fp32_train(img.bfloat16())
    with pytest.raises(ValueError, match="float32"):
        net.forward_fp32_train(img[0])
    net.backbone.layer3[2].bn2.eval()                # one BatchNorm in eval mode is named
    with pytest.raises(NotImplementedError, match=r"backbone\.layer3\.2\.bn2.*eval mode"):
        net.check_fp32_train()
    with pytest.raises(NotImplementedError, match=r"backbone\.layer3\.2\.bn2"):
        net.forward_fp32_train(img)
    net.train()
    net.classifier.ASPP.convs[4][2].momentum = None
    with pytest.raises(NotImplementedError, match=r"classifier\.ASPP\.convs\.4\.2.*momentum"):
        net.forward_fp32_train(img)
    net.classifier.ASPP.convs[4][2].momentum = 0.1
    net.classifier.classifier[1] = torch.nn.BatchNorm2d(512, track_running_stats=False)
    with pytest.raises(NotImplementedError, match=r"classifier\.classifier\.1.*running statistics"):
        net.forward_fp32_train(img)
    net.classifier.classifier[1] = torch.nn.BatchNorm2d(512)
    net.eval()
    with pytest.raises(NotImplementedError, match="eval mode"):
        net.forward_fp32_train(img)
    # the train-mode network on the CPU: the first kernel wrapper refuses the tensor
    net.train()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.forward_fp32_train(img)
    # K16's entry points on the same model: as before (they pack an operand before the first kernel wrapper refuses)
    monkeypatch.undo()
    with pytest.raises(NotImplementedError, match="train mode"):
        net.check_fp32()
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        net.forward_fp32(img)
    net.eval()
    net.check_fp32()
    with pytest.raises(ValueError, match="float32"):
        net.forward_fp32(img.bfloat16())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.forward_fp32(img)
    assert sorted(k for k in net.state_dict() if 'ASPP.project' in k)[0] == 'classifier.ASPP.project.0.weight'


# ------------------------------------------------------------------------------------------------------------ the trainers
def _settings(tmp_path, **clip):
    from openess_amd.config.settings import Settings
    cfg = yaml.load(open(CFG), yaml.Loader)
    cfg['clip'].update(clip)
    path = tmp_path / "settings.yaml"
    path.write_text(yaml.dump(cfg))
    return Settings(str(path), generate_log=False)


class _StubModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(()))
        self.calls = []

    def forward(self, x):
        self.calls.append(('bf16', x))
        return x * self.w, None

    def forward_fp32_train(self, x, want_feats=False):
        self.calls.append(('fp32', x))
        return x * self.w, None


def _stub_trainer(tmp_path, option, train_precision='bf16'):
    from openess_amd.training.finetune_trainer import OpenESSFineTuneModel
    s = _settings(tmp_path, config_option=option)
    tr = object.__new__(OpenESSFineTuneModel)
    tr.settings, tr.device, tr.train_precision, tr.eval_precision = s, torch.device('cpu'), train_precision, 'bf16'
    losses = []
    tr.task_loss = lambda logits, gt: (losses.append((logits, gt)), logits.sum())[1]
    return tr, losses


def test_task_train_step_precision_argument_frame2recon(tmp_path):
    tr, losses = _stub_trainer(tmp_path, 'frame2recon')
    stub = _StubModel()
    tr.model_recon, tr.models_dict = stub, {'model_recon': stub}
    img, gt = torch.full((2, 3), 2.0), torch.zeros(2, 3, dtype=torch.long)
    batch = (None, gt, img)
    total, out, _ = tr.task_train_step(batch, precision='fp32')
    assert [c[0] for c in stub.calls] == ['fp32'] and stub.calls[0][1] is img and len(losses) == 1 and losses[0][1] is gt
    assert set(out) == {'semseg_recon_loss'} and float(out['semseg_recon_loss']) == float(total.detach()) == 12.0
    assert total.requires_grad and stub.training
    tr.task_train_step(batch)                                    # None: the trainer's train_precision
    tr.task_train_step(batch, precision='bf16')
    assert [c[0] for c in stub.calls] == ['fp32', 'bf16', 'bf16'] and len(losses) == 3
    for bad in ('half', 'fp16', 'FP32', 32):
        with pytest.raises(ValueError, match="precision"):
            tr.task_train_step(batch, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            tr.train_step(batch, precision=bad)
    assert len(stub.calls) == 3


def test_train_step_passes_precision_through(tmp_path):
    tr, _ = _stub_trainer(tmp_path, 'frame2recon')
    stub = _StubModel()
    tr.model_recon, tr.models_dict = stub, {'model_recon': stub}
    tr.optimizers_dict = {'optimizer_recon': torch.optim.SGD(stub.parameters(), lr=0.5)}
    reducer_calls = []
    tr.grad_reducer = type('R', (), {'prepare': lambda self: reducer_calls.append('prepare'),
                                     '__call__': lambda self: reducer_calls.append('reduce')})()
    batch = (None, torch.zeros(2, 3, dtype=torch.long), torch.full((2, 3), 2.0))
    losses, _, total = tr.train_step(batch, precision='fp32')
    assert [c[0] for c in stub.calls] == ['fp32'] and reducer_calls == ['prepare', 'reduce']
    assert set(losses) == {'semseg_recon_loss'} and float(total) == 12.0 and float(stub.w.detach()) == 1.0 - 0.5 * 12.0


def test_event_trainer_built_in_bf16_refuses_an_fp32_step(tmp_path):
    tr, losses = _stub_trainer(tmp_path, 'frame2voxel')
    tr.models_dict = {}
    batch = (torch.zeros(1), torch.zeros(1, dtype=torch.long), None)
    with pytest.raises(RuntimeError, match="train_precision: fp32"):
        tr.task_train_step(batch, precision='fp32')
    with pytest.raises(RuntimeError, match="train_precision: fp32"):
        tr.train_step(batch, precision='fp32')
    assert not losses


def test_yaml_key_still_refuses_frame2recon_at_construction(tmp_path, monkeypatch):
    from openess_amd.training import _supervised as sup

    def boom(*a, **k):
        raise AssertionError("a model was built before the refusal")
    monkeypatch.setattr(sup, 'deeplabv3_resnet50', boom)
    monkeypatch.setattr(sup.BaseTrainer, '__init__', boom)
    from openess_amd.training.finetune_trainer import OpenESSFineTuneModel
    with pytest.raises(NotImplementedError, match="BatchNorm.*strided and dilated"):
        OpenESSFineTuneModel(settings=_settings(tmp_path, train_precision='fp32', config_option='frame2recon'))
    with pytest.raises(NotImplementedError, match="eval_precision: fp32 is not wired for frame2recon"):
        OpenESSFineTuneModel(settings=_settings(tmp_path, eval_precision='fp32', config_option='frame2recon'))
