"""Host-side checks of the fp32 MaskCLIP tower (K25): every refusal of the three wrappers (a ValueError naming the operand, before
the device check and before any launch), every OESS_EINVAL of the three raw entries by calls that cannot launch, the
`online_teacher_precision` settings key, what the stage-1 trainer hands PretrainStep as online teacher, and the shipped YAML.
No GPU."""
import ctypes
import os

import pytest
import torch
import yaml

EINVAL = -22
CFG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")
CFG = os.path.join(CFG_DIR, "pretrain_dsec_synthetic.yaml")


def _aligned():
    buf = ctypes.create_string_buffer(1 << 16)
    addr = ctypes.addressof(buf)
    return buf, addr + (-addr) % 16


# --------------------------------------------------------------------------------------------- raw entries, no launch
def test_layernorm_f32_entry_validates_arguments_before_any_launch():
    from openess_amd import _lib
    ln = _lib.load().oess_layernorm_f32
    buf, a = _aligned()

    def call(x=a, xs=768, rows=4, C=768, gamma=a, beta=a, eps=1e-6, y=a, ys=768):
        return ln(x, xs, rows, C, gamma, beta, eps, y, ys, None)

    for bad in (dict(C=0, xs=8, ys=8), dict(C=-4), dict(C=2049, xs=2052, ys=2052), dict(eps=0.0), dict(eps=-1e-6),
                dict(eps=float("nan")), dict(xs=767), dict(ys=767), dict(xs=0), dict(rows=0), dict(rows=-1), dict(x=None),
                dict(y=None), dict(gamma=None), dict(beta=None), dict(x=a + 2), dict(y=a + 1), dict(gamma=a + 3), dict(beta=a + 2),
                dict(xs=1 << 31), dict(ys=1 << 31), dict(rows=1 << 34)):
        assert call(**bad) == EINVAL, bad
    del buf


def test_attention_f32_entry_validates_arguments_before_any_launch():
    from openess_amd import _lib
    att = _lib.load().oess_attention_d64_f32
    buf, a = _aligned()

    def call(qkv=a, qs=3 * 128, B=2, L=9, heads=2, scale=0.125, out=a, os_=128):
        return att(qkv, qs, B, L, heads, scale, out, os_, None)

    for bad in (dict(L=0), dict(L=-1), dict(heads=0), dict(heads=-1), dict(B=0), dict(B=-2), dict(qs=3 * 128 - 4), dict(qs=3 * 128 + 2),
                dict(qs=3 * 128 + 1), dict(os_=124), dict(os_=130), dict(qkv=a + 8), dict(qkv=a + 4), dict(out=a + 8), dict(out=a + 4),
                dict(qkv=None), dict(out=None), dict(scale=0.0), dict(scale=-0.125), dict(scale=float("inf")), dict(scale=float("nan")),
                dict(B=1 << 16, L=1 << 15), dict(qs=1 << 31), dict(os_=1 << 31), dict(heads=(1 << 20) + 1, qs=1 << 30, os_=1 << 30),
                dict(B=1 << 11, L=1 << 19, heads=1 << 10, qs=3 << 16, os_=1 << 16)):
        assert call(**bad) == EINVAL, bad
    del buf


def test_linear_tokens_f32_entry_validates_arguments_before_any_launch():
    from openess_amd import _lib
    lin = _lib.load().oess_linear_tokens_f32
    buf, a = _aligned()

    def call(x=a, xs=24, rows=5, Cin=24, w=a, bias=a, Cout=11, act=0, res=a, rs=11, out=a, os_=11):
        return lin(x, xs, rows, Cin, w, bias, Cout, act, res, rs, out, os_, None)

    for bad in (dict(x=None), dict(w=None), dict(out=None), dict(rows=0), dict(rows=-1), dict(rows=1 << 31), dict(Cin=0), dict(Cin=-1),
                dict(Cin=(1 << 20) + 1, xs=1 << 21), dict(Cout=0), dict(Cout=-3), dict(act=-1), dict(act=2), dict(act=3), dict(xs=23),
                dict(os_=10), dict(rs=10), dict(w=a + 4), dict(w=a + 8), dict(bias=a + 2), dict(res=a + 1), dict(xs=1 << 31),
                dict(os_=1 << 31), dict(rs=1 << 31)):
        assert call(**bad) == EINVAL, bad
    del buf


def test_the_convolution_entries_still_refuse_the_gelu_code():
    """GELU is an epilogue of oess_linear_tokens_f32 alone: its internal code is not an `act` of the convolution entries"""
    from openess_amd import _lib
    lib = _lib.load()
    buf, a = _aligned()
    v = _lib.F32View(a, 0, 0, 16, 1)
    ref = ctypes.byref(v)
    assert lib.oess_conv2d_fwd_f32(ref, None, 1, 1, 4, 16, 0, a, None, 8, 1, 1, 1, 0, 3, None, ref, None) == EINVAL
    assert lib.oess_conv2d_dilated_fwd_f32(ref, None, 1, 1, 4, 16, 0, a, None, 8, 1, 1, 1, 0, 1, 3, None, ref, None) == EINVAL
    del buf


# --------------------------------------------------------------------------------------------- wrappers
def test_layer_norm_tokens_f32_refusals():
    from openess_amd import hip
    rows, C = 5, 64
    x, g, b = torch.zeros(rows, C), torch.ones(C), torch.zeros(C)
    wide = torch.empty(rows, 2 * C)
    for bad in (x.bfloat16(), x.double(), x[0], x[None], wide[:, ::2], torch.zeros(C, rows).T, torch.zeros(0, C), torch.zeros(rows, 0),
                None, torch.zeros(3, 2052)):
        with pytest.raises(ValueError, match="layer_norm_tokens_f32: x "):
            hip.layer_norm_tokens_f32(bad, g, b)
    for p in (g.double(), g.bfloat16(), torch.ones(2 * C)[::2], torch.ones(C + 1), torch.ones(C - 1), torch.ones(1, C), g.to("meta"), None):
        with pytest.raises(ValueError, match="gamma must be contiguous fp32"):
            hip.layer_norm_tokens_f32(x, p, b)
        with pytest.raises(ValueError, match="beta must be contiguous fp32"):
            hip.layer_norm_tokens_f32(x, g, p)
    for eps in (0.0, -1e-6, float("nan")):
        with pytest.raises(ValueError, match="eps"):
            hip.layer_norm_tokens_f32(x, g, b, eps=eps)
    for o in (x.bfloat16(), x.to("meta"), torch.empty(rows + 1, C), torch.empty(rows, C - 4), x[0], wide[:, ::2], torch.empty(C, rows).T):
        with pytest.raises(ValueError, match="layer_norm_tokens_f32: out "):
            hip.layer_norm_tokens_f32(x, g, b, out=o)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.layer_norm_tokens_f32(x, g, b, out=wide[:, :C])


def test_attention_d64_f32_refusals():
    from openess_amd import hip
    B, L, heads = 1, 5, 1
    C = 64
    qkv = torch.zeros(B * L, 3 * C)
    for bad in (qkv.bfloat16(), qkv[:, :-4], qkv[:-1], qkv[0], torch.zeros(B * L, 6 * C)[:, ::2], None):
        with pytest.raises(ValueError, match="attention_d64_f32: qkv "):
            hip.attention_d64_f32(bad, B, L, heads)
    for unaligned in (torch.zeros(B * L, 3 * C + 2)[:, :3 * C], torch.zeros(B * L * 3 * C + 1)[1:].view(B * L, 3 * C)):
        with pytest.raises(ValueError, match="qkv rows must be 16-byte aligned"):
            hip.attention_d64_f32(unaligned, B, L, heads)
    for kw in (dict(B=0), dict(L=0), dict(heads=0), dict(B=-1), dict(L=2.5)):
        with pytest.raises(ValueError, match="positive integers"):
            hip.attention_d64_f32(qkv, **{**dict(B=B, L=L, heads=heads), **kw})
    for o in (torch.empty(B * L, C, dtype=torch.bfloat16), torch.empty(B * L, C, device="meta"), torch.empty(B * L + 1, C),
              torch.empty(B * L, C + 4), torch.empty(B * L, 2 * C)[:, ::2], torch.empty(C, B * L).T):
        with pytest.raises(ValueError, match="attention_d64_f32: out "):
            hip.attention_d64_f32(qkv, B, L, heads, out=o)
    for o in (torch.empty(B * L, C + 2)[:, :C], torch.empty(B * L * C + 1)[1:].view(B * L, C)):
        with pytest.raises(ValueError, match="out rows must be 16-byte aligned"):
            hip.attention_d64_f32(qkv, B, L, heads, out=o)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.attention_d64_f32(qkv, B, L, heads, out=torch.empty(B * L, C + 64)[:, :C])


def test_linear_tokens_f32_refusals():
    from openess_amd import hip
    rows, Cin, Cout = 5, 24, 11
    x = torch.zeros(rows, Cin)
    packed = hip.pack_conv_weight_f32(torch.zeros(Cout, Cin, 1, 1))
    assert tuple(packed.shape) == (32, 32)
    bias, res = torch.zeros(Cout), torch.zeros(rows, Cout)
    for bad in (x.bfloat16(), x[0], torch.zeros(rows, 2 * Cin)[:, ::2], torch.zeros(Cin, rows).T, torch.zeros(0, Cin), None):
        with pytest.raises(ValueError, match="linear_tokens_f32: x "):
            hip.linear_tokens_f32(bad, packed, bias, Cout)
    for p in (packed.double(), packed[:16], packed[:, ::2], packed.to("meta"), None):
        with pytest.raises(ValueError, match="linear_tokens_f32: packed "):
            hip.linear_tokens_f32(x, p, bias, Cout)
    for co in (0, -1, 11.0, 64):                                   # 64: the operand was packed for fewer output channels
        with pytest.raises(ValueError, match="linear_tokens_f32: (Cout|packed) "):
            hip.linear_tokens_f32(x, packed, None, co)
    for bb in (bias.double(), torch.zeros(Cout + 1), torch.zeros(2 * Cout)[::2], bias.to("meta")):
        with pytest.raises(ValueError, match="bias must be contiguous fp32"):
            hip.linear_tokens_f32(x, packed, bb, Cout)
    for act in ('relu', 'sigmoid', 1, 'GELU'):
        with pytest.raises(ValueError, match="act must be one of"):
            hip.linear_tokens_f32(x, packed, bias, Cout, act=act)
    for r in (res.bfloat16(), torch.zeros(rows, Cout + 1), torch.zeros(rows + 1, Cout), torch.zeros(Cout, rows).T, res.to("meta")):
        with pytest.raises(ValueError, match="linear_tokens_f32: residual "):
            hip.linear_tokens_f32(x, packed, bias, Cout, residual=r)
    for o in (res.double(), torch.empty(rows, Cout - 1), torch.empty(rows, 2 * Cout)[:, ::2], res.to("meta"), res[0]):
        with pytest.raises(ValueError, match="linear_tokens_f32: out "):
            hip.linear_tokens_f32(x, packed, bias, Cout, out=o)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.linear_tokens_f32(x, packed, bias, Cout, act='gelu', residual=res, out=torch.empty(rows, Cout + 5)[:, :Cout])


# --------------------------------------------------------------------------------------------- settings key, trainer, YAML
def _settings(tmp_path, **clip):
    from openess_amd.config.settings import Settings
    cfg = yaml.load(open(CFG), yaml.Loader)
    cfg['clip'].update(clip)
    path = tmp_path / "settings.yaml"
    path.write_text(yaml.dump(cfg))
    return Settings(str(path), generate_log=False)


def test_online_teacher_precision_key(tmp_path):
    assert _settings(tmp_path).online_teacher_precision == 'bf16'
    assert _settings(tmp_path, online_teacher_precision='bf16').online_teacher_precision == 'bf16'
    assert _settings(tmp_path, online_teacher_precision='fp32').online_teacher_precision == 'fp32'
    for bad in ('fp16', 'FP32', 32, True, 'float32'):
        with pytest.raises(ValueError, match="online_teacher_precision"):
            _settings(tmp_path, online_teacher_precision=bad)


def test_build_models_hands_the_step_the_fp32_callable(tmp_path, monkeypatch):
    from openess_amd.models import maskclip_model
    from openess_amd.training import pretrain_trainer as pt
    seen = []

    class Tower:
        def __init__(self, **kw):
            self.kw = kw

        def to(self, device):
            return self

        def eval(self):
            return self

        def forward_fp32(self, img):
            return "fp32"

        def __call__(self, img):
            return "bf16"

    class Step:
        def __init__(self, **kw):
            seen.append(kw)
            self.models_dict = {}

    monkeypatch.setattr(maskclip_model, 'maskClipFeatureExtractor', Tower)
    monkeypatch.setattr(pt, 'PretrainStep', Step)
    for precision, want in (('fp32', 'fp32'), ('bf16', 'bf16'), (None, 'bf16')):
        clip = {'pl_sources': 'online_maskclip'}
        if precision is not None:
            clip['online_teacher_precision'] = precision
        tr = object.__new__(pt.OpenESSPretrainModel)
        tr.settings, tr.device, tr.train_precision = _settings(tmp_path, **clip), 'cpu', 'bf16'
        tr.buildModels()
        teacher = seen[-1]['online_teacher']
        assert teacher(None) == want and seen[-1]['precision'] == 'bf16'
        assert isinstance(teacher, Tower) == (want == 'bf16')                 # the default is the module itself
        assert (getattr(teacher, '__self__', None).__class__ is Tower) == (want == 'fp32')
    tr = object.__new__(pt.OpenESSPretrainModel)
    tr.settings, tr.device, tr.train_precision = _settings(tmp_path, online_teacher_precision='fp32'), 'cpu', 'bf16'
    tr.buildModels()
    assert seen[-1]['online_teacher'] is None                                 # the key alone builds no tower
    s = _settings(tmp_path, pl_sources='online_maskclip')
    s.online_teacher_precision = 'half'
    tr = object.__new__(pt.OpenESSPretrainModel)
    tr.settings, tr.device, tr.train_precision = s, 'cpu', 'bf16'
    with pytest.raises(ValueError, match="online_teacher_precision"):
        tr.buildModels()


def test_fp32_training_with_an_online_teacher_stays_refused(tmp_path):
    """the fp32 tower is a teacher for the bf16 step: train_precision fp32 with an online teacher is refused as before"""
    from openess_amd.training.pretrain_step import PretrainStep
    from openess_amd.training.pretrain_trainer import OpenESSPretrainModel
    with pytest.raises(NotImplementedError):
        PretrainStep(online_teacher=lambda x: x, precision='fp32', device='cpu')
    s = _settings(tmp_path, train_precision='fp32', pl_sources='online_maskclip', online_teacher_precision='fp32')
    with pytest.raises(NotImplementedError):
        OpenESSPretrainModel(settings=s)


def test_shipped_yaml_differs_from_the_bf16_one_by_the_two_keys_alone():
    new = yaml.load(open(os.path.join(CFG_DIR, "pretrain_dsec_synthetic_online_maskclip_fp32.yaml")), yaml.Loader)
    bf16 = yaml.load(open(CFG), yaml.Loader)
    assert new['clip'].pop('online_teacher_precision') == 'fp32'
    assert new['clip']['pl_sources'] == 'online_maskclip' and bf16['clip']['pl_sources'] != 'online_maskclip'
    new['clip']['pl_sources'] = bf16['clip']['pl_sources']
    assert new == bf16


def test_tower_has_forward_fp32_on_every_module_and_the_same_state_dict():
    from openess_amd.models import maskclip_model as mm
    for cls in (mm.TransformerEncoderLayer, mm.VisionTransformer, mm.MaskClipHead, mm.maskClipFeatureExtractor):
        assert callable(getattr(cls, 'forward_fp32'))
    assert callable(mm.TransformerEncoderLayer.forward_value_path_fp32)
    m = mm.maskClipFeatureExtractor(text_categories=5, img_size=(32, 32))
    assert not any('pw32' in k or 'fp32' in k for k in m.state_dict())
