"""Host-side checks of MaskCLIP's refinement, no GPU: the float64 restatement of tests/maskclip_refine_reference.py
against the reference's own float64 output in tests/golden/maskclip_refine.npz (explicit and factored form, and the two mutations
the fixture must tell apart), the fixture's margins, the settings keys and their refusals, what the stage-1 trainer hands
PretrainStep, the shipped YAML, and every refusal of the wrapper (a ValueError naming the operand, before the device check) and of
the raw entry (OESS_EINVAL by calls that cannot launch)."""
import ctypes
import functools
import os

import pytest
import torch
import yaml

from tests import maskclip_refine_cases as rc
from tests import maskclip_refine_reference as rr

EINVAL, ENOMEM = -22, -12
CFG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")
CFG = os.path.join(CFG_DIR, "pretrain_dsec_synthetic.yaml")
SMOOTHED = [n for n, c in rc.CASES.items() if c[5] > 0 and c[0] > 1 and c[1] * c[2] > 1]


# --------------------------------------------------------------------------------------------- fixture and restatement
def test_fixture_is_small_and_complete():
    assert os.path.getsize(rc.GOLDEN) < (1 << 20)
    g = rc.golden()
    for name, (K, H, W, C, pd, ks, k_bf16) in rc.CASES.items():
        c = rc.case(name)
        assert tuple(c["output"].shape) == tuple(c["ref64"].shape) == tuple(c["ref32"].shape) == (rc.N, K, H, W)
        assert tuple(c["k"].shape) == (rc.N, H * W, C) and (c["pd"], c["ks"]) == (pd, ks)
        assert c["output"].dtype == c["k"].dtype == c["ref32"].dtype == torch.float32 and c["ref64"].dtype == torch.float64
        assert torch.equal(c["k"].bfloat16().float(), c["k"]) == k_bf16
    assert tuple(g["layer/k64"].shape) == (rc.LAYER["B"], rc.LAYER["tokens"], rc.LAYER["C"]) and g["layer/k64"].dtype.name == "float64"


@pytest.mark.parametrize("name", list(rc.CASES))
def test_fixture_margins_hold(name):
    """no threshold decision can differ between float64 and float32: every pixel and every class is compared"""
    c = rc.case(name)
    m = rc.margins(c["output"], c["pd"], c["ks"])
    assert rc.margins_hold(name, m), m
    if c["pd"] > 0:
        assert m["pd_dist"] >= rc.PD_MARGIN
    if c["ks"] > 0:
        assert m["neither"] == 0 and m["ks_dist"] >= rc.KS_MARGIN
    # and the reference's own two precisions agree to rounding: no decision differed when the file was written
    assert rc.rel_max(c["ref32"], c["ref64"]) < 1e-5


@pytest.mark.parametrize("name", list(rc.CASES))
@pytest.mark.parametrize("form", ["explicit", "factored"])
def test_restatement_equals_the_reference_float64(name, form):
    c = rc.case(name)
    out = rr.refine(c["output"], c["k"], c["pd"], c["ks"], form=form)
    assert rc.rel_max(out, c["ref64"]) <= 1e-12
    if c["ks"] <= 0:                                         # smoothing off: the logits with the -100 rows
        assert torch.equal(out, c["ref64"]) and bool((out == -100).any())


@pytest.mark.parametrize("name", SMOOTHED)
def test_fixture_tells_the_normalisation_axis(name):
    """F.normalize's default dim 1 of a 3-D tensor is the token axis; normalising over the channels misses by orders of magnitude"""
    c = rc.case(name)
    assert rc.rel_max(rr.refine(c["output"], c["k"], c["pd"], c["ks"], normalize_dim=2), c["ref64"]) > 1e-2


def _layer():
    g = rc.golden()
    ops = {k: torch.from_numpy(g["layer/" + k]) for k in ("x", "ln1_w", "ln1_b", "in_w", "in_b", "out_w", "out_b")}
    return ops, torch.from_numpy(g["layer/k64"])


def test_last_layer_keys_restated():
    ops, k64 = _layer()
    for key, v in rc.layer_operands().items():
        assert torch.equal(v, ops[key]), key
    assert rc.rel_max(rr.last_layer_k(**ops), k64) <= 1e-12
    assert rc.rel_max(rr.last_layer_k(**ops, residual=True), k64) > 1e-2         # k has no residual: only v gets `+= x`


def test_exact_cases_are_exact_in_float64():
    out, k = rc.identity_case()
    assert torch.equal(rr.refine(out, k, 0.5, 1.0), rr.refine(out, k, 0.5, 1e-30))
    out, k, expect = rc.grouped_case()
    assert torch.equal(rr.refine(out, k, 0.5, 2.0).float(), expect)
    assert bool((k.abs().sum(dim=1) == 0).any()) and set(expect.unique().tolist()) <= {i / 16 for i in range(17)}


# --------------------------------------------------------------------------------------------- settings, trainer, YAML
def _settings(tmp_path, **clip):
    from openess_amd.config.settings import Settings
    cfg = yaml.load(open(CFG), yaml.Loader)
    cfg['clip'].update(clip)
    path = tmp_path / "settings.yaml"
    path.write_text(yaml.dump(cfg))
    return Settings(str(path), generate_log=False)


def test_settings_keys(tmp_path):
    s = _settings(tmp_path)
    assert (s.online_maskclip_refine, s.online_maskclip_pd_thresh, s.online_maskclip_ks_thresh) == (False, 0.5, 1.0)
    s = _settings(tmp_path, pl_sources='online_maskclip', online_maskclip_refine=True, online_maskclip_pd_thresh=0.3, online_maskclip_ks_thresh=0)
    assert (s.online_maskclip_refine, s.online_maskclip_pd_thresh, s.online_maskclip_ks_thresh) == (True, 0.3, 0)
    for key in ('online_maskclip_pd_thresh', 'online_maskclip_ks_thresh'):
        for bad in (-0.1, -1, float('nan'), float('inf'), '0.5', True, None):
            with pytest.raises(ValueError, match=key):
                _settings(tmp_path, **{key: bad})
    for bad in ('yes', 1, None, 0.5):
        with pytest.raises(ValueError, match="online_maskclip_refine"):
            _settings(tmp_path, online_maskclip_refine=bad)


def test_refine_without_the_online_teacher_is_refused_at_construction(tmp_path):
    from openess_amd.training import base_trainer_ov as bt
    from openess_amd.training.pretrain_trainer import OpenESSPretrainModel
    s = _settings(tmp_path, online_maskclip_refine=True)
    assert s.pl_sources != 'online_maskclip'
    with pytest.raises(ValueError, match="online_maskclip_refine: True needs pl_sources: online_maskclip"):
        OpenESSPretrainModel(settings=s)
    assert bt.online_maskclip_refine(_settings(tmp_path)) is None
    assert bt.online_maskclip_refine(_settings(tmp_path, pl_sources='online_maskclip')) is None
    ok = _settings(tmp_path, pl_sources='online_maskclip', online_maskclip_refine=True, online_maskclip_pd_thresh=0.25)
    assert bt.online_maskclip_refine(ok) == {'pd_thresh': 0.25, 'ks_thresh': 1.0}


def test_build_models_hands_the_step_the_refined_forward(tmp_path, monkeypatch):
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

        def forward_fp32(self, img, refine=False):
            return ("fp32", refine)

        def __call__(self, img, refine=False):
            return ("bf16", refine)

    class Step:
        def __init__(self, **kw):
            seen.append(kw)
            self.models_dict = {}

    monkeypatch.setattr(maskclip_model, 'maskClipFeatureExtractor', Tower)
    monkeypatch.setattr(pt, 'PretrainStep', Step)

    def build(**clip):
        tr = object.__new__(pt.OpenESSPretrainModel)
        tr.settings, tr.device, tr.train_precision = _settings(tmp_path, **clip), 'cpu', 'bf16'
        tr.buildModels()
        return seen[-1]['online_teacher']

    for precision in ('bf16', 'fp32'):
        teacher = build(pl_sources='online_maskclip', online_teacher_precision=precision, online_maskclip_refine=True,
                        online_maskclip_pd_thresh=0.4, online_maskclip_ks_thresh=0.9)
        assert teacher(None) == (precision, True)
        assert isinstance(teacher, functools.partial) and teacher.keywords == {'refine': True}
        tower = teacher.func if precision == 'bf16' else teacher.func.__self__
        assert isinstance(tower, Tower) and tower.kw['pd_thresh'] == 0.4 and tower.kw['ks_thresh'] == 0.9
        teacher = build(pl_sources='online_maskclip', online_teacher_precision=precision)
        assert teacher(None) == (precision, False) and not isinstance(teacher, functools.partial)
        assert 'pd_thresh' not in (teacher if precision == 'bf16' else teacher.__self__).kw


def test_shipped_yaml_differs_from_the_plain_one_by_its_keys_alone():
    new = yaml.load(open(os.path.join(CFG_DIR, "pretrain_dsec_synthetic_online_maskclip_refine.yaml")), yaml.Loader)
    plain = yaml.load(open(CFG), yaml.Loader)
    assert new['clip'].pop('online_maskclip_refine') is True
    assert new['clip'].pop('online_maskclip_pd_thresh') == 0.5 and new['clip'].pop('online_maskclip_ks_thresh') == 1.0
    assert new['clip']['pl_sources'] == 'online_maskclip' and plain['clip']['pl_sources'] != 'online_maskclip'
    new['clip']['pl_sources'] = plain['clip']['pl_sources']
    assert new == plain


def test_model_surface_and_state_dict():
    from openess_amd.models import maskclip_model as mm
    assert callable(mm.TransformerEncoderLayer.forward_key_path) and callable(mm.TransformerEncoderLayer.forward_key_path_fp32)
    assert callable(mm.MaskClipHead.refine_output)
    plain = mm.maskClipFeatureExtractor(text_categories=5, img_size=(32, 32))
    m = mm.maskClipFeatureExtractor(text_categories=5, img_size=(32, 32), ks_thresh=0.9, pd_thresh=0.25)
    assert (plain.decoder.ks_thresh, plain.decoder.pd_thresh) == (1, 0.5) and (m.decoder.ks_thresh, m.decoder.pd_thresh) == (0.9, 0.25)
    assert list(m.state_dict().keys()) == list(plain.state_dict().keys())
    assert not any('thresh' in k or 'k_out' in k for k in m.state_dict())
    for bad in (dict(ks_thresh=-1), dict(pd_thresh=-0.5), dict(pd_thresh=float('nan'))):
        with pytest.raises(ValueError, match="thresh"):
            mm.MaskClipHead(**bad)


# --------------------------------------------------------------------------------------------- wrapper refusals
def test_maskclip_refine_refusals():
    from openess_amd import hip
    B, K, H, W, C = 2, 5, 3, 4, 64
    x, k = torch.zeros(B, K, H, W), torch.zeros(B, H * W, C)
    for bad in (x.double(), x.bfloat16(), x[0], x[None], None, torch.zeros(B, 33, H, W), torch.zeros(B, 0, H, W), torch.zeros(0, K, H, W),
                torch.zeros(B, K, 65, 64), torch.zeros(B, K, 0, W), torch.zeros(B, K, 1, 4097)):
        with pytest.raises(ValueError, match="maskclip_refine: logits "):
            hip.maskclip_refine(bad, k)
    wide = torch.zeros(B, H * W, 2 * C)
    for bad in (k.double(), k.half(), k[0], k[:1], k[:, :-1], torch.zeros(B, H * W, 96), torch.zeros(B, H * W, 32), torch.zeros(B, H * W, 1088),
                wide[:, :, ::2], k.transpose(1, 2).contiguous().transpose(1, 2), k.to("meta"), k[:1].expand(B, H * W, C), "k"):
        with pytest.raises(ValueError, match="maskclip_refine: k "):
            hip.maskclip_refine(x, bad)
    for name in ("pd_thresh", "ks_thresh"):
        for bad in (-0.5, float("nan"), float("inf"), "1", None, True):
            with pytest.raises(ValueError, match=f"maskclip_refine: {name} "):
                hip.maskclip_refine(x, k, **{name: bad})
    for o in (x.double(), torch.zeros(B, K, H, W + 1), x.to("meta"), x[:1].expand(B, K, H, W), torch.zeros(B, K, H, 1).expand(B, K, H, W), "out",
              torch.zeros(256).as_strided((B, K, H, W), (1, 1, 5, 15))):
        with pytest.raises(ValueError, match="maskclip_refine: out must be fp32"):
            hip.maskclip_refine(x, k, out=o)
    n = B * K * H * W
    buf = torch.zeros(2 * n)
    for logits, o in ((x, x), (buf[:n].view(B, K, H, W), buf[n - 1:2 * n - 1].view(B, K, H, W))):
        with pytest.raises(ValueError, match="maskclip_refine: out must not overlap logits"):
            hip.maskclip_refine(logits, k, out=o)
    # everything in order: the device check is what stops a CPU call, and k may be None or a strided bf16 view
    for kk in (k, None, wide[:, :, :C], wide.bfloat16()[:, :, C:], torch.zeros(B, H * W + 1, C)[:, 1:]):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            hip.maskclip_refine(x, kk, out=torch.empty(B, K, H, W + 2)[..., 1:W + 1])
    with pytest.raises(ValueError, match="maskclip_refine: logits "):
        hip.maskclip_refine_phase_ms(x.double(), k)


# --------------------------------------------------------------------------------------------- raw entry, no launch
def test_refine_entry_validates_arguments_before_any_launch():
    from openess_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    a = ctypes.addressof(buf)
    a += (-a) % 16
    need = lib.oess_maskclip_refine_workspace_bytes
    assert need(8, 11, 28, 40, 768) >= 8 * 1120 * 16 * 4 + 8 * 9 * 768 * 17 * 4 + 8 * 768 * 16 * 4
    assert 0 < need(8, 11, 28, 40, 0) < need(8, 11, 28, 40, 64)
    for bad in ((0, 11, 5, 7, 64), (65536, 11, 5, 7, 64), (2, 0, 5, 7, 64), (2, 33, 5, 7, 64), (2, 11, 0, 7, 64), (2, 11, 5, 0, 64),
                (2, 11, 64, 65, 64), (2, 11, 5, 7, 32), (2, 11, 5, 7, 96), (2, 11, 5, 7, 1088), (2, 11, 5, 7, -64)):
        assert need(*bad) == 0, bad

    def call(x=a, xs=(385, 35, 7, 1), B=2, K=11, H=5, W=7, k=a, dt=0, krs=64, kis=35 * 64, C=64, pd=0.5, ks=1.0, out=a + 32768,
             os_=(385, 35, 7, 1), ws=a, wsb=1 << 30, entry=lib.oess_maskclip_refine_f32, extra=()):
        return entry(x, *xs, B, K, H, W, k, dt, krs, kis, C, pd, ks, out, *os_, ws, wsb, *extra, None)

    for bad in (dict(x=None), dict(out=None), dict(ws=None), dict(B=0), dict(B=65536), dict(K=0), dict(K=33), dict(H=0), dict(W=0),
                dict(H=64, W=65), dict(C=0), dict(C=32), dict(C=96), dict(C=1088), dict(dt=2), dict(dt=-1), dict(krs=63), dict(kis=34 * 64 + 63),
                dict(kis=-1), dict(krs=1 << 40), dict(pd=-0.5), dict(ks=-1.0), dict(pd=float("nan")), dict(ks=float("nan")),
                dict(pd=float("inf")), dict(ks=float("inf")), dict(xs=(385, 35, 7, -1)), dict(xs=(1 << 40, 35, 7, 1)),
                dict(os_=(385, 35, 7, 0)), dict(os_=(385, 35, 1, 1)), dict(os_=(0, 35, 7, 1)), dict(os_=(385, 35, 7, -1)),
                dict(os_=(1 << 40, 35, 7, 1)), dict(x=a + 2), dict(out=a + 32770), dict(k=a + 2), dict(k=a + 1, dt=1), dict(ws=a + 8)):
        assert call(**bad) == EINVAL, bad
    assert call(wsb=need(2, 11, 5, 7, 64) - 1) == ENOMEM
    assert call(k=None, wsb=need(2, 11, 5, 7, 0) - 1) == ENOMEM                   # without keys the smaller workspace is what counts
    ms = (ctypes.c_float * 5)()
    assert call(entry=lib.oess_maskclip_refine_phase_ms, extra=(None,)) == EINVAL
    assert call(entry=lib.oess_maskclip_refine_phase_ms, extra=(ms,), K=0) == EINVAL
    del buf
