"""Host side of K34 (no GPU): the float64 restatement on two hand-computed cases, the settings keys of the shipped YAML, the new C
entries in the header, the binding and the library, their refusals (they return before any HIP call), the construction refusals
of the step and the trainer, the loader's `sam_feature_sources`, and PretrainStep's keyword-only option."""
import ctypes
import inspect
import os
import random
import re

import numpy as np
import pytest
import torch
import yaml

from tests import sam_distill_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "configs")
SAM_YAML = os.path.join(CFG, "pretrain_dsec_synthetic_frame2recon_sam.yaml")
ENTRIES = {"oess_upsampled_cosine_workspace_bytes": 6, "oess_upsampled_cosine_planes_floats": 3, "oess_upsampled_cosine_fwd": 22,
           "oess_upsampled_cosine_bwd": 21}


# ------------------------------------------------------------------------------------------------------------ the reference
def test_reference_constant_positive_map_against_ones_is_zero():
    """every interpolated student vector is k (1, ..., 1), every SAM vector (1, ..., 1): cos = 1 everywhere"""
    amap = torch.full((2, 8, 3, 4), 2.5)
    loss, grad, min_norm = sr.from_map(torch.ones(2, 8, 5, 5), amap, (9, 13))
    assert abs(float(loss)) < 1e-12 and float(grad.abs().max()) < 1e-12 and min_norm > 1


def test_reference_channel_disjoint_supports_give_one():
    """the student lives on channels 0..3, the SAM map on 4..7: every dot product is 0, the loss exactly 1"""
    g = torch.Generator().manual_seed(1)
    amap = torch.zeros(1, 8, 2, 3)
    amap[:, :4] = 1 + torch.rand(1, 4, 2, 3, generator=g)
    sam = torch.zeros(1, 8, 4, 4)
    sam[:, 4:] = 1 + torch.rand(1, 4, 4, 4, generator=g)
    loss, grad, _ = sr.from_map(sam, amap, (5, 7))
    assert float(loss) == 1.0
    assert float(grad[:, 4:].abs().max()) > 0 and float(grad[:, :4].abs().max()) == 0      # d cos / da = t / (|a| |t|) at cos = 0


def test_reference_crops_the_rows_of_the_square_map():
    sam = torch.arange(16.).reshape(1, 1, 4, 4) + 1
    feat = torch.ones(1, 1, 2, 8, dtype=torch.float64)
    _, sam_up = sr.distill(sam.double(), feat)
    full = torch.nn.functional.interpolate(sam.double(), size=(8, 8), mode='bilinear', align_corners=False)
    assert tuple(sam_up.shape) == (1, 1, 2, 8) and torch.equal(sam_up, full[:, :, :2])


def test_case_inputs_stay_clear_of_the_clamp():
    for i, align in sr.variants():
        for bf16 in (False, True):
            assert sr.case(i, bf16, align)['min_norm'] > sr.MIN_NORM


# ------------------------------------------------------------------------------------------------------------ settings
def test_settings_on_the_shipped_yaml(tmp_path):
    from openess_amd.config.settings import Settings
    s = Settings(SAM_YAML, generate_log=False)
    assert s.if_sam_distillation is True and s.config_option == 'frame2recon' and s.sam_feature_sources == ''
    new = yaml.load(open(SAM_YAML), yaml.Loader)
    old = yaml.load(open(os.path.join(CFG, "pretrain_dsec_synthetic.yaml")), yaml.Loader)
    assert new['clip'].pop('if_sam_distillation') is True and old['clip'].pop('if_sam_distillation') is False
    assert new['clip'].pop('config_option') == 'frame2recon' and old['clip'].pop('config_option') == 'frame2voxel'
    assert new == old                                                     # the two differ by these keys alone
    new['clip'].update(if_sam_distillation=True, config_option='frame2recon', sam_feature_sources=3)
    (tmp_path / "bad.yaml").write_text(yaml.dump(new))
    with pytest.raises(ValueError, match="sam_feature_sources"):
        Settings(str(tmp_path / "bad.yaml"), generate_log=False)
    new['clip']['sam_feature_sources'] = 'sam_feats'
    (tmp_path / "named.yaml").write_text(yaml.dump(new))
    assert Settings(str(tmp_path / "named.yaml"), generate_log=False).sam_feature_sources == 'sam_feats'


# ------------------------------------------------------------------------------------------------------------ the entries
def test_entries_are_declared_bound_and_exported():
    from openess_amd import _lib
    header = open(os.path.join(ROOT, "include", "oess.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        m = re.search(r"(size_t|int)\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m and len(m.group(2).split(',')) == nargs, name
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_size_t if m.group(1) == 'size_t' else ctypes.c_int) and len(args) == nargs
        assert hasattr(cdll, name) and getattr(lib, name).argtypes == args
    assert lib.oess_abi_version() == 13 == _lib.ABI_VERSION and int(re.search(r"#define\s+OESS_ABI_VERSION\s+(\d+)", header).group(1)) == 13


def test_entries_refuse_on_the_host():
    """every refusal returns before the first HIP call: the pointers are never read"""
    from openess_amd import _lib
    lib = _lib.load()
    ok = dict(a=4096, bf16=0, aps=8, t=8192, tps=8, B=2, h=2, w=3, C=8, Ho=4, Wo=6, ac=0, ht=5, wt=5, Mh=6, Mw=6, ws=1 << 16, nws=1 << 12,
              planes=1 << 17, loss=1 << 18, g=1 << 19, ga=1 << 20, gaps=8)

    def fwd(**kw):
        k = dict(ok, **kw)
        return lib.oess_upsampled_cosine_fwd(k['a'], k['bf16'], k['aps'], k['t'], k['tps'], k['B'], k['h'], k['w'], k['C'], k['Ho'], k['Wo'],
                                             k['ac'], k['ht'], k['wt'], k['Mh'], k['Mw'], 1e-8, k['ws'], k['nws'], k['planes'], k['loss'], None)

    def bwd(**kw):
        k = dict(ok, **kw)
        return lib.oess_upsampled_cosine_bwd(k['a'], k['bf16'], k['aps'], k['t'], k['tps'], k['B'], k['h'], k['w'], k['C'], k['Ho'], k['Wo'],
                                             k['ac'], k['ht'], k['wt'], k['Mh'], k['Mw'], k['planes'], k['g'], k['ga'], k['gaps'], None)
    common = (dict(a=None), dict(t=None), dict(C=6), dict(C=0), dict(C=1028, aps=1028, tps=1028, gaps=1028), dict(Ho=1), dict(Wo=2),
              dict(aps=7), dict(tps=4), dict(B=0), dict(h=0), dict(w=-1), dict(Ho=-4), dict(ht=0), dict(wt=-1), dict(Mh=3), dict(Mw=5),
              dict(bf16=1, aps=6))
    need = lib.oess_upsampled_cosine_workspace_bytes(2, 2, 3, 8, 4, 6)
    assert 0 < need <= ok['nws']
    for bad in common + (dict(ws=None), dict(loss=None), dict(nws=need - 1), dict(nws=0), dict(ws=(1 << 16) + 4)):
        assert fwd(**bad) == -22, bad
    for bad in common + (dict(planes=None), dict(g=None), dict(ga=None), dict(gaps=7)):
        assert bwd(**bad) == -22, bad
    for bad in (dict(C=6), dict(C=1028), dict(Ho=1), dict(Wo=2), dict(B=0), dict(h=0)):
        k = dict(ok, **bad)
        assert lib.oess_upsampled_cosine_workspace_bytes(k['B'], k['h'], k['w'], k['C'], k['Ho'], k['Wo']) == 0, bad
    assert lib.oess_upsampled_cosine_planes_floats(2, 4, 6) == 2 * 2 * 4 * 6 and lib.oess_upsampled_cosine_planes_floats(2, 0, 6) == 0


def test_wrapper_refuses_cpu_tensors():
    from openess_amd import hip
    with pytest.raises(ValueError, match="no CPU fallback"):
        hip.sam_distill_loss(torch.ones(1, 4, 2, 2), torch.ones(1, 4, 2, 2))
    with pytest.raises(ValueError, match="no CPU fallback"):
        hip.sam_distill_loss(torch.ones(1, 4, 2, 2), hip.UpsampledFeature(torch.ones(1, 4, 1, 1), (2, 2)))


# ------------------------------------------------------------------------------------------------------------ the step and the trainer
def test_step_option_is_keyword_only_and_off_by_default():
    from openess_amd.training.pretrain_step import PretrainStep
    sig = inspect.signature(PretrainStep.__init__, follow_wrapped=False)
    p = sig.parameters['sam_distillation']
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert 'sam_feat' in inspect.signature(PretrainStep.task_train_step).parameters
    assert inspect.signature(PretrainStep.task_train_step).parameters['sam_feat'].default is None
    kw = dict(img_size=(32, 48), nr_events_data=2, device='cpu')
    assert PretrainStep(**kw).sam_distillation is False
    for contrastive, sam, lazy in ((False, False, False), (True, False, True), (False, True, True), (True, True, True)):
        st = PretrainStep(config_option='frame2recon', if_spatial_contrastive=contrastive, sam_distillation=sam, **kw)
        assert st.sam_distillation is sam and st.model_recon.lazy_feats is lazy


def _raise(*a, **k):
    raise AssertionError("a model was built before the refusal")


def test_step_refuses_frame2voxel_before_any_model_is_built(monkeypatch):
    from openess_amd.training import pretrain_step as ps
    for name in ('E2VIDRecurrent', 'SemSegE2VID', 'deeplabv3_resnet50', 'DilationFeatureExtractor'):
        monkeypatch.setattr(ps, name, _raise)
    with pytest.raises(NotImplementedError, match="KeyError"):
        ps.PretrainStep(config_option='frame2voxel', sam_distillation=True, device='cpu')
    with pytest.raises(AssertionError, match="a model was built"):       # the patch is live: the accepted option reaches the models
        ps.PretrainStep(config_option='frame2recon', sam_distillation=True, device='cpu')


def test_trainer_refuses_frame2voxel_ddd17_and_a_source_without_the_key(monkeypatch):
    from openess_amd.config.settings import Settings
    from openess_amd.training import base_trainer_ov, pretrain_trainer
    monkeypatch.setattr(base_trainer_ov.BaseTrainer, '__init__', _raise)
    monkeypatch.setattr(pretrain_trainer, 'PretrainStep', _raise)
    s = Settings(SAM_YAML, generate_log=False)
    with pytest.raises(AssertionError, match="a model was built"):       # the shipped YAML passes the checks
        pretrain_trainer.OpenESSPretrainModel(s)
    s.config_option = 'frame2voxel'
    with pytest.raises(NotImplementedError, match="KeyError"):
        pretrain_trainer.OpenESSPretrainModel(s)
    s.config_option, s.dataset_name_b = 'frame2recon', 'DDD17_events'
    with pytest.raises(NotImplementedError, match="no SAM feature slot"):
        pretrain_trainer.OpenESSPretrainModel(s)
    s.dataset_name_b, s.if_sam_distillation, s.sam_feature_sources = 'DSEC_events', False, 'sam_feats'
    with pytest.raises(ValueError, match="sam_feature_sources"):
        pretrain_trainer.OpenESSPretrainModel(s)


# ------------------------------------------------------------------------------------------------------------ the loader
def _sequence(tmp_path, **kw):
    from openess_amd.DSEC.dataset.sequence_ov import Sequence
    from tests.synth_datasets import make_dsec_sequence
    seq = tmp_path / "zurich_city_00_a"
    if not seq.is_dir():
        make_dsec_sequence(str(seq), seed=7, n_labels=8, n_events=20000)
    return seq, (lambda **more: Sequence(seq, mode='train', nr_events_data=2, nr_events_per_data=500, config_option='recon_only',
                                         pl_sources='pl_fcclip_rgb', **dict(kw, **more)))


def test_sam_feature_sources_loads_and_flips(tmp_path, monkeypatch):
    seq, build = _sequence(tmp_path)
    rng = np.random.default_rng(34)
    feats = [rng.standard_normal((256, 64, 64)).astype(np.float16 if i == 0 else np.float32) for i in range(2)]
    os.makedirs(seq / "sam_feats" / "left")
    for i, f in enumerate(feats):
        np.save(seq / "sam_feats" / "left" / f"{6 + i:06d}.npy", f)         # the first six label frames are dropped
    ds = build(if_sam_distillation=True, sam_feature_sources='sam_feats')
    assert len(ds) == 2
    for i, f in enumerate(feats):
        got = ds[i][3]
        assert got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(f.astype(np.float32)))
    # without the key: the reference's ones, with or without the loss
    assert torch.equal(build()[0][3], torch.ones(256, 64, 64)) and torch.equal(build(if_sam_distillation=True)[0][3], torch.ones(256, 64, 64))
    # the horizontal flip of the augmentation mirrors the features with the frame
    draws = iter([0.9] + [0.0] * 8)
    monkeypatch.setattr(random, 'random', lambda: next(draws))
    flipped = build(if_sam_distillation=True, sam_feature_sources='sam_feats', augmentation=True)[1]
    assert torch.equal(flipped[3], torch.from_numpy(feats[1]).flip(2))
    assert torch.equal(flipped[0], build()[1][0].flip(1))                 # the label map went the same way


def test_sam_feature_sources_names_a_missing_or_misshapen_file(tmp_path):
    seq, build = _sequence(tmp_path)
    os.makedirs(seq / "sam_feats" / "left")
    ds = build(if_sam_distillation=True, sam_feature_sources='sam_feats')
    with pytest.raises(FileNotFoundError, match="000006.npy"):
        ds[0]
    np.save(seq / "sam_feats" / "left" / "000006.npy", np.zeros((256, 32, 32), np.float32))
    with pytest.raises(ValueError, match="000006.npy"):
        ds[0]
    np.save(seq / "sam_feats" / "left" / "000006.npy", np.zeros((256, 64, 64), np.float64))
    with pytest.raises(ValueError, match="000006.npy"):
        ds[0]
    with pytest.raises(ValueError, match="if_sam_distillation"):
        build(sam_feature_sources='sam_feats')
