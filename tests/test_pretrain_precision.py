"""Host-side checks of fp32 pre-training (K20): PretrainStep's `precision` argument and the pre-training trainer's `train_precision`
key, their refusals before any model is built, the shipped fp32 YAML, the dtype dispatch of hip.UpsampledNormalizedFeature and
hip.PointwiseFeature, and the argument checks of the two new entry points.  No GPU."""
import inspect
import os

import pytest
import torch
import yaml

CFG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")
CFG = os.path.join(CFG_DIR, "pretrain_dsec_synthetic.yaml")


def _settings(tmp_path, model=None, **clip):
    from openess_amd.config.settings import Settings
    cfg = yaml.load(open(CFG), yaml.Loader)
    cfg['clip'].update(clip)
    cfg['model'].update(model or {})
    path = tmp_path / "settings.yaml"
    path.write_text(yaml.dump(cfg))
    return Settings(str(path), generate_log=False)


@pytest.fixture
def no_models(monkeypatch):
    """Every model constructor PretrainStep and the trainer call raises: a refusal that still passes came before any was built."""
    from openess_amd.training import pretrain_step as ps
    from openess_amd.training import pretrain_trainer as pt

    def boom(*a, **k):
        raise AssertionError("a model was built before the refusal")
    for name in ('E2VIDRecurrent', 'deeplabv3_resnet50', 'DilationFeatureExtractor', 'ImageReconstructor'):
        monkeypatch.setattr(ps, name, boom)
    fake = type('SemSegE2VID', (), {'__init__': boom, 'check_fp32_config': staticmethod(ps.SemSegE2VID.check_fp32_config)})
    monkeypatch.setattr(ps, 'SemSegE2VID', fake)
    monkeypatch.setattr(pt.BaseTrainer, '__init__', boom)


def test_precision_value_is_validated(no_models):
    from openess_amd.training.pretrain_step import PretrainStep
    for bad in ('fp16', 'FP32', 32, None, True):
        with pytest.raises(ValueError, match="precision"):
            PretrainStep(precision=bad, device='cpu')


def test_fp32_refusals_come_before_any_model(no_models):
    from openess_amd.training.pretrain_step import PretrainStep
    with pytest.raises(NotImplementedError, match="DeepLabv3 has no fp32 backward"):
        PretrainStep(config_option='frame2recon', precision='fp32', device='cpu')
    with pytest.raises(NotImplementedError, match="ViT has no fp32 form"):
        PretrainStep(online_teacher=lambda x: x, precision='fp32', device='cpu')
    with pytest.raises(NotImplementedError, match="wavefront"):
        PretrainStep(wavefront=True, precision='fp32', device='cpu')
    # what is served gets past the refusals and into the (patched) first constructor; so does every bf16 configuration
    with pytest.raises(AssertionError, match="before the refusal"):
        PretrainStep(precision='fp32', if_spatial_contrastive=True, device='cpu')
    for kw in ({'config_option': 'frame2recon'}, {'online_teacher': lambda x: x}, {'wavefront': True}, {}):
        with pytest.raises(AssertionError, match="before the refusal"):
            PretrainStep(device='cpu', **kw)


def test_default_signature_is_unchanged_and_positional():
    from openess_amd.training.pretrain_step import PretrainStep
    names = list(inspect.signature(PretrainStep.__init__).parameters)
    assert names == ['self', 'config_option', 'num_classes', 'img_size', 'nr_events_data', 'nr_temporal_bins', 'if_spatial_contrastive',
                     'if_dense_clip_supervision', 'superpixel_size', 'lr', 'weight_task_loss', 'task_loss', 'output_stride', 'device',
                     'e2vid_config', 'text_embeddings', 'seed', 'online_teacher', 'wavefront', 'precision']
    assert inspect.signature(PretrainStep.__init__).parameters['precision'].default == 'bf16'
    st = PretrainStep('frame2voxel', 11, (32, 48), 2, 5, True, True, 25, 1e-4, 1.0, ('dice', 'cross_entropy'), 32, 'cpu')
    assert st.precision == 'bf16' and getattr(st, 'reconstructor_fp32', None) is None and st.reconstructor.precision == 'bf16'
    assert st.task_backend.materialize_ch256 == 'pooled' and st.model_frame.lazy_features


def test_fp32_step_builds_one_more_reconstructor_over_the_same_model():
    from openess_amd.training.pretrain_step import PretrainStep
    st = PretrainStep(img_size=(32, 48), nr_events_data=2, if_spatial_contrastive=True, superpixel_size=25, device='cpu', precision='fp32')
    assert st.precision == 'fp32' and st.reconstructor.precision == 'bf16' and st.reconstructor_fp32.precision == 'fp32'
    assert st.reconstructor_fp32.model is st.reconstructor.model is st.front_end_sensor_b
    assert sorted(st.models_dict) == ['back_end', 'front_sensor_b', 'model_frame']
    assert sorted(st.optimizers_dict) == ['optimizer_frame', 'optimizer_voxel']
    assert st.task_backend.materialize_ch256 == 'pooled' and st.model_frame.lazy_features


def test_trainer_refusals_come_before_any_model(tmp_path, no_models):
    from openess_amd.training.pretrain_trainer import OpenESSPretrainModel
    s = _settings(tmp_path, train_precision='fp32', config_option='frame2recon')
    with pytest.raises(NotImplementedError, match="DeepLabv3.*no fp32 backward"):
        OpenESSPretrainModel(settings=s)
    s = _settings(tmp_path, train_precision='fp32', pl_sources='online_maskclip')
    with pytest.raises(NotImplementedError, match="ViT has no fp32 form"):
        OpenESSPretrainModel(settings=s)
    s = _settings(tmp_path, model={'unfrozen_e2vid': True}, train_precision='fp32')
    with pytest.raises(NotImplementedError, match="unfrozen_e2vid"):
        OpenESSPretrainModel(settings=s)
    s = _settings(tmp_path)
    s.train_precision = 'half'
    with pytest.raises(ValueError, match="train_precision"):
        OpenESSPretrainModel(settings=s)
    for clip in ({'train_precision': 'fp32'}, {}, {'config_option': 'frame2recon'}):
        with pytest.raises(AssertionError, match="before the refusal"):
            OpenESSPretrainModel(settings=_settings(tmp_path, **clip))


def test_trainer_sets_train_precision_before_the_base_constructor(tmp_path, monkeypatch):
    from openess_amd.training import pretrain_trainer as pt
    seen = []
    monkeypatch.setattr(pt.BaseTrainer, '__init__', lambda self, settings, train=True: seen.append(self.train_precision))
    pt.OpenESSPretrainModel(settings=_settings(tmp_path, train_precision='fp32'))
    pt.OpenESSPretrainModel(settings=_settings(tmp_path))
    assert seen == ['fp32', 'bf16']


def test_shipped_fp32_yaml_differs_from_the_bf16_one_by_the_key_alone():
    fp32 = yaml.load(open(os.path.join(CFG_DIR, "pretrain_dsec_synthetic_fp32.yaml")), yaml.Loader)
    bf16 = yaml.load(open(CFG), yaml.Loader)
    assert fp32['clip'].pop('train_precision') == 'fp32'
    assert bf16['clip']['if_spatial_contrastive'] is True and bf16['clip']['config_option'] == 'frame2voxel'
    assert fp32 == bf16


def test_feature_holders_dispatch_on_dtype_before_any_launch():
    from openess_amd import hip
    with pytest.raises(ValueError, match="C in"):
        hip.UpsampledNormalizedFeature(torch.zeros(1, 96, 4, 4), 4)
    for dtype in (torch.float16, torch.float64):
        with pytest.raises(ValueError, match="bfloat16 or float32"):
            hip.UpsampledNormalizedFeature(torch.zeros(1, 64, 4, 4, dtype=dtype), 4)
    for C in hip.HEADPOOL_F32_CHANNELS:
        assert hip.UpsampledNormalizedFeature(torch.zeros(1, C, 4, 4), 4).shape == (1, C, 16, 16)
    assert hip.UpsampledNormalizedFeature(torch.zeros(1, 512, 4, 4, dtype=torch.bfloat16), 4).shape == (1, 512, 16, 16)
    with pytest.raises(RuntimeError):                                  # a CPU tensor never reaches a kernel
        hip.UpsampledNormalizedFeature(torch.zeros(1, 64, 4, 4), 4).pool(torch.zeros(1, 16, 16, dtype=torch.int64), 10, 10)
    with pytest.raises(ValueError, match="float32"):
        hip._BilinearL2NormPoolF32.apply(torch.zeros(1, 64, 4, 4, dtype=torch.bfloat16), 4, torch.zeros(256, dtype=torch.int64), 10, 10)

    calls = []
    conv = type('Conv', (), {'weight': torch.zeros(256, 32, 1, 1), 'bias': None, '__call__': lambda self, x: calls.append('bf16') or x,
                             'forward_f32_train': lambda self, x: calls.append('fp32') or x})()
    hip.PointwiseFeature(torch.zeros(1, 32, 4, 4), conv).materialize()
    hip.PointwiseFeature(torch.zeros(1, 32, 4, 4, dtype=torch.bfloat16), conv).materialize()
    assert calls == ['fp32', 'bf16']
    with pytest.raises(ValueError, match="bfloat16 or float32"):
        hip.PointwiseFeature(torch.zeros(1, 32, 4, 4, dtype=torch.float64), conv).materialize()
    with pytest.raises(ValueError, match="bfloat16 or float32"):
        hip.PointwiseFeature(torch.zeros(1, 32, 4, 4, dtype=torch.float16), conv).pool(torch.zeros(1, 4, 4, dtype=torch.int64), 10, 10)


def test_semseg_keeps_refusing_pooled_for_inference_and_serves_it_for_training():
    from openess_amd.models.style_networks import SemSegE2VID
    with pytest.raises(NotImplementedError, match="no 'pooled' form"):
        SemSegE2VID.check_fp32_config('concat', 'pooled')
    SemSegE2VID.check_fp32_config('concat', 'pooled', train=True)
    with pytest.raises(NotImplementedError, match="concat"):
        SemSegE2VID.check_fp32_config('sum', 'pooled', train=True)
    net = SemSegE2VID(256, 11, skip_connect=True, skip_type='concat', text_embeddings_path='', materialize_ch256='pooled')
    with pytest.raises(NotImplementedError, match="no 'pooled' form"):
        net.forward_fp32({k: torch.zeros(1, 1, 8, 8) for k in (1, 2, 4, 8)})
    with pytest.raises(ValueError, match="fp32 latents"):              # past the configuration check, refused on the latents' dtype
        net.forward_fp32_train({k: torch.zeros(1, 1, 8, 8, dtype=torch.bfloat16) for k in (1, 2, 4, 8)})


def test_teacher_head_fp32_train_refuses_other_dtypes():
    from openess_amd.models.image_model import DilationFeatureExtractor
    m = DilationFeatureExtractor(image_weights=None)
    with pytest.raises(ValueError, match="float32"):
        m.head_fp32_train(torch.zeros(1, 2048, 2, 2, dtype=torch.bfloat16))


def test_new_entry_points_validate_arguments_on_the_host():
    from openess_amd import _lib
    lib = _lib.load()
    assert lib.oess_abi_version() == 13 == _lib.ABI_VERSION
    fwd, bwd = lib.oess_bilinear_l2norm_pool_fwd_f32, lib.oess_bilinear_l2norm_pool_bwd_f32
    assert fwd(None, 256, None, 100, 800, 8, 110, 160, 256, 4, 1, 1e-12, None, None, None, 0, None) == -22
    assert bwd(None, 256, None, None, None, 100, 800, 8, 110, 160, 256, 4, 1, 1e-12, None, 0, None, 256, None) == -22
    buf = (16 * 4 * 64 + 4096) * 4                                       # host memory is enough: every check precedes the launch
    import ctypes
    mem = ctypes.create_string_buffer(buf + 64)
    base = (ctypes.addressof(mem) + 63) & ~63
    ok = dict(ids=base, k=base, count=base, ws=base)
    for C, stride, x in ((96, 96, base), (64, 65, base), (64, 64, base + 4), (64, 32, base)):       # C, pixel stride, alignment, stride < C
        assert fwd(x, stride, ok['ids'], 50, 50, 1, 4, 4, C, 4, 1, 1e-12, ok['k'], ok['count'], ok['ws'], 1 << 30, None) == -22, (C, stride)
        assert bwd(x, stride, ok['ids'], base, base, 50, 50, 1, 4, 4, C, 4, 1, 1e-12, ok['ws'], 1 << 30, base, C, None) == -22, (C, stride)
    assert fwd(base, 64, base, 50, 50, 1, 4, 4, 64, 0, 1, 1e-12, base, base, base, 1 << 30, None) == -22       # scale < 1
    assert fwd(base, 64, base, 50, 50, 1, 4, 4, 64, 4, 1, 0.0, base, base, base, 1 << 30, None) == -22         # eps <= 0
    assert fwd(base, 64, base, 50, 50, 1, 4, 4, 64, 4, 1, 1e-12, base, base, base, 16, None) == -12            # workspace too small
    assert bwd(base, 64, base, base, base, 50, 50, 1, 4, 4, 64, 4, 1, 1e-12, base, 16, base, 64, None) == -12
