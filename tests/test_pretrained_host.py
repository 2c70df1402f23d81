"""Host-side checks of the pretrained-weight loading (K33): adapt_weights' key rules, the E2VID checkpoint loader, the trainers'
refusals before any model is built, the missing-file fallback (seeded weights bit for bit, one warning per network) and the
settings keys.  No GPU."""
import logging

import pytest
import torch

from tests import pretrained_cases as pc


# ------------------------------------------------------------------ adapt_weights
@pytest.mark.parametrize("name", sorted(pc.TEACHER_LAYOUTS))
def test_adapt_weights_key_rules(tmp_path, name):
    from openess_amd.models.image_model import IMAGE_WEIGHTS, adapt_weights
    assert sorted(IMAGE_WEIGHTS) == sorted(pc.TEACHER_LAYOUTS)
    keys = pc.resnet50_keys()
    assert len(keys) == 318 and not any(k.startswith('fc.') for k in keys)
    plain = {k: torch.full((1,), float(i)) for i, k in enumerate(keys)}
    path = pc.write_teacher(tmp_path / f"{name}.pt", name, plain)
    got = adapt_weights(name, path)
    if pc.TEACHER_LAYOUTS[name][1] == '':
        # the files with plain keys keep everything; fc.* leaves in ResNetEncoder.load_state_dict (checked below on a real module)
        assert got.pop('fc.weight').numel() == 1 and got.pop('fc.bias').numel() == 1
    assert list(got) == keys
    for k in keys:
        assert torch.equal(got[k], plain[k]), k


def test_adapt_weights_refuses_an_unknown_name_and_loads_strictly(tmp_path):
    from openess_amd.models.image_model import DilationFeatureExtractor, adapt_weights
    state = pc.teacher_state()
    path = pc.write_teacher(tmp_path / "w.pt", 'imagenet', state)
    with pytest.raises(ValueError, match="image_weights.*'byol'"):
        adapt_weights('byol', path)
    with pytest.raises(ValueError, match="image_weights.*'byol'"):
        DilationFeatureExtractor('byol', weights_path=path)
    t = DilationFeatureExtractor('imagenet', weights_path=path)            # fc.* in the file is dropped, the rest is strict
    for k, v in state.items():
        assert torch.equal(t.encoder.state_dict()[k], v), k
    assert not any(p.requires_grad for p in t.encoder.parameters()) and all(p.requires_grad for p in t.decoder.parameters())
    short = dict(state)
    short.pop('layer4.2.conv3.weight')
    torch.save(short, str(tmp_path / "short.pt"))
    with pytest.raises(RuntimeError, match="layer4.2.conv3.weight"):
        DilationFeatureExtractor('dino', weights_path=str(tmp_path / "short.pt"))
    with pytest.raises(FileNotFoundError):
        DilationFeatureExtractor('dino', weights_path=str(tmp_path / "absent.pt"))
    for nothing in (None, '', 'none', 'random'):                           # no file is looked for
        DilationFeatureExtractor(nothing, weights_path=str(tmp_path / "absent.pt"))


# ------------------------------------------------------------------ load_model
@pytest.mark.parametrize("config,spelling,prefix", [(pc.LIGHT, 'model', False), (pc.LIGHT, 'config', False), (pc.LIGHT, 'model', True),
                                                    (pc.GRU, 'config', True)])
def test_load_model_round_trip(tmp_path, config, spelling, prefix):
    from openess_amd.e2vid.run_reconstruction import load_model as load_for_reconstruction
    from openess_amd.e2vid.utils.loading_utils import load_model
    path = str(tmp_path / "e2vid.pth.tar")
    state = pc.write_e2vid(path, config, spelling=spelling, module_prefix=prefix)
    model, decoder = load_model(path)
    assert decoder is None and model.recurrent_block_type == config['recurrent_block_type']
    assert list(model.state_dict()) == list(state)
    for k, v in state.items():
        assert torch.equal(model.state_dict()[k], v), k
    again = load_for_reconstruction(path)                                 # delegates; returns the model alone, as before
    assert all(torch.equal(again.state_dict()[k], v) for k, v in state.items())


def test_load_model_refusals(tmp_path):
    from openess_amd.e2vid.utils.loading_utils import load_model
    path = str(tmp_path / "e2vid.pth.tar")
    pc.write_e2vid(path, arch='E2VID')
    with pytest.raises(NotImplementedError, match="arch 'E2VID'"):
        load_model(path)
    state = pc.e2vid_state()
    state.pop('unetrecurrent.encoders.2.recurrent_block.Gates.weight')        # a truncated state dict
    pc.write_e2vid(path, state=state)
    with pytest.raises(RuntimeError, match="Missing key.*encoders.2.recurrent_block.Gates.weight"):
        load_model(path)
    torch.save({'arch': 'E2VIDRecurrent', 'state_dict': pc.e2vid_state()}, path)
    with pytest.raises(ValueError, match="no model config"):
        load_model(path)


# ------------------------------------------------------------------ refusals before construction
@pytest.fixture
def no_models(monkeypatch):
    """Every model constructor the trainers and PretrainStep call raises: a refusal that still passes came before any was built."""
    from openess_amd.training import _supervised as sup
    from openess_amd.training import pretrain_step as ps
    from openess_amd.training import pretrain_trainer as pt

    def boom(*a, **k):
        raise AssertionError("a model was built before the refusal")
    for mod, names in ((sup, ('E2VIDRecurrent', 'deeplabv3_resnet50', 'ImageReconstructor')),
                       (ps, ('E2VIDRecurrent', 'deeplabv3_resnet50', 'DilationFeatureExtractor', 'ImageReconstructor'))):
        for name in names:
            monkeypatch.setattr(mod, name, boom)
        fake = type('SemSegE2VID', (), {'__init__': boom, 'check_fp32_config': staticmethod(mod.SemSegE2VID.check_fp32_config)})
        monkeypatch.setattr(mod, 'SemSegE2VID', fake)
    monkeypatch.setattr(sup.BaseTrainer, '__init__', boom)
    assert pt.BaseTrainer is sup.BaseTrainer


def _trainers():
    from openess_amd.training.finetune_trainer import OpenESSFineTuneModel
    from openess_amd.training.pretrain_trainer import OpenESSPretrainModel
    return ((OpenESSPretrainModel, "pretrain_dsec_synthetic.yaml"), (OpenESSFineTuneModel, "finetune_dsec_synthetic.yaml"))


BAD_CONFIGS = [(dict(pc.LIGHT, num_bins=3), "num_bins = 3.*nr_temporal_bins is 5"),
               (dict(pc.LIGHT, num_encoders=4), "num_encoders = 4.*SemSegE2VID"),
               (dict(pc.LIGHT, base_num_channels=16), "base_num_channels = 16.*SemSegE2VID")]


@pytest.mark.parametrize("config,message", BAD_CONFIGS)
def test_checkpoints_the_trainers_cannot_run_are_refused_before_any_model(tmp_path, no_models, config, message):
    from openess_amd.training.pretrain_step import PretrainStep
    path = str(tmp_path / "e2vid.pth.tar")
    pc.write_e2vid(path, config)
    for cls, base in _trainers():
        with pytest.raises(ValueError, match=message):
            cls(settings=pc.settings(tmp_path, base, config_option='frame2voxel', e2vid_checkpoint=path))
    with pytest.raises(ValueError, match=message):
        PretrainStep(device='cpu', e2vid_checkpoint=path)


def test_fp32_keys_refuse_what_the_fp32_step_does_not_run(tmp_path, no_models):
    path = str(tmp_path / "e2vid.pth.tar")
    pc.write_e2vid(path, dict(pc.LIGHT, norm='IN'))
    for cls, base in _trainers():
        with pytest.raises(NotImplementedError, match="norm='IN'"):
            cls(settings=pc.settings(tmp_path, base, config_option='frame2voxel', e2vid_checkpoint=path, train_precision='fp32'))
        with pytest.raises(AssertionError, match="before the refusal"):       # bf16 leaves it to the kernels' own check, as now
            cls(settings=pc.settings(tmp_path, base, config_option='frame2voxel', e2vid_checkpoint=path))
    with pytest.raises(NotImplementedError, match="norm='IN'"):
        _trainers()[1][0](settings=pc.settings(tmp_path, _trainers()[1][1], config_option='frame2voxel', e2vid_checkpoint=path,
                                               eval_precision='fp32'))


def test_a_file_that_fits_and_a_file_that_is_absent_get_past_the_refusals(tmp_path, no_models):
    path = str(tmp_path / "e2vid.pth.tar")
    pc.write_e2vid(path, pc.GRU)                                              # ConvGRU checkpoints are accepted
    for cls, base in _trainers():
        for kw in ({'e2vid_checkpoint': path}, {'e2vid_checkpoint': str(tmp_path / "absent.pth.tar")}, {}):
            with pytest.raises(AssertionError, match="before the refusal"):
                cls(settings=pc.settings(tmp_path, base, config_option='frame2voxel', **kw))
    pc.write_e2vid(path, arch='E2VID')
    for cls, base in _trainers():                                             # exists and does not fit: always raises
        with pytest.raises(NotImplementedError, match="arch 'E2VID'"):
            cls(settings=pc.settings(tmp_path, base, config_option='frame2voxel', e2vid_checkpoint=path))


def test_require_pretrained_names_the_key_of_the_missing_file(tmp_path, no_models):
    from openess_amd.training.pretrain_step import PretrainStep
    absent = str(tmp_path / "absent.pt")
    pre, ft = _trainers()
    cases = [(pre, 'frame2voxel', {'e2vid_checkpoint': absent}, "e2vid_checkpoint"),
             (pre, 'frame2voxel', {}, "path_to_model.*E2VID_lightweight.pth.tar"),
             (ft, 'frame2voxel', {'e2vid_checkpoint': absent}, "e2vid_checkpoint"),
             (ft, 'recon2voxel', {}, "path_to_model"),
             (pre, 'frame2recon', {'image_weights': 'dino', 'image_weights_path': absent}, "image_weights_path"),
             (pre, 'frame2recon', {'image_weights': 'moco_v2'}, "image_weights: 'weights/moco_v2.pt'"),
             (pre, 'frame2recon', {'pre_trained_backbone': absent}, "pre_trained_backbone"),
             (ft, 'frame2recon', {'pre_trained_backbone': absent}, "pre_trained_backbone")]
    for (cls, base), option, keys, message in cases:
        with pytest.raises(FileNotFoundError, match="require_pretrained.*" + message):
            cls(settings=pc.settings(tmp_path, base, config_option=option, require_pretrained=True, **keys))
        if cls is pre[0] or option != 'frame2recon':
            # without the key the same settings reach the (patched) base constructor
            with pytest.raises(AssertionError, match="before the refusal"):
                cls(settings=pc.settings(tmp_path, base, config_option=option, **keys))
    for kw, message in (({'e2vid_checkpoint': absent}, "e2vid_checkpoint"),
                        ({'image_weights': 'dino', 'image_weights_path': absent}, "image_weights_path"),
                        ({'config_option': 'frame2recon', 'pretrained_backbone': absent}, "pre_trained_backbone")):
        with pytest.raises(FileNotFoundError, match=message):
            PretrainStep(device='cpu', require_pretrained=True, **kw)


# ------------------------------------------------------------------ fallback
def _parent_state(config_option, seed=1205):
    """PretrainStep's networks as the parent commit builds them: torch.manual_seed(seed), then the same constructors."""
    from openess_amd.e2vid.model.model import E2VID_LIGHTWEIGHT_CONFIG, E2VIDRecurrent
    from openess_amd.models.deeplabv3 import deeplabv3_resnet50
    from openess_amd.models.image_model import DilationFeatureExtractor
    from openess_amd.models.style_networks import SemSegE2VID
    torch.manual_seed(seed)
    nets = {}
    if config_option == 'frame2voxel':
        nets['front_sensor_b'] = E2VIDRecurrent(E2VID_LIGHTWEIGHT_CONFIG)
        nets['back_end'] = SemSegE2VID(input_c=256, output_c=11, skip_connect=True, skip_type='concat', text_embeddings_path='',
                                       materialize_ch256=False)
    else:
        nets['model_recon'] = deeplabv3_resnet50(num_classes=11, text_embeddings_path='', output_stride=32, pretrained_backbone='')
    nets['model_frame'] = DilationFeatureExtractor(image_weights=None)
    return {f"{n}.{k}": v for n, m in nets.items() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("config_option", ['frame2voxel', 'frame2recon'])
def test_missing_files_leave_the_seeded_weights_and_one_warning_per_network(tmp_path, caplog, config_option):
    from openess_amd.training.pretrain_step import PretrainStep
    absent = str(tmp_path / "absent.pt")
    want = _parent_state(config_option)
    kw = dict(config_option=config_option, img_size=(32, 48), nr_events_data=2, device='cpu')
    plain = PretrainStep(**kw)                                               # the defaults: no file is looked for
    with caplog.at_level(logging.WARNING):
        caplog.clear()
        st = PretrainStep(e2vid_checkpoint=absent, image_weights='dino', image_weights_path=absent, pretrained_backbone=absent, **kw)
    for step in (plain, st):
        got = {f"{n}.{k}": v for n, m in step.models_dict.items() for k, v in m.state_dict().items()}
        assert list(got) == list(want)
        for k, v in want.items():
            assert torch.equal(got[k], v), k
    warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    first = 'e2vid_checkpoint' if config_option == 'frame2voxel' else 'pre_trained_backbone'
    assert len(warned) == 2 and first in warned[0] and 'image_weights_path' in warned[1]
    assert all(absent in w and 'seeded random weights' in w for w in warned)


def test_build_models_of_a_stage_2_trainer_warns_once_and_keeps_the_seeded_front_end(tmp_path, caplog, monkeypatch):
    from openess_amd.e2vid.model.model import E2VID_LIGHTWEIGHT_CONFIG, E2VIDRecurrent
    from openess_amd.training.finetune_trainer import OpenESSFineTuneModel
    s = pc.settings(tmp_path, "finetune_dsec_synthetic.yaml", config_option='frame2voxel')
    tr = object.__new__(OpenESSFineTuneModel)
    tr.settings, tr.device, tr.train_precision, tr.eval_precision = s, torch.device('cpu'), 'bf16', 'bf16'
    torch.manual_seed(7)
    with caplog.at_level(logging.WARNING):
        tr.buildModels()
    torch.manual_seed(7)
    want = E2VIDRecurrent(E2VID_LIGHTWEIGHT_CONFIG).state_dict()
    assert all(torch.equal(tr.front_end_sensor_b.state_dict()[k], v) for k, v in want.items())
    warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warned) == 1 and 'path_to_model' in warned[0] and 'E2VID_lightweight.pth.tar' in warned[0]
    # and a file that exists is what the front end holds, built from the file's own config
    path = str(tmp_path / "gru.pth.tar")
    state = pc.write_e2vid(path, pc.GRU)
    tr.settings = pc.settings(tmp_path, "finetune_dsec_synthetic.yaml", config_option='frame2voxel', e2vid_checkpoint=path)
    with caplog.at_level(logging.INFO):
        caplog.clear()
        tr.buildModels()
    assert tr.front_end_sensor_b.recurrent_block_type == 'convgru' and not tr.front_end_sensor_b.training
    assert all(torch.equal(tr.front_end_sensor_b.state_dict()[k], v) for k, v in state.items())
    assert not any(p.requires_grad for p in tr.front_end_sensor_b.parameters())
    loaded = [r.getMessage() for r in caplog.records if r.getMessage().startswith('loaded')]
    n_params = sum(v.numel() for v in state.values())
    assert len(loaded) == 1 and path in loaded[0] and f"{len(state)} tensors" in loaded[0] and f"{n_params} parameters" in loaded[0]


# ------------------------------------------------------------------ settings
def test_settings_keys_parse_and_default(tmp_path):
    for base in ("pretrain_dsec_synthetic.yaml", "finetune_dsec_synthetic.yaml"):
        s = pc.settings(tmp_path, base)
        assert (s.e2vid_checkpoint, s.image_weights_path, s.require_pretrained) == (None, None, False)
        assert s.path_to_model == 'e2vid/pretrained/E2VID_lightweight.pth.tar' and s.pretrained_backbone == ''
        s = pc.settings(tmp_path, base, e2vid_checkpoint='a/b.pth.tar', image_weights_path='w/dino.pt', require_pretrained=True)
        assert (s.e2vid_checkpoint, s.image_weights_path, s.require_pretrained) == ('a/b.pth.tar', 'w/dino.pt', True)
        assert s.path_to_model == 'e2vid/pretrained/E2VID_lightweight.pth.tar'
    for key, bad in (('e2vid_checkpoint', 3), ('e2vid_checkpoint', ''), ('image_weights_path', ['x']), ('require_pretrained', 'yes'),
                     ('require_pretrained', 1)):
        with pytest.raises(ValueError, match=key):
            pc.settings(tmp_path, **{key: bad})
    from openess_amd.training import pretrained
    assert pretrained.e2vid_path(pc.settings(tmp_path)) == ('path_to_model', 'e2vid/pretrained/E2VID_lightweight.pth.tar')
    assert pretrained.e2vid_path(pc.settings(tmp_path, e2vid_checkpoint='x.tar')) == ('e2vid_checkpoint', 'x.tar')
