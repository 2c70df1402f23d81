"""Host-side checks of the joint OpenESS stage's `train_precision` / `eval_precision` keys (K23): the shipped fp32 YAML, its
dispatch, the refusals at construction (before any model is built) and where the keys land.  No GPU."""
import os

import pytest
import yaml

CFG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")
CFG = os.path.join(CFG_DIR, "openess_dsec_synthetic.yaml")
CFG_FP32 = os.path.join(CFG_DIR, "openess_dsec_synthetic_fp32.yaml")


def _settings(tmp_path, **clip):
    from openess_amd.config.settings import Settings
    cfg = yaml.load(open(CFG), yaml.Loader)
    cfg['clip'].update(clip)
    path = tmp_path / "settings.yaml"
    path.write_text(yaml.dump(cfg))
    return Settings(str(path), generate_log=False)


class Reached(Exception):
    """the patched base constructor: every check of OpenESSModel.__init__ has passed, nothing is built yet"""


@pytest.fixture
def no_models(monkeypatch):
    """The base constructor (which builds the models, and needs a GPU) is replaced by one that records the trainer and raises."""
    from openess_amd.training import openess_trainer as ot
    ot.reached = []

    def base_init(self, settings, train=True):
        ot.reached.append(self)
        raise Reached()

    def boom(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(ot.BaseTrainer, '__init__', base_init)
    monkeypatch.setattr(ot, 'deeplabv3_resnet50', boom)
    yield ot
    del ot.reached


def test_shipped_fp32_yaml_differs_from_the_bf16_one_by_the_keys_alone():
    fp32, bf16 = yaml.load(open(CFG_FP32), yaml.Loader), yaml.load(open(CFG), yaml.Loader)
    assert fp32['clip'].pop('train_precision') == 'fp32' and fp32['clip'].pop('eval_precision') == 'fp32'
    assert fp32 == bf16


def test_shipped_fp32_yaml_loads_and_dispatches_to_the_joint_trainer(no_models):
    import train
    from openess_amd.config.settings import Settings
    s = Settings(CFG_FP32, generate_log=False)
    assert s.train_precision == 'fp32' and s.eval_precision == 'fp32' and s.config_option == 'frame2recon'
    with pytest.raises(Reached):                                              # nothing refused fp32
        train.build_trainer(s)
    (tr,) = no_models.reached
    assert type(tr) is no_models.OpenESSModel and (tr.train_precision, tr.eval_precision) == ('fp32', 'fp32')


def test_bad_key_values_are_refused_at_construction(tmp_path, no_models):
    for key in ('train_precision', 'eval_precision'):
        s = _settings(tmp_path)
        setattr(s, key, 'half')                       # a value set past the YAML check is refused by the trainer as well
        with pytest.raises(ValueError, match=key):
            no_models.OpenESSModel(settings=s)
        for bad in ('fp16', 'FP32', 32):
            with pytest.raises(ValueError, match=key):
                _settings(tmp_path, **{key: bad})
    assert no_models.reached == []                    # every refusal came before the base constructor


@pytest.mark.parametrize("train_precision,eval_precision", [(None, None), ('bf16', 'bf16'), ('fp32', 'bf16'), ('bf16', 'fp32'),
                                                            ('fp32', 'fp32')])
def test_keys_land_on_the_trainer(tmp_path, no_models, train_precision, eval_precision):
    keys = {k: v for k, v in (('train_precision', train_precision), ('eval_precision', eval_precision)) if v is not None}
    with pytest.raises(Reached):
        no_models.OpenESSModel(settings=_settings(tmp_path, **keys))
    (tr,) = no_models.reached
    want = (train_precision or 'bf16', eval_precision or 'bf16')               # a YAML without the keys keeps bf16
    assert (tr.train_precision, tr.eval_precision) == want
    assert tr._step_precision(None) == want[0] and tr._step_precision('fp32') == 'fp32' and tr._step_precision('bf16') == 'bf16'
    with pytest.raises(ValueError, match="precision"):
        tr._step_precision('fp16')
    tr.two_streams = True
    assert tr._step_precision('bf16') == 'bf16'
    with pytest.raises(NotImplementedError, match="two_streams"):
        tr._step_precision('fp32')
