"""Host side of K31 (no GPU): the settings key of the shipped YAML, the new C entry in the header, the binding and the library, its
refusals (they return before any launch), the wrapper's refusal of a CPU tensor, and PretrainStep's keyword-only options."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "configs")


def test_settings_expose_the_key_of_the_shipped_yaml():
    from openess_amd.config.settings import Settings
    s = Settings(os.path.join(CFG, "pretrain_dsec_synthetic_switchable.yaml"), generate_log=False)
    assert s.if_switchable_train is True and s.if_finetuning is False and s.if_pretraining is True
    assert Settings(os.path.join(CFG, "pretrain_dsec_synthetic.yaml"), generate_log=False).if_switchable_train is False
    new = yaml.load(open(os.path.join(CFG, "pretrain_dsec_synthetic_switchable.yaml")), yaml.Loader)
    old = yaml.load(open(os.path.join(CFG, "pretrain_dsec_synthetic.yaml")), yaml.Loader)
    assert new['clip'].pop('if_switchable_train') is True and old['clip'].pop('if_switchable_train') is False
    assert new == old                                                     # the two differ by the key alone


def test_entry_is_declared_bound_and_exported():
    from openess_amd import _lib
    header = open(os.path.join(ROOT, "include", "oess.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int\s+oess_argmax_labels\s*\(([^)]*)\)", code)
    assert m and len(m.group(1).split(',')) == 12
    res, args = _lib.SIGNATURES["oess_argmax_labels"]
    assert res is ctypes.c_int and len(args) == 12 and args[2] is ctypes.c_longlong
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "oess_argmax_labels")
    lib = _lib.load()
    assert lib.oess_argmax_labels.argtypes == args
    assert lib.oess_abi_version() == 13 == _lib.ABI_VERSION and int(re.search(r"#define\s+OESS_ABI_VERSION\s+(\d+)", header).group(1)) == 13
    assert lib.oess_conv2d_route_count() == 24


def test_entry_refuses_on_the_host():
    """every refusal returns before the first HIP call: the pointers are never read"""
    from openess_amd import _lib
    f = _lib.load().oess_argmax_labels
    ok = dict(logits=4096, bf16=0, ps=11, B=2, K=11, h=3, w=4, H=6, W=8, ac=0, out=8192)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['logits'], a['bf16'], a['ps'], a['B'], a['K'], a['h'], a['w'], a['H'], a['W'], a['ac'], a['out'], None)
    for bad in (dict(logits=None), dict(out=None), dict(K=0), dict(K=257, ps=257), dict(B=0), dict(h=0), dict(w=-1), dict(H=0), dict(W=-2),
                dict(ps=10), dict(B=1 << 16, H=1 << 16), dict(B=1 << 16, h=1 << 16), dict(ps=1 << 62),
                dict(B=1 << 15, H=1 << 15, W=(1 << 31) - 1)):
        assert call(**bad) == -22, bad


def test_wrapper_refuses_a_cpu_tensor():
    from openess_amd import hip
    with pytest.raises(ValueError, match="no CPU fallback"):
        hip.argmax_labels(torch.zeros(1, 3, 2, 2))
    with pytest.raises(ValueError, match="no CPU fallback"):
        hip.argmax_labels(None)


def test_step_options_are_keyword_only_and_default_to_off():
    from openess_amd.training.pretrain_step import PretrainStep
    sig = inspect.signature(PretrainStep.__init__, follow_wrapped=False)
    for name, default in (('online_labels', None), ('switchable_train', False), ('switch_epoch', 5)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default == default
    kw = dict(img_size=(32, 48), nr_events_data=2, device='cpu')
    st = PretrainStep(**kw)
    assert (st.online_labels, st.switchable_train, st.switch_epoch, st.epoch_count, st.switched) == (None, False, 5, 0, False)
    st.epoch_count = 9
    assert not st.switched
    st = PretrainStep(switchable_train=True, **kw)
    assert not st.switched
    st.epoch_count = 4
    assert not st.switched
    st.epoch_count = 5
    assert st.switched
    st = PretrainStep(switchable_train=True, switch_epoch=0, online_labels=len, **kw)
    assert st.switched and st.online_labels is len
    with pytest.raises(NotImplementedError, match="no online teacher"):
        PretrainStep(online_labels=len, precision='fp32', **kw)
    with pytest.raises(TypeError):
        PretrainStep(switchable=True, **kw)
