"""Host-side checks of `recon_sources: online_e2vid`: the settings keys and the trainers' refusals before anything
is built, the shipped YAMLs, the DSEC dataset without a reconstructions/ tree (same `random` draws as the PNG source), collate of
the event slot with and without an arena, the unchanged default path, the entry point's argument checks, and the CPU oracle
against its own float64 form under the share bound the GPU test uses.  No GPU."""
import ctypes
import glob
import os
import random
import shutil

import numpy as np
import pytest
import torch
import yaml

from tests import online_recon_cases as oc

CFG_DIR = oc.CFG
NEW = ("pretrain_dsec_synthetic_frame2recon_online_recon.yaml", "finetune_dsec_synthetic_frame2recon_online_recon.yaml",
       "openess_dsec_synthetic_online_recon.yaml")


def _settings(tmp_path, name=NEW[0], dataset=None, **clip):
    from openess_amd.config.settings import Settings
    cfg = yaml.load(open(os.path.join(CFG_DIR, name)), yaml.Loader)
    cfg['clip'].update(clip)
    if dataset == 'DDD17_events':
        cfg['dataset']['name_b'] = dataset
        cfg['dataset'][dataset] = dict(cfg['dataset']['DSEC_events'], split_train='train')
    path = tmp_path / "settings.yaml"
    path.write_text(yaml.dump(cfg))
    return Settings(str(path), generate_log=False)


# ------------------------------------------------------------------------------------------------------------------ settings
def test_every_yaml_loads_and_the_keys_default_to_the_png_tree():
    from openess_amd.config.settings import Settings
    files = sorted(glob.glob(os.path.join(CFG_DIR, "*.yaml")))
    assert len(files) >= 13 and all(os.path.join(CFG_DIR, n) in files for n in NEW)
    for f in files:
        s = Settings(f, generate_log=False)
        if os.path.basename(f) in NEW:
            assert s.recon_sources == 'online_e2vid' and s.online_recon_model == 'random' and s.online_recon_precision == 'bf16'
            assert s.config_option == 'frame2recon'
        else:
            assert s.recon_sources is None and s.online_recon_precision == 'bf16' and s.online_recon_model == s.path_to_model


@pytest.mark.parametrize("new,old", [(NEW[1], "finetune_dsec_synthetic.yaml"), (NEW[2], "openess_dsec_synthetic.yaml"),
                                     (NEW[0], "pretrain_dsec_synthetic.yaml")])
def test_shipped_yamls_differ_from_their_siblings_by_the_source_alone(new, old):
    a = yaml.load(open(os.path.join(CFG_DIR, new)), yaml.Loader)
    b = yaml.load(open(os.path.join(CFG_DIR, old)), yaml.Loader)
    assert a['clip'].pop('recon_sources') == 'online_e2vid' and a['clip'].pop('online_recon_model') == 'random'
    a['clip'].pop('online_recon_precision', None)
    assert a['clip'].pop('config_option') == 'frame2recon' and b['clip'].pop('config_option') in ('frame2recon', 'frame2voxel')
    assert a == b


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.fixture
def nothing_built(monkeypatch):
    """init_fn (models, optimisers), the loaders and the E2VID of the source raise: a refusal that still passes came first."""
    from openess_amd.training import base_trainer_ov as bt

    def boom(*a, **k):
        raise AssertionError("something was built before the refusal")
    for name in ('init_fn', 'createDataLoaders', 'build_online_recon'):
        monkeypatch.setattr(bt.BaseTrainer, name, boom)
    monkeypatch.setattr(bt.MetricsSemseg, '__init__', boom)


def test_constructor_refusals_name_the_key_and_come_before_anything_is_built(tmp_path, nothing_built):
    from openess_amd.training.finetune_trainer import OpenESSFineTuneModel
    from openess_amd.training.openess_trainer import OpenESSModel
    from openess_amd.training.pretrain_trainer import OpenESSPretrainModel
    for option in ('frame2voxel', 'recon2voxel'):
        with pytest.raises(ValueError, match="recon_sources.*frame2recon"):
            OpenESSPretrainModel(settings=_settings(tmp_path, config_option=option))
    with pytest.raises(ValueError, match="recon_sources.*frame2recon"):
        OpenESSFineTuneModel(settings=_settings(tmp_path, NEW[1], config_option='frame2voxel'))
    with pytest.raises(ValueError, match="recon_sources.*DSEC_events.*DDD17_events"):
        OpenESSPretrainModel(settings=_settings(tmp_path, dataset='DDD17_events'))
    with pytest.raises(ValueError, match="online_recon_precision.*fp16"):
        OpenESSModel(settings=_settings(tmp_path, NEW[2], online_recon_precision='fp16'))
    with pytest.raises(ValueError, match="online_recon_model.*no_such_file"):
        OpenESSPretrainModel(settings=_settings(tmp_path, online_recon_model=str(tmp_path / "no_such_file.pth.tar")))
    s = _settings(tmp_path)
    del s.online_recon_model                      # the default is settings.path_to_model, which does not ship
    s.online_recon_model = s.path_to_model
    with pytest.raises(ValueError, match="online_recon_model"):
        OpenESSPretrainModel(settings=s)
    with pytest.raises(ValueError, match="recon_sources must be"):
        OpenESSPretrainModel(settings=_settings(tmp_path, recon_sources='online_firenet'))
    s = _settings(tmp_path)
    s.e2vid_config.auto_hdr = True
    with pytest.raises(ValueError, match="auto_hdr"):
        OpenESSPretrainModel(settings=s)
    # what is served gets past the refusals: to the GPU check on a box without one, to the patched first constructor with one
    for cls, name, clip in ((OpenESSPretrainModel, NEW[0], {}), (OpenESSFineTuneModel, NEW[1], {'online_recon_precision': 'fp32'}),
                            (OpenESSModel, NEW[2], {})):
        with pytest.raises((AssertionError, RuntimeError), match="before the refusal|need the GPU"):
            cls(settings=_settings(tmp_path, name, **clip))


def test_without_the_key_the_options_are_none(tmp_path):
    from openess_amd.training.base_trainer_ov import online_recon_options
    assert online_recon_options(_settings(tmp_path, "finetune_dsec_synthetic.yaml")) is None
    assert online_recon_options(_settings(tmp_path, "pretrain_dsec_synthetic.yaml")) is None
    assert online_recon_options(_settings(tmp_path)) == {'precision': 'bf16', 'model': 'random'}
    assert online_recon_options(_settings(tmp_path, online_recon_precision='fp32'))['precision'] == 'fp32'


# ------------------------------------------------------------------------------------------------------------------ datasets
def _dsec_kw(root, **kw):
    from tests.test_datasets_golden import COMMON
    return dict(dsec_dir=root, **COMMON, mode='train', config_option='frame2recon', fixed_duration=False, skip_ratio=1,
                superpixel_sources='sp_sam_rgb', **kw)


def test_dsec_dataset_without_a_reconstructions_tree_draws_what_the_png_source_draws(tmp_path):
    from tests import synth_datasets as sd
    from openess_amd.datasets.DSEC_events_loader import DSECEvents
    from openess_amd.datasets import _io
    with_png = sd.make_dsec_tree(str(tmp_path / "png"))
    without = sd.make_dsec_tree(str(tmp_path / "online"))
    dirs = glob.glob(os.path.join(without, "**", "reconstructions"), recursive=True)
    assert len(dirs) == 3
    for d in dirs:
        shutil.rmtree(d)
    assert not glob.glob(os.path.join(without, "**", "reconstructions*"), recursive=True)
    online = DSECEvents(augmentation=True, recon_sources='online_e2vid', **_dsec_kw(without))
    png = DSECEvents(augmentation=True, **_dsec_kw(with_png))
    with pytest.raises(Exception):                                       # the tree really has none
        DSECEvents(augmentation=True, **_dsec_kw(without))[0]
    assert len(online) == len(png) >= 4
    seen = {'flip': set(), 'brightness': set(), 'contrast': set(), 'noise': set()}
    for trial, i in enumerate(list(range(len(online))) * 3):
        # the PNG source with the reference's helpers recording their factors
        rec = []
        orig_b, orig_c = _io.adjust_brightness, _io.adjust_contrast
        _io.adjust_brightness = lambda img, f: (rec.append(('b', f)), orig_b(img, f))[1]
        _io.adjust_contrast = lambda img, f: (rec.append(('c', f)), orig_c(img, f))[1]
        try:
            random.seed(1000 + trial), torch.manual_seed(5 + trial)
            a = png[i]
            state_png = random.getstate()
            rec_png = list(rec)
            del rec[:]
            random.seed(1000 + trial), torch.manual_seed(5 + trial)
            b = online[i]
            state_online = random.getstate()
        finally:
            _io.adjust_brightness, _io.adjust_contrast = orig_b, orig_c
        assert state_png == state_online                                  # the `random` stream is a PNG-source run's
        ev, aug = b[2], b[2]['aug']
        assert set(ev) == {'x', 'y', 't', 'p', 'seg_offsets', 'flip', 'aug', 'sequence'} and ev['flip'] is False
        raw = online.datasets[0].raw_events(0)
        assert ev['x'].dtype == raw['x'].dtype and ev['seg_offsets'].numel() == raw['seg_offsets'].numel()
        # factors: the PNG run calls brightness (recon, frame) then contrast (recon, frame); the online run only the frame's
        want = {'brightness': 1.0, 'contrast': 1.0}
        pairs = {'b': [f for k, f in rec_png if k == 'b'], 'c': [f for k, f in rec_png if k == 'c']}
        frame_only = {'b': [f for k, f in rec if k == 'b'], 'c': [f for k, f in rec if k == 'c']}
        if pairs['b']:
            want['brightness'] = pairs['b'][0]
            assert frame_only['b'] == [pairs['b'][1]]
        if pairs['c']:
            want['contrast'] = pairs['c'][0]
            assert frame_only['c'] == [pairs['c'][1]]
        assert aug['brightness'] == want['brightness'] and aug['contrast'] == want['contrast']
        # label / pseudo-label / superpixel items (flips included) are the PNG run's, so the flip coin agreed
        for slot in (1, 3, 4, 5):
            assert torch.equal(a[slot], b[slot]), slot
        assert a[6] == b[6].replace(without, with_png)
        assert isinstance(aug['flip'], bool) and isinstance(aug['noise_seed'], int) and 0 <= aug['noise_seed'] < 2 ** 62
        seen['flip'].add(aug['flip']), seen['noise'].add(aug['noise_seed'] != 0)
        seen['brightness'].add(aug['brightness'] != 1.0), seen['contrast'].add(aug['contrast'] != 1.0)
        if aug['noise_seed'] == 0 and not pairs['b'] and not pairs['c']:
            assert torch.equal(a[0], b[0])                                # no torch draw at all: the frame is the PNG run's bits
    assert all(v == {False, True} for v in seen.values()), seen           # every coin fell both ways
    # flip: decided by the same coin; recorded for the image, never applied to the events
    random.seed(3)
    flips = [online[0][2]['aug']['flip'] for _ in range(12)]
    random.seed(3)
    labels = [png[0][1] for _ in range(12)]
    plain = png.datasets[0].get_label(png.datasets[0].label_pathstrings[0])
    assert flips == [not torch.equal(l, torch.from_numpy(plain).long()) for l in labels]


def test_validation_dataset_serves_the_event_slot_with_everything_off(tmp_path):
    from tests import synth_datasets as sd
    from openess_amd.datasets.DSEC_events_loader import DSECEvents
    root = sd.make_dsec_tree(str(tmp_path / "dsec"))
    for d in glob.glob(os.path.join(root, "**", "reconstructions"), recursive=True):
        shutil.rmtree(d)
    kw = _dsec_kw(root)
    kw.update(mode='val', superpixel_sources='', skip_ratio=2)
    val = DSECEvents(augmentation=False, recon_sources='online_e2vid', **kw)
    state = random.getstate()
    item = val[0]
    assert random.getstate() == state                                     # no draw
    assert item[2]['aug'] == {'flip': False, 'brightness': 1.0, 'contrast': 1.0, 'noise_seed': 0}
    assert torch.is_tensor(item[0]) and item[0].shape == (3, 440, 640)


def test_synthetic_dataset_event_slot():
    ds_on = oc.dataset((64, 96), augmentation=True, length=8)
    from openess_amd.datasets.synthetic_events import SyntheticEvents
    ds_off = SyntheticEvents(length=8, sensor_hw=(104, 96), crop_rows=40, nr_events_data=oc.NWIN, nr_events_window=oc.NEV,
                             nr_bins=oc.BINS, config_option='frame2recon', superpixel_size=25)
    augs = []
    for i in range(8):
        a, b = ds_off[i], ds_on[i]
        for slot in (0, 1, 3, 4, 5):
            assert torch.equal(a[slot], b[slot])                          # every other slot is what it was
        assert torch.is_tensor(a[2]) and a[2].shape == (3, 64, 96)
        ev = b[2]
        assert ev['seg_offsets'].tolist() == [0, oc.NEV, 2 * oc.NEV, 3 * oc.NEV] and ev['flip'] is False
        assert ev['x'].numel() == oc.NWIN * oc.NEV and ev['t'].dtype == torch.int64
        augs.append(ev['aug'])
    assert any(a['noise_seed'] for a in augs) and any(a['flip'] for a in augs) and any(a['contrast'] != 1.0 for a in augs)
    assert augs == [ds_on[i][2]['aug'] for i in range(8)]                 # a sample's draws are its own
    assert all(oc.dataset((64, 96), mode='val', augmentation=True)[i][2]['aug']['noise_seed'] == 0 for i in range(2))


# ------------------------------------------------------------------------------------------------------------------ collate
def test_collate_of_the_event_slot_with_and_without_an_arena():
    from openess_amd.datasets.ring_loader import Arena, _decode, _encode
    from openess_amd.datasets.synthetic_events import collate
    ds = oc.dataset((44, 60), augmentation=True)
    samples = [ds[i] for i in range(3)]
    plain = collate(samples)
    arena = Arena(torch.empty(32 << 20, dtype=torch.uint8))
    ring = _decode(_encode(collate(samples, arena=arena)), arena.buf)    # what the consumer's side of the ring sees
    for batch in (plain, ring):
        assert len(batch) == 7 and torch.is_tensor(batch[0]) and batch[0].shape == (3, 3, 44, 60)         # slot 0: the frame, as before
        ev = batch[2]
        assert set(ev) == {'x', 'y', 't', 'p', 'events_per_sample', 'seg_offsets', 'flip', 'aug'}
        n = oc.NWIN * oc.NEV
        assert ev['events_per_sample'].tolist() == [n] * 3 and ev['flip'] == [False] * 3
        assert ev['seg_offsets'].tolist() == [oc.NEV * k for k in range(3 * oc.NWIN + 1)]
        for k in ('x', 'y', 't', 'p'):
            assert torch.equal(ev[k], torch.cat([s[2][k] for s in samples]))
        assert ev['aug'] == {k: [s[2]['aug'][k] for s in samples] for k in ('flip', 'brightness', 'contrast', 'noise_seed')}
        assert batch[1].shape == (3, 44, 60) and batch[6] == [s[6] for s in samples]
    lo, hi = arena.buf.data_ptr(), arena.buf.data_ptr() + arena.buf.numel()
    for k in ('x', 'y', 't', 'p'):                                        # the arena path wrote the columns into the slot
        assert lo <= ring[2][k].data_ptr() < hi and not lo <= plain[2][k].data_ptr() < hi


def test_without_the_key_the_tuple_and_the_batch_are_what_they_were(tmp_path):
    from tests import synth_datasets as sd
    from openess_amd.datasets.DSEC_events_loader import DSECEvents
    from openess_amd.datasets.synthetic_events import collate
    root = sd.make_dsec_tree(str(tmp_path / "dsec"))
    default = DSECEvents(augmentation=True, **_dsec_kw(root))
    explicit = DSECEvents(augmentation=True, recon_sources=None, **_dsec_kw(root))
    items = []
    for ds in (default, explicit):
        random.seed(9), torch.manual_seed(9)
        items.append([ds[i] for i in range(2)])
    for a, b in zip(*items):
        assert len(a) == 7 and torch.is_tensor(a[2]) and a[2].shape == (3, 440, 640) and a[2].dtype == torch.float32
        assert all(torch.equal(a[k], b[k]) for k in range(6)) and a[6] == b[6]
    batch = collate(items[0])
    assert len(batch) == 7 and all(torch.is_tensor(batch[k]) for k in range(6)) and batch[2].shape == (2, 3, 440, 640)
    # frame2voxel under the key's dataset argument is untouched too: the key acts on frame2recon alone
    kw = _dsec_kw(root)
    kw['config_option'] = 'frame2voxel'
    random.seed(4), torch.manual_seed(4)
    a = DSECEvents(augmentation=True, **kw)[0]
    random.seed(4), torch.manual_seed(4)
    b = DSECEvents(augmentation=True, recon_sources='online_e2vid', **kw)[0]
    assert isinstance(a[0], dict) and torch.is_tensor(b[2]) and torch.equal(a[2], b[2]) and torch.equal(a[0]['x'], b[0]['x'])


# ------------------------------------------------------------------------------------------------------------------ entry point
def test_entry_point_validates_arguments_on_the_host():
    from openess_amd import _lib
    lib = _lib.load()
    assert lib.oess_abi_version() == 13 == _lib.ABI_VERSION                # additions only
    q = lib.oess_gray_augment_scratch_bytes
    assert q(8, 440, 640) == 8 * 69 * 4 and q(3, 5, 7) == 3 * 4 and q(1, 64, 64) == 4 and q(1, 64, 65) == 8
    assert q(0, 5, 7) == 0 and q(1, 0, 7) == 0 and q(1, 1 << 20, 1 << 20) == 0 and q(1 << 40, 5, 7) == 0
    mem = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(mem) + 63) & ~63
    I, F, U = (ctypes.c_int32 * 2), (ctypes.c_float * 2), (ctypes.c_uint64 * 2)
    flip, one, seed = I(0, 1), F(1.0, 1.0), U(0, 0)
    fn = lib.oess_gray_augment_rgb_f32
    assert fn(None, 2, 5, 7, flip, one, one, seed, base, None, 0, None) == -22
    assert fn(base, 2, 5, 7, flip, one, one, seed, None, None, 0, None) == -22
    for k in range(4):
        cols = [flip, one, one, seed]
        cols[k] = None
        assert fn(base, 2, 5, 7, *cols, base, None, 0, None) == -22
    assert fn(base, 0, 5, 7, flip, one, one, seed, base, None, 0, None) == -22
    assert fn(base, 2, 0, 7, flip, one, one, seed, base, None, 0, None) == -22
    assert fn(base, 2, 32768, 32768, flip, one, one, seed, base, None, 0, None) == -22          # 3 H W >= 2^31
    assert fn(base, 2, 5, 7, flip, one, one, seed, base + 2, None, 0, None) == -22              # out off 4 bytes
    assert fn(base, 2, 5, 7, I(0, 2), one, one, seed, base, None, 0, None) == -22
    assert fn(base, 2, 5, 7, flip, F(1.0, float('nan')), one, seed, base, None, 0, None) == -22
    assert fn(base, 2, 5, 7, flip, one, F(-1.0, 1.0), seed, base, None, 0, None) == -22
    assert fn(base, 2, 5, 7, flip, one, F(float('inf'), 1.0), seed, base, None, 0, None) == -22
    assert fn(base, 2, 5, 7, flip, one, F(0.9, 1.0), seed, base, None, 0, None) == -22          # a blend without scratch
    assert fn(base, 2, 5, 7, flip, one, F(0.9, 1.0), seed, base, base + 2, 64, None) == -22     # scratch off 4 bytes
    assert fn(base, 2, 5, 7, flip, one, F(0.9, 1.0), seed, base, base, 7, None) == -12          # scratch too small


def test_wrapper_refuses_on_the_host():
    from openess_amd import hip
    u8 = torch.zeros(2, 5, 7, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU tensor"):
        hip.recon_augment(u8, [0, 0], [1.0, 1.0], [1.0, 1.0], [0, 0])
    with pytest.raises(ValueError, match="uint8"):
        hip.recon_augment(u8.float(), [0, 0], [1.0, 1.0], [1.0, 1.0], [0, 0])


# ------------------------------------------------------------------------------------------------------------------ the oracle's own error
@pytest.mark.parametrize("hw", oc.SIZES)
def test_cpu_oracle_in_fp32_stays_inside_the_share_bound(hw):
    """The yardstick of tests/test_hip_online_recon.py (b): torch fp32 against float64 on the same case differs on at most
    share_bound(hw) of the pixels and by at most one grey level (tools/exp_recon_augment_bounds.py prints the same figures)."""
    model = oc.oracle_model(oc.filled_state_dict())
    batch, ds = oc.host_batch(hw)
    vox = oc.oracle_voxels(batch[2], ds)
    assert vox.shape == (oc.B, oc.NWIN * oc.BINS) + tuple(hw)
    a = oc.post_cpu(oc.oracle_image(vox, model, hw, torch.float32)).numpy().astype(np.int64)
    b = oc.post_cpu(oc.oracle_image(vox, model, hw, torch.float64)).numpy().astype(np.int64)
    assert a.shape == (oc.B,) + tuple(hw) and len(np.unique(b)) > 64      # a real image, not a saturated one
    assert np.abs(a - b).max() <= 1 and float((a != b).mean()) <= oc.share_bound(hw)
