"""Host-side checks of the online SLIC superpixels (K24): the lattice rule, the refusals of the hip.slic_* wrappers and of the
trainers' constructor before anything is built or launched, the datasets under `superpixel_sources: online_slic` (no superpixel
file is looked up), the shipped YAML and the argument checks of the three entry points.  No GPU."""
import os

import pytest
import torch
import yaml

from tests import slic_cases as sc
from tests import slic_reference as ref

CFG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")
CFG = os.path.join(CFG_DIR, "pretrain_dsec_synthetic_online_slic.yaml")


def _settings(tmp_path, name="pretrain_dsec_synthetic_online_slic.yaml", **clip):
    from openess_amd.config.settings import Settings
    cfg = yaml.load(open(os.path.join(CFG_DIR, name)), yaml.Loader)
    cfg['clip'].update(clip)
    path = tmp_path / "settings.yaml"
    path.write_text(yaml.dump(cfg))
    return Settings(str(path), generate_log=False)


# ------------------------------------------------------------------------------------------------------------------ lattice
@pytest.mark.parametrize("H,W,n,ny,nx,step", [(40, 56, 12, 2, 4, 20), (37, 53, 6, 2, 2, 27), (64, 64, 256, 16, 16, 4),
                                              (110, 160, 100, 8, 12, 14), (440, 640, 100, 8, 12, 55), (200, 346, 25, 3, 6, 67)])
def test_lattice_rule(H, W, n, ny, nx, step):
    from openess_amd import hip
    assert hip.slic_lattice(H, W, n) == (ny, nx, step) == ref.lattice(H, W, n)
    if (H, W, n) in sc.EXPECTED_K:
        assert ny * nx == sc.EXPECTED_K[(H, W, n)]
    ys, xs = ref.lattice_pixels(H, W, ny, nx)
    assert ys == [int((i + 0.5) * H / ny) for i in range(ny)] and 0 <= min(ys) and max(ys) < H and max(xs) < W


def test_lattice_never_has_more_centres_than_segments():
    from openess_amd import hip
    for H in (13, 37, 64, 110, 200, 260, 440):
        for W in (13, 53, 96, 160, 346, 640):
            for n in (4, 6, 12, 25, 30, 100, 256):
                if n * min(H, W) < max(H, W):             # s > min(H, W): the max(1, .) of the rule takes over
                    continue
                ny, nx, step = hip.slic_lattice(H, W, n)
                assert 1 <= ny * nx <= n, (H, W, n)
                assert step * ny >= H and step * nx >= W
    with pytest.raises(ValueError):
        hip.slic_lattice(40, 56, 0)


# ------------------------------------------------------------------------------------------------------------------ wrappers
def test_wrappers_refuse_before_any_launch():
    from openess_amd import hip
    ok = torch.zeros(1, 3, 40, 56)
    with pytest.raises(ValueError, match="min\\(H, W\\) >= 13"):
        hip.slic_superpixels(torch.zeros(1, 3, 12, 56), 12)
    with pytest.raises(ValueError, match="min\\(H, W\\) >= 13"):
        hip.slic_lab(torch.zeros(1, 3, 40, 12))
    with pytest.raises(ValueError, match="at most 256"):
        hip.slic_superpixels(torch.zeros(1, 3, 64, 68), 272)              # 16 x 17 = 272 centres
    for sigma in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match="sigma"):
            hip.slic_superpixels(ok, 12, sigma=sigma)
        with pytest.raises(ValueError, match="sigma"):
            hip.slic_lab(ok, sigma=sigma)
    with pytest.raises(ValueError, match="compactness"):
        hip.slic_lab(ok, compactness=0.0)
    with pytest.raises(ValueError, match="iters"):
        hip.slic_superpixels(ok, 12, iters=0)
    for bad in (ok.double(), ok.to(torch.bfloat16), torch.zeros(1, 1, 40, 56), torch.zeros(3, 40, 56)):
        with pytest.raises(ValueError, match="float32 tensor \\[B, 3, H, W\\]"):
            hip.slic_superpixels(bad, 12)
        with pytest.raises(ValueError, match="float32 tensor \\[B, 3, H, W\\]"):
            hip.slic_lab(bad)
    for fn in (lambda: hip.slic_superpixels(ok, 12), lambda: hip.slic_lab(ok), lambda: hip.slic_lab(ok, lattice=(2, 4))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):          # a CPU tensor never reaches a kernel
            fn()


def test_assign_and_update_refuse_before_any_launch():
    from openess_amd import hip
    lab, cen, lbl = torch.zeros(2, 40, 56, 3), torch.zeros(2, 8, 5), torch.zeros(2, 40, 56, dtype=torch.int64)
    with pytest.raises(ValueError, match="lab must be"):
        hip.slic_assign(lab.permute(0, 3, 1, 2), cen, lbl, 20)
    with pytest.raises(ValueError, match="lab must be"):
        hip.slic_update(lab.double(), lbl, cen)
    with pytest.raises(ValueError, match="centers must be"):
        hip.slic_assign(lab, torch.zeros(2, 8, 4), lbl, 20)
    with pytest.raises(ValueError, match="centers must be"):
        hip.slic_update(lab, lbl, torch.zeros(1, 8, 5))
    with pytest.raises(ValueError, match="K <= 256"):
        hip.slic_assign(lab, torch.zeros(2, 257, 5), lbl, 20)
    with pytest.raises(ValueError, match="prev_labels must be"):
        hip.slic_assign(lab, cen, lbl.int(), 20)
    with pytest.raises(ValueError, match="labels must be"):
        hip.slic_update(lab, lbl[:, :39], cen)
    with pytest.raises(ValueError, match="step"):
        hip.slic_assign(lab, cen, lbl, 0)
    with pytest.raises(ValueError, match="lattice"):
        hip.slic_assign(lab, cen, None, 20)
    with pytest.raises(ValueError, match="lattice"):
        hip.slic_assign(lab, cen, None, 20, lattice=(3, 3))
    for fn in (lambda: hip.slic_assign(lab, cen, lbl, 20), lambda: hip.slic_assign(lab, cen, None, 20, lattice=(2, 4)),
               lambda: hip.slic_update(lab, lbl, cen)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()


def test_entry_points_validate_arguments_on_the_host():
    import ctypes
    from openess_amd import _lib
    lib = _lib.load()
    assert lib.oess_abi_version() == 13 == _lib.ABI_VERSION                # additions only
    mem = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(mem) + 63) & ~63
    view = _lib.F32View(base, 3 * 40 * 56, 56, 1, 40 * 56)
    v = ctypes.byref(view)
    lab_fn, asg, upd = lib.oess_slic_lab_f32, lib.oess_slic_assign_f32, lib.oess_slic_update_f32
    assert lab_fn(None, 1, 40, 56, 3.0, 6.0, base, 0, 0, None, None) == -22
    assert lab_fn(v, 1, 40, 56, 3.0, 6.0, None, 0, 0, None, None) == -22
    assert lab_fn(v, 1, 40, 56, 0.0, 6.0, base, 0, 0, None, None) == -22                 # sigma <= 0
    assert lab_fn(v, 1, 40, 56, 7.0, 6.0, base, 0, 0, None, None) == -22                 # radius beyond the LDS tile
    assert lab_fn(v, 1, 40, 56, 3.0, 0.0, base, 0, 0, None, None) == -22                 # compactness <= 0
    assert lab_fn(v, 1, 12, 56, 3.0, 6.0, base, 0, 0, None, None) == -22                 # min(H, W) < 13
    assert lab_fn(v, 1, 40, 12, 3.0, 6.0, base, 0, 0, None, None) == -22
    assert lab_fn(v, 1, 4096, 4097, 3.0, 6.0, base, 0, 0, None, None) == -22             # more than 2^24 pixels
    assert lab_fn(v, 1, 64, 68, 3.0, 6.0, base, 16, 17, base, None) == -22               # K = 272
    assert lab_fn(v, 1, 40, 56, 3.0, 6.0, base, 0, 4, base, None) == -22
    assert asg(None, base, base, 1, 40, 56, 8, 20, 0, 0, base, None) == -22
    assert asg(base, base, base, 1, 40, 56, 257, 20, 0, 0, base, None) == -22            # K > 256
    assert asg(base, base, base, 1, 40, 56, 0, 20, 0, 0, base, None) == -22
    assert asg(base, base, base, 1, 40, 56, 8, 0, 0, 0, base, None) == -22               # step < 1
    assert asg(base, base, None, 1, 40, 56, 8, 20, 3, 3, base, None) == -22              # no previous labels: ny nx must be K
    assert upd(None, base, base, 1, 40, 56, 8, base, None, base, 4096, None) == -22
    assert upd(base, base, base, 1, 40, 56, 257, base, None, base, 1 << 20, None) == -22
    assert upd(base, base, base, 1, 40, 56, 8, base, None, base + 4, 4096, None) == -22        # workspace not 8-byte aligned
    assert upd(base, base, base, 1, 40, 56, 8, base, None, base, 8 * 48 - 1, None) == -12      # workspace too small


# ------------------------------------------------------------------------------------------------------------------ trainers
@pytest.fixture
def nothing_built(monkeypatch):
    """init_fn (models, optimisers) and the loaders raise: a refusal that still passes came before anything was built."""
    from openess_amd.training import base_trainer_ov as bt

    def boom(*a, **k):
        raise AssertionError("something was built before the refusal")
    monkeypatch.setattr(bt.BaseTrainer, 'init_fn', boom)
    monkeypatch.setattr(bt.BaseTrainer, 'createDataLoaders', boom)
    monkeypatch.setattr(bt.MetricsSemseg, '__init__', boom)


def test_constructor_refusals_come_before_anything_is_built(tmp_path, nothing_built):
    from openess_amd.training.openess_trainer import OpenESSModel
    from openess_amd.training.pretrain_trainer import OpenESSPretrainModel
    with pytest.raises(ValueError, match="recon2voxel"):
        OpenESSPretrainModel(settings=_settings(tmp_path, config_option='recon2voxel'))
    with pytest.raises(ValueError, match="26.*25"):                      # superpixel_size: 25 in the YAML
        OpenESSPretrainModel(settings=_settings(tmp_path, online_slic_segments=26))
    with pytest.raises(ValueError, match="0 .*25"):
        OpenESSPretrainModel(settings=_settings(tmp_path, online_slic_segments=0))
    with pytest.raises(ValueError, match="31.*30"):                      # OpenESSModel pools with its own size, 30
        OpenESSModel(settings=_settings(tmp_path, config_option='frame2recon', superpixel_size=100, online_slic_segments=31))
    # what is served gets past the refusals (to the GPU check on this box, or to the patched first constructor on a GPU box)
    for cls, clip in ((OpenESSPretrainModel, {}), (OpenESSPretrainModel, {'online_slic_segments': 25}),
                      (OpenESSPretrainModel, {'config_option': 'frame2recon', 'online_slic_segments': 12}),
                      (OpenESSModel, {'config_option': 'frame2recon', 'online_slic_segments': 30}),
                      (OpenESSPretrainModel, {'config_option': 'recon2voxel', 'superpixel_sources': 'sp_sam_rgb', 'online_slic_segments': 999})):
        with pytest.raises((AssertionError, RuntimeError), match="before the refusal|need the GPU"):
            cls(settings=_settings(tmp_path, **clip))


def test_segments_default_to_the_pooling_size(tmp_path):
    from openess_amd.training.base_trainer_ov import online_slic_segments
    s = _settings(tmp_path)
    assert s.superpixel_sources == 'online_slic' and s.online_slic_segments is None
    assert online_slic_segments(s, 25) == 25 and online_slic_segments(s, 30) == 30
    assert online_slic_segments(_settings(tmp_path, online_slic_segments=12), 25) == 12
    assert online_slic_segments(_settings(tmp_path, superpixel_sources='sp_slic_rgb'), 25) is None
    assert online_slic_segments(_settings(tmp_path, superpixel_sources=''), 25) is None


def test_shipped_yaml_differs_from_the_bf16_one_by_the_source_alone():
    new = yaml.load(open(CFG), yaml.Loader)
    old = yaml.load(open(os.path.join(CFG_DIR, "pretrain_dsec_synthetic.yaml")), yaml.Loader)
    assert new['clip'].pop('superpixel_sources') == 'online_slic' and old['clip'].pop('superpixel_sources') == 'sp_sam_rgb'
    assert new == old and new['clip']['if_spatial_contrastive'] is True
    from openess_amd.config.settings import Settings, dataset_superpixel_sources
    s = Settings(CFG, generate_log=False)
    assert s.superpixel_sources == 'online_slic' and dataset_superpixel_sources(s) == ''
    s.superpixel_sources = 'sp_slic_rgb'
    assert dataset_superpixel_sources(s) == 'sp_slic_rgb'


# ------------------------------------------------------------------------------------------------------------------ datasets
class _Stop(Exception):
    pass


def _builder_kwargs(monkeypatch, tmp_path, name_b, cls_path):
    """What BaseTrainer.createDataLoaders hands the dataset builder under online_slic (the trainer is not constructed)."""
    import importlib
    from openess_amd.training import base_trainer_ov as bt
    seen = []

    def builder(*a, **kw):
        seen.append(kw)
        if len(seen) == 2:
            raise _Stop
        return object()
    tr = object.__new__(bt.BaseTrainer)
    s = _settings(tmp_path)
    s.dataset_name_b, s.synthetic_data, s.dataset_path_b = name_b, False, str(tmp_path)
    s.split_train_b = 'train'
    tr.settings, tr.world, tr.rank = s, 1, 0
    tr.online_slic_segments = bt.online_slic_segments(s, 25)
    mod, cls = cls_path.rsplit('.', 1)
    monkeypatch.setattr(importlib.import_module(mod), cls, builder)
    with pytest.raises(_Stop):
        tr.createDataLoaders()
    return seen


@pytest.mark.parametrize("name_b,cls_path", [("DSEC_events", "openess_amd.datasets.DSEC_events_loader.DSECEvents"),
                                             ("DDD17_events", "openess_amd.datasets.ddd17_events_loader.DDD17Events")])
def test_dataset_builders_receive_an_empty_source(monkeypatch, tmp_path, name_b, cls_path):
    seen = _builder_kwargs(monkeypatch, tmp_path, name_b, cls_path)
    assert [kw['superpixel_sources'] for kw in seen] == ['', '']


def test_dsec_dataset_under_online_slic_opens_no_superpixel_file(tmp_path):
    """A DSEC tree WITHOUT any superpixel directory: the train dataset built the way the trainer builds it under online_slic
    serves its samples with the ones-map in the superpixel slot; built with a file source it cannot."""
    import glob
    import shutil
    from tests import synth_datasets as sd
    from tests.test_datasets_golden import COMMON
    from openess_amd.config.settings import Settings, dataset_superpixel_sources
    from openess_amd.datasets.DSEC_events_loader import DSECEvents
    root = sd.make_dsec_tree(str(tmp_path / "dsec"))
    dirs = glob.glob(os.path.join(root, "**", "sp_*"), recursive=True)
    assert dirs
    for d in dirs:
        shutil.rmtree(d)
    assert not glob.glob(os.path.join(root, "**", "*sp_*"), recursive=True) and not glob.glob(os.path.join(root, "**", "*slic*"), recursive=True)
    kw = dict(dsec_dir=root, **COMMON, mode='train', config_option='frame2voxel', augmentation=False, fixed_duration=False, skip_ratio=1)
    ds = DSECEvents(superpixel_sources=dataset_superpixel_sources(Settings(CFG, generate_log=False)), **kw)
    for i in (0, len(ds) - 1):
        item = ds[i]
        assert item[4].dtype == torch.int64 and torch.equal(item[4], torch.ones_like(item[1]))
    with pytest.raises(Exception):                                       # the tree really has none
        DSECEvents(superpixel_sources='sp_slic_rgb', **kw)[0]


def test_synthetic_dataset_serves_the_ones_map():
    from openess_amd.datasets.synthetic_events import SyntheticEvents
    kw = dict(length=2, sensor_hw=(72, 96), crop_rows=8, nr_events_data=2, nr_events_window=50, superpixel_size=25)
    grid = SyntheticEvents(**kw)[0]
    ones = SyntheticEvents(superpixel_sources='', **kw)[0]
    assert int(grid[4].max()) == 24 and torch.equal(ones[4], torch.ones(64, 96, dtype=torch.int64))
    for a, b in zip(grid[:4], ones[:4]):                                  # every other slot is untouched
        if isinstance(a, dict):
            assert all(torch.equal(a[k], b[k]) for k in a)
        else:
            assert torch.equal(a, b)
