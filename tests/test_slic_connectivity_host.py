"""Host-side checks of SLIC's connectivity pass (K24): the three statements of tests/slic_connectivity_reference.py agree on
every test map and give the answers written down for the hand-made ones, no SLIC test map has a component of max_size pixels
(the condition under which the GPU pass, which makes no cut, equals the loop with it), the sizes rule, the wrappers' refusals
before the library is loaded, the settings key and the shipped YAML.  No GPU."""
import os

import numpy as np
import pytest
import torch
import yaml

from tests import slic_connectivity_cases as cc
from tests import slic_connectivity_reference as cref

CFG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")
ONLINE = "pretrain_dsec_synthetic_online_slic.yaml"
CONNECTED = "pretrain_dsec_synthetic_online_slic_connected.yaml"


# ------------------------------------------------------------------------------------------------------------ the statements
def test_case_lists():
    assert len(cc.A_NAMES) == 24 and [c.name for c in cc.slic_label_cases()] == cc.A_NAMES
    assert [c.name for c in cc.hand_made()] == cc.B_NAMES
    for name in cc.ALL_NAMES:
        c = cc.get(name)
        assert c.maps.dtype == np.int64 and c.maps.ndim == 3 and c.maps.shape[0] == 2
        assert not np.array_equal(c.maps[0], c.maps[1]), name                 # two different maps: a leak between samples shows
        assert 1 <= c.bound and c.min_size >= 0


@pytest.mark.parametrize("name", [n for n in cc.B_NAMES if cc.get(n).expected is not None])
def test_hand_made_maps_have_their_written_down_answers(name):
    c = cc.get(name)
    for m, want in zip(c.maps, c.expected):
        got, n = cref.enforce_sequential(m, c.min_size, c.max_size)
        assert np.array_equal(got, want)
        assert n == (int(want.max()) + 1 if name != "all-different-min5" else 0)


def test_written_down_answers_separate_the_rules():
    """The cases are only worth something if a plausible wrong rule fails them."""
    c = cc.get("last-seen")
    assert c.expected[0][20, 25] == 2 and c.expected[1][20, 25] == 1          # last seen: C, B; first seen would be D = 3 in both
    c = cc.get("corner-no-donor")
    for m, e in zip(c.maps, c.expected):
        assert e[0, 0] == 0 and m[0, 0] == 2 and e.max() == 1
    assert c.expected[0][2, 0] == 1 and c.expected[1][2, 0] == 1              # the corner's lower neighbour ends up as 1, the corner as 0
    c = cc.get("chain-of-two")
    assert c.expected[0][10, 1] == 1 and c.expected[0][10, 2] == 2 and c.expected[1][10, 31] == 1 and c.expected[1][10, 32] == 2
    c = cc.get("labels-2^40")
    assert int(c.maps.min()) >= 5 and len(np.unique(c.maps[1] & 0xffffffff)) == 1 and len(np.unique(c.maps[1])) == 2
    ref, counts = cc.reference("labels-2^40")
    assert counts[1] > 1                                                      # labels equal in their low 32 bits are still two labels


@pytest.mark.parametrize("name", cc.A_NAMES + cc.B_NAMES)
def test_the_three_statements_agree(name):
    c = cc.get(name)
    ref, counts = cc.reference(name)                                          # the loop without the cut
    for i, m in enumerate(c.maps):
        cut, n_cut = cref.enforce_sequential(m, c.min_size, c.max_size)
        free, n_free = cref.enforce_order_free(m, c.min_size)
        assert np.array_equal(cut, ref[i]) and np.array_equal(free, ref[i]) and n_cut == n_free == counts[i]
        assert 0 <= int(ref[i].min()) and int(ref[i].max()) < c.bound and counts[i] <= c.bound


@pytest.mark.parametrize("name", cc.A_NAMES)
def test_no_slic_map_reaches_max_size(name):
    c = cc.get(name)
    _, H, W = c.maps.shape
    for m in c.maps:
        assert cref.largest_component(m) < c.max_size
    if name == "checker-37x53-n6-it1" or name == "checker-37x53-n6-it10":
        assert c.max_size == 1470


def test_slic_maps_do_have_fragments():
    """What the pass is for: the checker case at 110 x 160, K = 96 has hundreds of components below min_size."""
    c = cc.get("checker-110x160-n100-it10")
    small = [sum(1 for v in cref.components(m)[1].values() if v < c.min_size) for m in c.maps]
    assert max(small) > 500, small


def test_oversize_case_has_components_above_max_size():
    c = cc.get(cc.C_NAME)
    assert (c.min_size, c.max_size) == (128, 768)
    ref, counts = cc.reference(cc.C_NAME)
    for i, m in enumerate(c.maps):
        assert cref.largest_component(m) >= c.max_size
        free, n = cref.enforce_order_free(m, c.min_size)
        assert np.array_equal(free, ref[i]) and n == counts[i]
        assert not np.array_equal(cref.enforce_sequential(m, c.min_size, c.max_size)[0], ref[i])       # the cut does change these


# ------------------------------------------------------------------------------------------------------------------ wrappers
def test_sizes_rule():
    from openess_amd import hip
    want = {(40, 56, 8): (140, 840, 16), (37, 53, 4): (245, 1470, 8), (64, 64, 256): (8, 48, 512), (110, 160, 96): (91, 550, 193)}
    for (H, W, K), v in want.items():
        assert hip.slic_connectivity_sizes(H, W, K) == v == cc.sizes(H, W, K)
    assert hip.slic_connectivity_sizes(440, 640, 96) == (1466, 8800, 192)
    assert hip.slic_connectivity_sizes(4, 4, 256) == (0, 0, 16)               # min_size 0: bound is H W
    for bad in ((0, 5, 1), (5, 0, 1), (5, 5, 0)):
        with pytest.raises(ValueError):
            hip.slic_connectivity_sizes(*bad)


def test_wrapper_refuses_before_the_library_is_loaded(monkeypatch):
    from openess_amd import _lib, hip

    def boom():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(_lib, 'load', boom)
    ok = torch.zeros(2, 37, 53, dtype=torch.int64)
    for fn in (hip.slic_enforce_connectivity, hip.slic_connectivity_phase_ms):
        for bad in (ok.int(), ok.float(), ok[0], ok[None], ok.transpose(1, 2), ok[:, :, ::2], torch.zeros(0, 4, 4, dtype=torch.int64),
                    torch.zeros(1, 0, 4, dtype=torch.int64), None):
            with pytest.raises(ValueError, match="labels"):
                fn(bad, 5)
        for bad in (-1, 2.5, None, "3", True, 1 << 31):
            with pytest.raises(ValueError, match="min_size"):
                fn(ok, bad)
    with pytest.raises(ValueError, match="2\\^24"):
        hip.slic_enforce_connectivity(torch.empty(1, 4096, 4097, dtype=torch.int64), 5)      # never touched
    with pytest.raises(ValueError, match="alias"):
        hip.slic_enforce_connectivity(ok, 5, out=ok)
    both = torch.zeros(3, 37, 53, dtype=torch.int64)
    with pytest.raises(ValueError, match="alias"):
        hip.slic_enforce_connectivity(both[:2], 5, out=both[1:])              # overlapping views of one buffer
    for bad in (ok.int(), torch.zeros(2, 37, 52, dtype=torch.int64), torch.zeros(2, 53, 37, dtype=torch.int64).transpose(1, 2)):
        with pytest.raises(ValueError, match="out must be"):
            hip.slic_enforce_connectivity(ok, 5, out=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                # a CPU tensor never reaches a kernel
        hip.slic_enforce_connectivity(ok, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.slic_enforce_connectivity(ok, 5, out=torch.zeros_like(ok))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                # disjoint halves of one buffer do not alias
        hip.slic_enforce_connectivity(both[:1], 5, out=both[2:])


def test_entry_points_validate_arguments_on_the_host():
    import ctypes
    from openess_amd import _lib
    lib = _lib.load()
    assert lib.oess_abi_version() == 13 == _lib.ABI_VERSION                   # additions only
    need, run, timed = lib.oess_slic_connectivity_workspace_bytes, lib.oess_slic_connectivity_i64, lib.oess_slic_connectivity_phase_ms
    assert need(2, 37, 53) == (2 * 1961 * 5 + 2 * 8 + 2) * 4 and need(1, 256, 1) == (256 * 5 + 1 + 1) * 4
    assert need(0, 4, 4) == 0 and need(1, 4096, 4097) == 0 and need(1, 4096, 4096) == ((1 << 24) * 5 + (1 << 16) + 1) * 4
    mem = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(mem) + 63) & ~63
    other = base + 2048
    big = 1 << 40
    assert run(None, 1, 4, 4, 2, other, None, base, big, None) == -22
    assert run(base, 1, 4, 4, 2, None, None, base, big, None) == -22
    assert run(base, 1, 4, 4, 2, other, None, None, big, None) == -22
    assert run(base, 1, 4, 4, 2, base, None, other, big, None) == -22         # out == labels
    assert run(base, 1, 4, 4, -1, other, None, base, big, None) == -22        # min_size < 0
    assert run(base, 1, 4096, 4097, 2, other, None, base, big, None) == -22   # more than 2^24 pixels
    for B, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert run(base, B, H, W, 2, other, None, base, big, None) == -22
    assert run(base, 1, 4, 4, 2, other, None, base + 2, big, None) == -22     # workspace off 4 bytes
    assert run(base, 1, 4, 4, 2, other, None, base, need(1, 4, 4) - 1, None) == -12
    assert run(base, 2, 37, 53, 2, other, None, base, need(1, 37, 53), None) == -12
    ms = (ctypes.c_float * 5)()
    assert timed(base, 1, 4, 4, 2, other, base, big, None, None) == -22
    assert timed(base, 1, 4, 4, 2, base, other, big, ms, None) == -22
    assert timed(base, 1, 4, 4, 2, other, base, 8, ms, None) == -12


# ------------------------------------------------------------------------------------------------------------------ trainers
def _settings(tmp_path, name=CONNECTED, **clip):
    from openess_amd.config.settings import Settings
    cfg = yaml.load(open(os.path.join(CFG_DIR, name)), yaml.Loader)
    cfg['clip'].update(clip)
    path = tmp_path / "settings.yaml"
    path.write_text(yaml.dump(cfg))
    return Settings(str(path), generate_log=False)


@pytest.fixture
def nothing_built(monkeypatch):
    """init_fn (models, optimisers) and the loaders raise: a refusal that still passes came before anything was built."""
    from openess_amd.training import base_trainer_ov as bt

    def boom(*a, **k):
        raise AssertionError("something was built before the refusal")
    monkeypatch.setattr(bt.BaseTrainer, 'init_fn', boom)
    monkeypatch.setattr(bt.BaseTrainer, 'createDataLoaders', boom)
    monkeypatch.setattr(bt.MetricsSemseg, '__init__', boom)


def test_settings_key(tmp_path):
    from openess_amd.config.settings import Settings
    assert Settings(os.path.join(CFG_DIR, ONLINE), generate_log=False).online_slic_connectivity is False        # the default
    assert Settings(os.path.join(CFG_DIR, "pretrain_dsec_synthetic.yaml"), generate_log=False).online_slic_connectivity is False
    s = _settings(tmp_path)
    assert s.online_slic_connectivity is True and s.online_slic_segments == 12 and s.superpixel_sources == 'online_slic'
    assert _settings(tmp_path, online_slic_connectivity=False).online_slic_connectivity is False


def test_constructor_refuses_the_key_without_online_slic(tmp_path, nothing_built):
    from openess_amd.training.base_trainer_ov import online_slic_segments
    from openess_amd.training.openess_trainer import OpenESSModel
    from openess_amd.training.pretrain_trainer import OpenESSPretrainModel
    for source in ('sp_slic_rgb', 'sp_sam_rgb', ''):
        with pytest.raises(ValueError, match="online_slic_connectivity.*superpixel_sources: online_slic"):
            OpenESSPretrainModel(settings=_settings(tmp_path, superpixel_sources=source))
        with pytest.raises(ValueError, match="online_slic_connectivity"):
            OpenESSModel(settings=_settings(tmp_path, superpixel_sources=source, config_option='frame2recon'))
        assert online_slic_segments(_settings(tmp_path, superpixel_sources=source, online_slic_connectivity=False), 25) is None
    # what is served gets past the refusals (to the GPU check on this box, or to the patched first constructor on a GPU box)
    with pytest.raises((AssertionError, RuntimeError), match="before the refusal|need the GPU"):
        OpenESSPretrainModel(settings=_settings(tmp_path))


def test_rows_are_the_bound_and_the_bound_is_refused_against_the_pooling_size():
    from openess_amd.training.base_trainer_ov import online_slic_rows
    assert online_slic_rows(64, 96, 12, 25, False) == 8 and online_slic_rows(64, 96, 12, 25, True) == 16
    assert online_slic_rows(64, 96, 25, 25, False) == 24                      # 24 centres fit 25 rows, their 48 labels do not
    with pytest.raises(ValueError, match="48 labels.*pooling size 25.*online_slic_segments must be about half the pooling size"):
        online_slic_rows(64, 96, 25, 25, True)
    assert online_slic_rows(64, 96, 25, 48, True) == 48
    with pytest.raises(ValueError, match="24 centres.*pooling size 23"):
        online_slic_rows(64, 96, 25, 23, False)
    assert online_slic_rows(440, 640, 100, 192, True) == 192
    with pytest.raises(ValueError, match="96 centres.*192 labels.*pooling size 100"):
        online_slic_rows(440, 640, 100, 100, True)


def test_prepare_batch_refuses_before_any_launch(tmp_path, monkeypatch):
    """BaseTrainer.prepare_batch on a trainer that was never constructed (no GPU here): with the key set and more segments
    than half the pooling size the refusal comes before SLIC is called."""
    from openess_amd import hip
    from openess_amd.training import base_trainer_ov as bt

    def boom(*a, **k):
        raise AssertionError("SLIC was launched before the refusal")
    monkeypatch.setattr(hip, 'slic_superpixels', boom)
    monkeypatch.setattr(hip, 'h2d_async', lambda t, device: t)
    tr = object.__new__(bt.BaseTrainer)
    tr.settings = _settings(tmp_path, online_slic_segments=25)
    tr.online_slic_segments = bt.online_slic_segments(tr.settings, 25)
    tr.device, tr._png_pending, tr._png_batches, tr._voxel_ds = torch.device('cpu'), [], 0, {'train': None}
    host = (torch.zeros(2, 15, 64, 96), None, torch.zeros(2, 3, 64, 96), torch.zeros(2, 64, 96, dtype=torch.int64),
            torch.ones(2, 64, 96, dtype=torch.int64), None, None)             # collate's 7 slots: frame in 2, superpixels in 4
    with pytest.raises(ValueError, match="48 labels.*pooling size 25"):
        tr.prepare_batch(host, 'train')
    tr.settings.online_slic_segments = tr.online_slic_segments = 12
    with pytest.raises(AssertionError, match="SLIC was launched"):            # 16 labels fit: the call goes on to SLIC
        tr.prepare_batch(host, 'train')


def test_shipped_yaml_differs_from_the_online_slic_one_by_the_key_and_the_segments():
    new = yaml.load(open(os.path.join(CFG_DIR, CONNECTED)), yaml.Loader)
    old = yaml.load(open(os.path.join(CFG_DIR, ONLINE)), yaml.Loader)
    assert new['clip'].pop('online_slic_connectivity') is True and new['clip'].pop('online_slic_segments') == 12
    assert 'online_slic_connectivity' not in old['clip'] and 'online_slic_segments' not in old['clip']
    assert new == old and new['clip']['superpixel_sources'] == 'online_slic' and new['clip']['superpixel_size'] == 25
    from openess_amd import hip
    ny, nx, _ = hip.slic_lattice(64, 96, 12)
    assert hip.slic_connectivity_sizes(64, 96, ny * nx)[2] == 16 <= 25
