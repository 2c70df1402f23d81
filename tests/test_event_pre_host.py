"""Host-side checks of EventPreprocessor's hot-pixel removal and flip: the hot-pixel file, the mask and its cache,
the new C symbols (header, binding, export, ABI 13) and their argument checks, the refusals of the hip wrappers before the
library is called, the CLI flags, the online-recon refusal of `flip`, and the float64 restatement against the fixture that the
reference's own EventPreprocessor produced (tests/golden/gen_golden_e2vid_hotflip.py).  No GPU."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import event_pre_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("oess_masked_stats_slice_pre_f32", "oess_masked_stats_slices_pre_f32", "oess_masked_normalize_slice_pre_f32",
               "oess_event_slice_to_nhwc8_pre_bf16", "oess_e2vid_events_head_enc0_pre_bf16")


def _pre(**kw):
    from openess_amd.e2vid.utils.inference_utils import EventPreprocessor
    return EventPreprocessor(SimpleNamespace(**kw))


# ------------------------------------------------------------------------------------------------------------------ the file
def test_hot_pixel_file_rows(tmp_path, capsys):
    from openess_amd.e2vid.utils.inference_utils import load_hot_pixels
    one = tmp_path / "one.txt"
    one.write_text("3,5\n")
    assert load_hot_pixels(str(one)).tolist() == [[3, 5]]                 # a single row (the reference's loop breaks on it)
    many = tmp_path / "many.txt"
    many.write_text("0,0\n19,11\n3,5\n3,5\n")
    rows = load_hot_pixels(str(many))
    assert rows.dtype == np.int64 and rows.tolist() == [[0, 0], [19, 11], [3, 5], [3, 5]]
    assert "Will remove 4 hot pixels" in capsys.readouterr().out
    assert load_hot_pixels(str(tmp_path / "absent.txt")).shape == (0, 2)
    assert "WARNING: could not load hot pixels file: " + str(tmp_path / "absent.txt") in capsys.readouterr().out


def test_constructor_reads_both_options(tmp_path, capsys):
    """The parent raised NotImplementedError for either option."""
    f = tmp_path / "hot.txt"
    f.write_text("0,0\n19,11\n3,5\n3,5\n")
    p = _pre(hot_pixels_file=str(f), flip=True, no_normalize=False)
    assert p.flip and len(p.hot_pixel_locations) == 4 and not p.no_normalize
    assert "Will flip event tensors." in capsys.readouterr().out
    q = _pre(hot_pixels_file=str(tmp_path / "absent.txt"))                # warning, nothing removed, no options left
    assert len(q.hot_pixel_locations) == 0 and q.pre_for(torch.zeros(1, 5, 12, 20)) is None
    assert _pre().pre_for(torch.zeros(1, 5, 12, 20)) is None and _pre(flip=False, hot_pixels_file=None).flip is False


def test_mask_is_built_once_per_size_and_out_of_range_rows_are_named(tmp_path):
    f = tmp_path / "hot.txt"
    f.write_text("0,0\n19,11\n3,5\n3,5\n")
    p = _pre(hot_pixels_file=str(f), flip=True)
    a = p.pre_for(torch.zeros(2, 5, 12, 20))
    assert a.flip and a.hot_mask.dtype == torch.uint8 and tuple(a.hot_mask.shape) == (12, 20)
    assert np.array_equal(a.hot_mask.numpy(), ec.mask_from_rows([[0, 0], [19, 11], [3, 5]], 12, 20)) and int(a.hot_mask.sum()) == 3
    assert p.pre_for(torch.zeros(1, 15, 12, 20)) is a                     # same (H, W, device): the cached object
    b = p.pre_for(torch.zeros(1, 5, 13, 21))
    assert b is not a and tuple(b.hot_mask.shape) == (13, 21) and p.pre_for(torch.zeros(3, 5, 13, 21)) is b
    with pytest.raises(ValueError, match=r"row 2 \(x=19, y=11\)"):        # raised when the mask is first built for that size
        p.pre_for(torch.zeros(1, 5, 11, 20))
    g = tmp_path / "neg.txt"
    g.write_text("2,2\n-1,3\n")
    with pytest.raises(ValueError, match=r"row 2 \(x=-1, y=3\)"):
        _pre(hot_pixels_file=str(g)).pre_for(torch.zeros(1, 5, 12, 20))
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):            # the options are never dropped silently
        p.pre_for(torch.zeros(5, 12, 20))
    flip_only = _pre(flip=True).pre_for(torch.zeros(1, 5, 12, 20))
    assert flip_only.hot_mask is None and flip_only.flip


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_new_symbols_are_declared_bound_and_exported_under_abi_13():
    from openess_amd import _lib
    header = open(os.path.join(ROOT, "include", "oess.h")).read()
    assert int(re.search(r"#define\s+OESS_ABI_VERSION\s+(\d+)", header).group(1)) == 13 == _lib.ABI_VERSION
    assert "oess_event_pre_t" in header and [f[0] for f in _lib.EventPre._fields_] == ["hot_mask", "flip"]
    lib = _lib.load()
    assert lib.oess_abi_version() == 13
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, header) and n in _lib.SIGNATURES and hasattr(lib, n)
        assert _lib.SIGNATURES[n][1].count(_lib.c_pre) == 1


def test_new_entry_points_validate_arguments_on_the_host():
    from openess_amd import _lib
    lib = _lib.load()
    pre = _lib.EventPre(None, 1)
    p = ctypes.byref(pre)
    assert lib.oess_masked_stats_slice_pre_f32(None, 2, 15, 0, 5, 12, 20, p, None, None) == -22
    assert lib.oess_masked_stats_slice_pre_f32(None, 2, 15, 0, 5, 12, 20, None, None, None) == -22          # pre must not be null
    assert lib.oess_masked_stats_slices_pre_f32(None, 2, 15, 5, 3, 12, 20, p, None, None) == -22
    assert lib.oess_masked_stats_slices_pre_f32(None, 2, 15, 5, 3, 0, 20, p, None, None) == -22
    assert lib.oess_masked_normalize_slice_pre_f32(None, None, 2, 15, 0, 5, 12, 20, p, 1, None, None) == -22
    assert lib.oess_event_slice_to_nhwc8_pre_bf16(None, 2, 15, 0, 5, 12, 20, p, None, 0, None, None) == -22
    assert lib.oess_e2vid_events_head_enc0_pre_bf16(None, 2, 15, 0, 5, 32, 48, p, None, 0, None, None, 1, None, None, 1, None, 64,
                                                    None) == -22


# ------------------------------------------------------------------------------------------------------------------ hip wrappers
def test_event_pre_holder_and_wrapper_refusals_come_before_the_library():
    from openess_amd import hip
    with pytest.raises(ValueError, match="uint8"):
        hip.EventPre(torch.zeros(12, 20, dtype=torch.float32))
    with pytest.raises(ValueError, match="uint8"):
        hip.EventPre(np.zeros((12, 20), np.uint8))
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        hip.EventPre(torch.zeros(1, 12, 20, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        hip.EventPre(torch.zeros(12, 40, dtype=torch.uint8)[:, ::2])
    assert hip.EventPre().hot_mask is None and hip.EventPre().flip is False and hip.EventPre(flip=1).flip is True
    ev = torch.zeros(2, 15, 12, 20)
    other = hip.EventPre(torch.zeros(20, 12, dtype=torch.uint8))          # a mask for another H x W
    cpu = hip.EventPre(torch.zeros(12, 20, dtype=torch.uint8))            # a mask that is not on the events' device
    calls = [lambda pre: hip.masked_normalize(ev, pre=pre), lambda pre: hip.masked_normalize_slice(ev, 0, 5, pre=pre),
             lambda pre: hip.masked_stats_slices(ev, 5, pre=pre), lambda pre: hip.masked_stats_slice(ev, 0, 5, pre=pre),
             lambda pre: hip.event_slice_to_nhwc8(ev, 0, 5, pre=pre),
             lambda pre: hip.e2vid_events_head_enc0(ev, 0, 5, True, None, None, True, None, None, True, pre=pre)]
    for call in calls:
        with pytest.raises(ValueError, match="hot_mask is \\(20, 12\\)"):
            call(other)
        with pytest.raises(ValueError, match="hot_mask is on cpu"):
            call(cpu)
        with pytest.raises(ValueError, match="hip.EventPre"):
            call((None, True))
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        hip.masked_normalize(torch.zeros(15, 12, 20), pre=hip.EventPre(flip=True))
    with pytest.raises(ValueError, match="normalize=False"):
        hip.masked_normalize_slice(ev, 0, 5, normalize=False)


# ------------------------------------------------------------------------------------------------------------------ surfaces
def test_cli_flags_parse_with_the_reference_names():
    from openess_amd.e2vid.run_reconstruction import build_parser
    a = build_parser().parse_args(["-c", "random", "-i", "events.txt", "--hot_pixels_file", "hot.txt", "--flip"])
    assert a.hot_pixels_file == "hot.txt" and a.flip is True
    b = build_parser().parse_args(["-c", "random", "-i", "events.txt"])
    assert b.hot_pixels_file is None and b.flip is False
    import inspect
    from openess_amd.e2vid.run_reconstruction import reconstruct
    sig = inspect.signature(reconstruct).parameters
    assert sig["hot_pixels_file"].default is None and sig["flip"].default is False


def test_online_recon_refuses_flip_and_serves_a_hot_pixel_list(tmp_path):
    from openess_amd.training.base_trainer_ov import online_recon_options
    from tests.test_online_recon_host import _settings
    s = _settings(tmp_path)
    s.e2vid_config.flip = True
    with pytest.raises(ValueError, match=r"e2vid_config\.flip"):
        online_recon_options(s)
    s.e2vid_config.flip = False
    s.e2vid_config.hot_pixels_file = str(tmp_path / "hot.txt")
    assert online_recon_options(s) == {'precision': 'bf16', 'model': 'random'}
    plain = _settings(tmp_path, "finetune_dsec_synthetic.yaml")          # without the key nothing is refused
    plain.e2vid_config.flip = True
    assert online_recon_options(plain) is None


def test_pretrain_step_hands_the_two_options_to_its_front_end(tmp_path):
    from openess_amd.training.pretrain_step import PretrainStep
    f = tmp_path / "hot.txt"
    f.write_text("1,2\n")
    kw = dict(img_size=(32, 48), nr_events_data=2, superpixel_size=25, device='cpu')
    st = PretrainStep(e2vid_options=SimpleNamespace(hot_pixels_file=str(f), flip=True, no_normalize=True), **kw)
    p = st.reconstructor.event_preprocessor
    assert p.flip and p.hot_pixel_locations.tolist() == [[1, 2]] and not p.no_normalize
    q = PretrainStep(e2vid_options=SimpleNamespace(hot_pixels_file=None, flip=False), **kw).reconstructor.event_preprocessor
    assert not q.flip and len(q.hot_pixel_locations) == 0 and q.pre_for(torch.zeros(1, 5, 32, 48)) is None


# ------------------------------------------------------------------------------------------------------------------ the fixture
@pytest.fixture(scope="module")
def golden():
    return dict(np.load(ec.GOLDEN))


@pytest.mark.parametrize("size", ec.SIZES)
@pytest.mark.parametrize("combo", sorted(ec.COMBOS))
def test_float64_restatement_reproduces_the_reference_fixture(golden, size, combo):
    """zero -> flip -> normalise in float64 NumPy against the reference's torch-fp32 output: 2 400 values of O(1), 1e-6."""
    hot, flip, nonorm = ec.COMBOS[combo]
    x, rows = golden[f"in_{size}"], golden[f"rows_{size}"]
    H, W = x.shape[2:]
    assert rows.tolist().count(rows[2].tolist()) == 2 and [0, 0] in rows.tolist() and [W - 1, H - 1] in rows.tolist()
    want = golden[f"out_{size}_{combo}"]
    got = ec.restate_f64(x, rows if hot else None, flip, nonorm)
    assert want.shape == got.shape == (2, 5, H, W)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
    if nonorm:
        assert np.array_equal(got.astype(np.float32), want)               # zero + flip alone move values, they do not round
