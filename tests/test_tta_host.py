"""Host side of K39 (no GPU): oess_segment_render_ensemble in the header, the binding and the library with the ABI untouched, its
refusals (they return before the first HIP call), hip.ensemble_render's ValueErrors on CPU tensors, and the flip / multi-scale
refusals of the Segmenter and of tools/segment.py."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "oess_segment_render_ensemble"


def test_entry_is_declared_bound_and_exported():
    from openess_amd import _lib, hip
    header = open(os.path.join(ROOT, "include", "oess.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int\s+" + NAME + r"\s*\(([^)]*)\)", code)
    assert m and len(m.group(1).split(',')) == 21
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == 21 and args[5] is ctypes.c_int and args[15] is ctypes.c_float
    assert all(a is ctypes.c_void_p for a in args[:5])
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    lib = _lib.load()
    assert getattr(lib, NAME).argtypes == args
    assert lib.oess_abi_version() == 13 == _lib.ABI_VERSION and int(re.search(r"#define\s+OESS_ABI_VERSION\s+(\d+)", header).group(1)) == 13
    assert lib.oess_conv2d_route_count() == 24 and int(re.search(r"#define\s+OESS_ROUTE_COUNT\s+(\d+)", header).group(1)) == 24
    assert int(re.search(r"#define\s+OESS_RENDER_MAX_VIEWS\s+(\d+)", header).group(1)) == 8 == hip.RENDER_MAX_VIEWS


def test_entry_refuses_on_the_host():
    """every refusal returns before the first HIP call: the device pointers are never read"""
    from openess_amd import _lib
    f = getattr(_lib.load(), NAME)
    ok = dict(ptrs=[4096, 8192], ps=[11, 14], hs=[3, 6], ws=[4, 8], flips=[0, 1], V=2, bf16=0, B=2, K=11, H=6, W=8, ac=0, palette=12288,
              grey=16384, alpha256=128, min_conf=0.0, ignore=255, labels=20480, conf=24576, rgb=28672)

    def arr(ctype, values):
        return None if values is None else (ctype * len(values))(*values)

    def call(**kw):
        a = dict(ok)
        for key, value in kw.items():
            if isinstance(value, tuple):                                  # (index, value): one entry of a host array
                a[key] = list(a[key])
                a[key][value[0]] = value[1]
            else:
                a[key] = value
        return f(arr(ctypes.c_void_p, a['ptrs']), arr(ctypes.c_longlong, a['ps']), arr(ctypes.c_int, a['hs']), arr(ctypes.c_int, a['ws']),
                 arr(ctypes.c_int, a['flips']), a['V'], a['bf16'], a['B'], a['K'], a['H'], a['W'], a['ac'], a['palette'], a['grey'],
                 a['alpha256'], a['min_conf'], a['ignore'], a['labels'], a['conf'], a['rgb'], None)
    for bad in (dict(ptrs=None), dict(ps=None), dict(hs=None), dict(ws=None), dict(flips=None), dict(ptrs=(0, None)), dict(ptrs=(1, None)),
                dict(V=0), dict(V=-2), dict(V=9), dict(flips=(0, 2)), dict(flips=(1, -1)), dict(hs=(0, 0)), dict(ws=(1, -8)),
                dict(ps=(0, 10)), dict(ps=(1, 0)), dict(labels=None, conf=None, rgb=None), dict(palette=None), dict(K=0), dict(K=-3),
                dict(K=256, ps=[256, 256]), dict(ignore=10), dict(ignore=-1), dict(ignore=256), dict(alpha256=-1), dict(alpha256=257),
                dict(min_conf=float('nan')), dict(min_conf=-1e-3), dict(B=0), dict(H=0), dict(W=-2), dict(B=1 << 16, H=1 << 16),
                dict(B=1 << 16, H=1, hs=(1, 1 << 16)), dict(ps=(1, 1 << 62)), dict(B=1, H=(1 << 31) - 1, W=(1 << 31) - 1)):
        assert call(**bad) == -22, bad


def test_wrapper_refuses_on_cpu_tensors():
    from openess_amd import hip
    x, y = torch.zeros(2, 5, 3, 4), torch.zeros(2, 5, 6, 8)
    for bad in ([], None, x, [x] * 9):
        with pytest.raises(ValueError, match="1 ... 8 views"):
            hip.ensemble_render(bad)
    for bad in ([True], [0, 1, 0], [0, 2]):
        with pytest.raises(ValueError, match="flips must hold"):
            hip.ensemble_render([x, y], flips=bad)
    for bad in (y.bfloat16(), y[:1], y[:, :4]):
        with pytest.raises(ValueError, match="share view 0's"):
            hip.ensemble_render([x, bad])
    for bad in (y.half(), y[0], None):
        with pytest.raises(ValueError, match="float32 / bfloat16"):
            hip.ensemble_render([x, bad])
    with pytest.raises(ValueError, match="no CPU fallback"):
        hip.ensemble_render([x, y], flips=[0, 1])
    with pytest.raises(ValueError, match="no CPU fallback"):
        hip.ensemble_render([x])                                          # one unflipped view is segment_render: its refusal


def test_views_and_their_refusals():
    from openess_amd.inference import tta_views
    assert tta_views() == [(1.0, False)] and tta_views(False, (1.0,)) == [(1.0, False)]
    assert tta_views(True) == [(1.0, False), (1.0, True)]
    assert tta_views(True, (0.75, 1, 1.25)) == [(1.0, False), (1.0, True), (0.75, False), (0.75, True), (1.25, False), (1.25, True)]
    assert len(tta_views(False, (1, 0.5, 0.75, 1.25, 1.5, 1.75, 2, 2.25))) == 8
    with pytest.raises(ValueError, match="at most 8 views"):
        tta_views(True, (1, 0.5, 0.75, 1.25, 1.5))
    with pytest.raises(ValueError, match="at most 8 views"):
        tta_views(False, (1, 0.5, 0.75, 1.25, 1.5, 1.75, 2, 2.25, 2.5))
    for bad in ((1.0, 0.0), (1.0, -0.5), (1.0, float('nan')), (1.0, float('inf')), ()):
        with pytest.raises(ValueError, match="finite and positive"):
            tta_views(False, bad)
    for bad in ((0.5, 0.75), (1.0, 1.0), (1, 0.5, 0.5)):
        with pytest.raises(ValueError, match="must hold 1.0"):
            tta_views(False, bad)
    with pytest.raises(ValueError, match="sequence of numbers"):
        tta_views(False, ("a",))


def test_segmenter_refuses_before_it_touches_a_network():
    """on bare objects: the refusals read nothing but the flags they are about"""
    from types import SimpleNamespace
    from openess_amd.inference import Segmenter
    seg = object.__new__(Segmenter)
    seg.is_event, seg.config_option, seg._vocab = True, 'frame2voxel', None
    with pytest.raises(ValueError, match="flip only"):
        seg.predict_events(None, scales=(0.75, 1.0))
    with pytest.raises(ValueError, match="flip only"):
        seg.predict((None, None, None), flip=True, scales=(1.0, 1.25))
    with pytest.raises(ValueError, match="finite and positive"):
        seg.predict_events(None, scales=(1.0, 0.0))
    seg._vocab = SimpleNamespace()
    with pytest.raises(ValueError, match="follow-up"):
        seg.predict_events(None, flip=True)
    seg._vocab = None
    seg._rec = SimpleNamespace(crop=SimpleNamespace(padding_left=3, padding_right=2))
    with pytest.raises(ValueError, match="left and right padding"):
        seg.predict_events(None, flip=True)
    img = object.__new__(Segmenter)
    img.is_event, img.config_option, img._vocab = False, 'frame2recon', SimpleNamespace()
    img.trainer = SimpleNamespace(models_dict={'model_recon': SimpleNamespace(if_linear_probing=False)})
    with pytest.raises(ValueError, match="follow-up"):
        img.predict((None, None, torch.zeros(1, 3, 8, 8)), scales=(1.0, 0.5))
    with pytest.raises(ValueError, match="at most 8 views"):
        img.predict((None, None, torch.zeros(1, 3, 8, 8)), flip=True, scales=(1, 0.5, 0.75, 1.25, 1.5))
    img._vocab = None
    img.trainer.models_dict['model_recon'].if_linear_probing = True
    with pytest.raises(ValueError, match="linear probe"):
        img.predict((None, None, torch.zeros(1, 3, 8, 8)), scales=(1.0, 0.5))


def _tool():
    spec = importlib.util.spec_from_file_location("segment_tool", os.path.join(ROOT, "tools", "segment.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_cli_argument_errors(tmp_path, capsys):
    tool = _tool()
    out = str(tmp_path / "out")
    cases = {
        "scales_on_an_event_student": (["-o", out, "--tta-scales", "0.75,1"], "--tta-scales needs --config-option frame2recon"),
        "scales_no_numbers": (["-o", out, "--config-option", "frame2recon", "--tta-scales", "1,big"], "comma list of numbers"),
        "scale_zero": (["-o", out, "--config-option", "frame2recon", "--tta-scales", "1,0"], "finite and positive"),
        "scale_negative": (["-o", out, "--config-option", "frame2recon", "--tta-scales=-1,1"], "finite and positive"),
        "scales_without_one": (["-o", out, "--config-option", "frame2recon", "--tta-scales", "0.5,0.75"], "must hold 1.0"),
        "nine_views": (["-o", out, "--config-option", "frame2recon", "--tta", "flip", "--tta-scales", "1,0.5,0.75,1.25,1.5"],
                       "at most 8 views"),
        "flip_with_classes": (["-o", out, "--tta", "flip", "--classes", "road,car"], "with --classes"),
        "scales_with_classes": (["-o", out, "--config-option", "frame2recon", "--tta-scales", "1,0.5", "--classes", "road,car"],
                                "with --classes"),
        "unknown_tta": (["-o", out, "--tta", "rotate"], "invalid choice"),
    }
    for name, (argv, message) in cases.items():
        with pytest.raises(SystemExit) as e:
            tool.main(argv)
        assert e.value.code == 2, name
        assert message in capsys.readouterr().err, name
    assert not os.path.exists(out)                                        # refused before anything is written
    # valid command lines pass the checks (no model is built by them)
    a = tool.build_parser().parse_args(["-o", out, "--config-option", "frame2recon", "--tta", "flip", "--tta-scales", "0.75,1,1.25"])
    tool.check_args(tool.build_parser(), a)
    assert (a.tta_flip, a.tta_scale_list, a.tta_views) == (True, (0.75, 1.0, 1.25), 6)
    a = tool.build_parser().parse_args(["-o", out])
    tool.check_args(tool.build_parser(), a)
    assert (a.tta_flip, a.tta_scale_list, a.tta_views) == (False, (1.0,), 1) and tool._tta(a) == {}
