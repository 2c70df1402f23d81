"""Host side of K35 (no GPU): the new C entry in the header, the binding and the library with the ABI untouched, its refusals (they
return before the first HIP call), the wrapper's and the Segmenter's refusals that need no device, and the argument errors of
tools/segment.py."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "configs", "finetune_dsec_synthetic.yaml")


def test_entry_is_declared_bound_and_exported():
    from openess_amd import _lib
    header = open(os.path.join(ROOT, "include", "oess.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int\s+oess_segment_render\s*\(([^)]*)\)", code)
    assert m and len(m.group(1).split(',')) == 19
    res, args = _lib.SIGNATURES["oess_segment_render"]
    assert res is ctypes.c_int and len(args) == 19 and args[2] is ctypes.c_longlong and args[13] is ctypes.c_float
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "oess_segment_render")
    lib = _lib.load()
    assert lib.oess_segment_render.argtypes == args
    assert lib.oess_abi_version() == 13 == _lib.ABI_VERSION and int(re.search(r"#define\s+OESS_ABI_VERSION\s+(\d+)", header).group(1)) == 13
    assert lib.oess_conv2d_route_count() == 24


def test_entry_refuses_on_the_host():
    """every refusal returns before the first HIP call: the pointers are never read"""
    from openess_amd import _lib
    f = _lib.load().oess_segment_render
    ok = dict(logits=4096, bf16=0, ps=11, B=2, K=11, h=3, w=4, H=6, W=8, ac=0, palette=8192, grey=12288, alpha256=128, min_conf=0.0,
              ignore=255, labels=16384, conf=20480, rgb=24576)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['logits'], a['bf16'], a['ps'], a['B'], a['K'], a['h'], a['w'], a['H'], a['W'], a['ac'], a['palette'], a['grey'],
                 a['alpha256'], a['min_conf'], a['ignore'], a['labels'], a['conf'], a['rgb'], None)
    for bad in (dict(logits=None), dict(labels=None, conf=None, rgb=None), dict(palette=None), dict(K=0), dict(K=-3), dict(K=256, ps=256),
                dict(ignore=10), dict(ignore=0), dict(ignore=-1), dict(ignore=256), dict(alpha256=-1), dict(alpha256=257),
                dict(min_conf=float('nan')), dict(min_conf=-1e-3), dict(B=0), dict(h=0), dict(w=-1), dict(H=0), dict(W=-2), dict(ps=10),
                dict(B=1 << 16, H=1 << 16), dict(B=1 << 16, h=1 << 16), dict(ps=1 << 62), dict(B=1, H=(1 << 31) - 1, W=(1 << 31) - 1)):
        assert call(**bad) == -22, bad


def test_wrapper_refuses_a_cpu_tensor():
    from openess_amd import hip
    with pytest.raises(ValueError, match="no CPU fallback"):
        hip.segment_render(torch.zeros(1, 3, 2, 2))
    with pytest.raises(ValueError, match="no CPU fallback"):
        hip.segment_render(None)


def test_segmenter_refuses_bad_arguments_before_building_anything():
    from openess_amd.inference import Segmenter
    with pytest.raises(ValueError, match="precision"):
        Segmenter(CFG, precision='fp16')
    with pytest.raises(ValueError, match="config_option"):
        Segmenter(CFG, config_option='voxel2frame')


def test_logits_at_stride_refuses_train_mode_a_probe_and_a_precision():
    from openess_amd.models.deeplabv3 import deeplabv3_resnet50
    net = deeplabv3_resnet50(11, '', 32, '')
    x = torch.zeros(1, 3, 64, 96)
    net.train()
    for precision in ('bf16', 'fp32'):
        with pytest.raises(NotImplementedError, match="train mode"):
            net.logits_at_stride(x, precision)
    with pytest.raises(ValueError, match="precision"):
        net.eval().logits_at_stride(x, 'fp16')
    probe = deeplabv3_resnet50(11, '', 32, '', if_linear_probing=True).eval()
    with pytest.raises(NotImplementedError, match="linear probe"):
        probe.logits_at_stride(x)


def _tool():
    spec = importlib.util.spec_from_file_location("segment_tool", os.path.join(ROOT, "tools", "segment.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _events(tmp_path, W, H):
    path = tmp_path / "events.txt"
    path.write_text(f"{W} {H}\n0.000001000 1 2 1\n0.000002000 3 4 0\n")
    return str(path)


def test_cli_argument_errors(tmp_path, capsys):
    tool = _tool()
    out = str(tmp_path / "out")
    good = _events(tmp_path, 96, 64)
    cases = {
        "events_with_frame2recon": (["-o", out, "-i", good, "--config-option", "frame2recon"], "event students"),
        "stateful_without_events": (["-o", out, "--stateful"], "--stateful needs -i"),
        "window_without_events": (["-o", out, "-N", "100"], "-N needs -i"),
        "two_sources": (["-o", out, "-i", good, "--split", "val"], "two sources"),
        "overlay_with_frame2recon": (["-o", out, "--overlay", "recon", "--config-option", "frame2recon"], "--overlay recon"),
        "alpha": (["-o", out, "--alpha", "1.5"], "--alpha"),
        "min_conf": (["-o", out, "--min-conf", "-0.1"], "--min-conf"),
        "missing_events": (["-o", out, "-i", str(tmp_path / "absent.txt")], "not found"),
    }
    for name, (argv, message) in cases.items():
        with pytest.raises(SystemExit) as e:
            tool.main(argv)
        assert e.value.code == 2, name
        assert message in capsys.readouterr().err, name
    bad = tmp_path / "wrong"
    bad.mkdir()
    with pytest.raises(SystemExit) as e:
        tool.main(["-o", out, "-i", _events(bad, 640, 480)])
    assert e.value.code == 2 and "480 x 640 is not the settings' shape [64, 96]" in capsys.readouterr().err
    assert not os.path.exists(out)                                        # refused before anything is written
    # a valid command line passes the checks (no model is built by them)
    a = tool.build_parser().parse_args(["-o", out, "-i", good, "--stateful", "--overlay", "recon"])
    assert tool.check_args(tool.build_parser(), a).img_size_b == [64, 96]
