"""What the PNG encoder promises without a GPU: its symbols, its size queries, the refusals that come before the
first HIP call, the wrapper's refusal of host tensors and the tools' --png-encoder option."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("oess_png_encode_bound", "oess_png_encode_scratch_bytes", "oess_png_encode_batch")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_symbols_in_header_binding_and_library():
    from openess_amd import _lib, hip
    header = open(os.path.join(ROOT, "include", "oess.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)) and n in _lib.SIGNATURES and hasattr(lib, n)
    seg = int(re.search(r"#define\s+OESS_PNG_ENCODE_SEGMENT\s+(\d+)", header).group(1))
    assert seg == hip.PNG_ENCODE_SEGMENT == 16384 and seg <= 65535
    assert _lib.load().oess_abi_version() == _lib.ABI_VERSION == 13
    assert _lib.load().oess_conv2d_route_count() == 24


def test_size_queries():
    from openess_amd import _lib, hip
    lib = _lib.load()
    S = 440 * (1 + 640 * 3)
    nseg = (S + 16383) // 16384
    assert lib.oess_png_encode_bound(440, 640, 3) == 75 + S + 17 * nseg == hip.png_encode_bound(440, 640, 3)
    assert lib.oess_png_encode_bound(1, 1, 1) == 75 + 2 + 17
    assert lib.oess_png_encode_bound(16384, 16384, 3) == 75 + 16384 * 49153 + 17 * 49153
    # every segment's chunk (12 + 5 + 16384 bytes at most), its sizes and checksums have room
    assert lib.oess_png_encode_scratch_bytes(8, 440, 640, 3) >= 8 * nseg * (12 + 5 + 16384 + 16)
    assert lib.oess_png_encode_scratch_bytes(8, 440, 640, 3) < 2 * 8 * nseg * 16384
    for bad in ((0, 4, 4, 1), (-1, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 16385, 4, 1), (1, 4, 16385, 1), (1, 4, 4, 2), (1, 4, 4, 0),
                (43690, 16384, 16384, 3)):
        assert lib.oess_png_encode_scratch_bytes(*bad) == 0
    assert lib.oess_png_encode_scratch_bytes(43689, 16384, 16384, 3) > 0
    for bad in ((0, 4, 1), (4, 0, 1), (16385, 4, 1), (4, 16385, 3), (4, 4, 2), (4, 4, -1)):
        assert lib.oess_png_encode_bound(*bad) == 0
        with pytest.raises(ValueError):
            hip.png_encode_bound(*bad)


def test_entry_refuses_before_the_first_hip_call():
    """null device pointers: nothing here can reach a launch"""
    from openess_amd import _lib
    lib = _lib.load()
    bound = lib.oess_png_encode_bound(8, 8, 1)
    need = lib.oess_png_encode_scratch_bytes(1, 8, 8, 1)
    fake = 1 << 20                                               # never dereferenced: a refusal comes first
    assert lib.oess_png_encode_batch(None, 1, 8, 8, 1, None, bound, None, None, need, None) == -22
    assert lib.oess_png_encode_batch(None, 1, 8, 8, 1, fake, bound, fake, fake, need, None) == -22
    assert lib.oess_png_encode_batch(fake, 1, 8, 8, 1, None, bound, fake, fake, need, None) == -22
    assert lib.oess_png_encode_batch(fake, 1, 8, 8, 1, fake, bound, None, fake, need, None) == -22
    assert lib.oess_png_encode_batch(fake, 1, 8, 8, 1, fake, bound, fake, None, need, None) == -22
    assert lib.oess_png_encode_batch(fake, 0, 8, 8, 1, fake, bound, fake, fake, need, None) == -22
    assert lib.oess_png_encode_batch(fake, 1, 8, 8, 2, fake, bound, fake, fake, need, None) == -22
    assert lib.oess_png_encode_batch(fake, 1, 0, 8, 1, fake, bound, fake, fake, need, None) == -22
    assert lib.oess_png_encode_batch(fake, 1, 8, 16385, 1, fake, 1 << 40, fake, fake, 1 << 40, None) == -22
    assert lib.oess_png_encode_batch(fake, 1, 8, 8, 1, fake, bound - 1, fake, fake, need, None) == -22
    assert lib.oess_png_encode_batch(fake, 1, 8, 8, 1, fake, bound, fake, fake, need - 1, None) == -22
    assert lib.oess_png_encode_batch(fake, 43690, 16384, 16384, 3, fake, 1 << 40, fake, fake, 1 << 62, None) == -22


def test_wrapper_refuses_host_tensors():
    from openess_amd import hip
    for t in (torch.zeros((1, 4, 4), dtype=torch.uint8), torch.zeros((1, 4, 4, 3), dtype=torch.uint8), None, [[1, 2]]):
        with pytest.raises(ValueError):
            hip.png_encode_batch(t)
        with pytest.raises(ValueError):
            hip.png_encode_files(t)


def test_tools_parse_png_encoder(capsys):
    seg = _tool("segment")
    ap = seg.build_parser()
    assert ap.parse_args(["-o", "x"]).png_encoder == "host"
    assert ap.parse_args(["-o", "x", "--png-encoder", "gpu"]).png_encoder == "gpu"
    assert ap.parse_args(["-o", "x", "--png-encoder", "host"]).png_encoder == "host"
    with pytest.raises(SystemExit):
        ap.parse_args(["-o", "x", "--png-encoder", "zlib"])
    assert "--png-encoder" in capsys.readouterr().err
    slic = _tool("write_slic_superpixels")
    with pytest.raises(SystemExit):
        slic.main(["--root", ".", "--png-encoder", "pillow"])
    assert "--png-encoder" in capsys.readouterr().err
    with pytest.raises(SystemExit, match="is not a directory"):       # the option parses; the missing root is what stops it
        slic.main(["--root", os.path.join(ROOT, "no", "such", "dir"), "--png-encoder", "gpu"])
