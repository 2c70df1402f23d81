"""CPU-side checks of the C-ABI boundary: the library loads and exports every symbol that
include/oess.h declares, and the Python binding lists exactly those symbols.  No compute calls."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "oess.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(oess_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_exported():
    from openess_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "liboess.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f"{n} declared in oess.h but not exported"


def test_binding_matches_header():
    from openess_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "oess.h")).read()
    declared_version = int(re.search(r"#define\s+OESS_ABI_VERSION\s+(\d+)", header).group(1))
    assert lib.oess_abi_version() == declared_version == _lib.ABI_VERSION
    assert b"gfx950" in lib.oess_build_info()
    assert lib.oess_strerror(-22) == b"invalid argument"


def test_workspace_query_and_argument_validation():
    """Host-only entry points / argument checks (return before any launch)."""
    from openess_amd import _lib
    lib = _lib.load()
    n = lib.oess_voxelize_workspace_bytes(1000, 4, 250, 5, 48, 64, 8)
    assert n >= 1000 * 4 * 16
    assert lib.oess_voxelize_workspace_bytes(-1, 4, 250, 5, 48, 64, 8) == 0
    # null pointers / bad shapes are rejected with OESS_EINVAL without touching the device
    assert lib.oess_voxelize_trilinear_f32(None, None, None, None, None, 1, 0, 5, 48, 64, 0, 0, None, None, 0, None) == -22
    assert lib.oess_task_loss_fwd(None, 0, None, 10, 10, 0, 0, 0, 11, 255, 3, None, None, None) == -22
    assert lib.oess_confusion_accumulate(None, None, 10, 11, 255, None, None) == -22


def test_round3_entry_points_validate_arguments_on_the_host():
    """Size queries and argument checks of the entry points added in round 3 (no launches)."""
    from openess_amd import _lib
    lib = _lib.load()
    # split-K scratch: wanted by the ASPP geometry at the BASELINE size, not by an ordinary layer or a tiny map
    assert lib.oess_conv2d_fwd_workspace_bytes(8, 28, 40, 2048, 256, 3, 3, 1, 12, 12, 1, 0) >= 2 * 8960 * 256 * 4
    assert lib.oess_conv2d_fwd_workspace_bytes(8, 110, 160, 64, 256, 1, 1, 1, 0, 1, 1, 0) == 0
    assert lib.oess_conv2d_fwd_workspace_bytes(0, 28, 40, 2048, 256, 3, 3, 1, 12, 12, 1, 0) == 0
    assert lib.oess_norm_partials_bytes(1, 140800, 256, 0) > 0 and lib.oess_norm_partials_bytes(0, 10, 8, 0) == 0
    assert lib.oess_png_decode_scratch_bytes(24 * 7000, 24, 440, 640) >= 24 * 440 * 641
    assert lib.oess_png_decode_gray8_batch(None, None, 100, 1, 8, 8, None, None, None, 0, None, None, None) == -22
    assert lib.oess_norm_tile_stats_apply_nhwc_bf16(None, 70, 256, 8960.0, 1e-5, None, None, None, None, 0.1, None, None, None, 256,
                                                    None, 0, 1, 8960, None, 256, None) == -22
    assert lib.oess_norm_stats_finalize_nhwc_bf16(None, 64, 1, 100, 64, 1e-5, None, None, None, None, 0.1, None, None, None, None,
                                                  None, 0, None) == -22


def test_stale_library_is_refused(tmp_path, monkeypatch):
    """A library built for another ABI version must not load (the version, not a missing symbol, is the check)."""
    import subprocess
    from openess_amd import _lib
    src = tmp_path / "fake.c"
    lines = ["int oess_abi_version(void) { return %d; }" % (_lib.ABI_VERSION - 1)]
    for name in _lib.SIGNATURES:
        if name != "oess_abi_version":
            lines.append(f"void* {name}(void) {{ return 0; }}")
    src.write_text("\n".join(lines))
    so = tmp_path / "libfake.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)])
    monkeypatch.setattr(_lib, "LIB_PATH", str(so))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.LibraryMissing, match="C-ABI version"):
        _lib.load()


def test_round4_entry_points_validate_arguments_on_the_host():
    from openess_amd import _lib
    lib = _lib.load()
    assert lib.oess_segment_mean_fwd_workspace_bytes(800, 256) >= 800 * 256 * 16 + 800 * 4 + 4
    assert lib.oess_segment_mean_fwd_workspace_bytes(0, 256) == 0
    assert lib.oess_segment_mean_fwd(None, 0, None, 100, 100, 100, 256, 100, None, None, None, 0, None) == -22
    assert lib.oess_linear_probe_partials_bytes(11) == 1024 * (121 + 11) * 8 and lib.oess_linear_probe_partials_bytes(33) == 0
    assert lib.oess_linear_probe_fwd_f32(None, None, None, 100, 11, None, None) == -22
    assert lib.oess_linear_probe_bwd_f32(None, None, None, 100, 11, None, None, None, None, 0, None) == -22
    assert lib.oess_maxpool3x3s2_fwd_nhwc_bf16(None, 64, 1, 8, 8, 64, None, 64, None, None) == -22
    assert lib.oess_maxpool3x3s2_bwd_nhwc_bf16(None, 64, None, 1, 8, 8, 64, None, 64, None) == -22
    assert lib.oess_dropout_nhwc_bf16(None, 8, None, 8, 10, 8, 0.1, 1, 2, None) == -22
    assert lib.oess_aspp_pool_fwd_f32(None, 1.0, None, None, None, None, None, 0.1, 1e-5, 8, 2048, 256, None, None, None, None, None) == -22
    assert lib.oess_aspp_pool_bwd_f32(None, None, 1.0, None, None, None, None, None, 8, 2048, 256, None, None, None, None, None, None) == -22


def test_collate_keeps_undecoded_png_maps_as_one_byte_stream():
    """device_png: collate concatenates the per-sample file bytes of a slot and keeps lengths / flips / size;
    every other slot stacks as before and the batch keeps the 7-slot layout."""
    import torch
    from openess_amd.datasets.synthetic_events import collate
    def sample(i):
        png = {'png': torch.arange(5 + i, dtype=torch.uint8), 'flip': bool(i & 1), 'hw': (4, 6)}
        return (torch.zeros(3, 4, 6), png, torch.ones(3, 4, 6), png, torch.zeros(4, 6, dtype=torch.int64), torch.ones(2), f"p{i}")
    b = collate([sample(0), sample(1), sample(2)])
    assert len(b) == 7 and b[0].shape == (3, 3, 4, 6) and b[6] == ["p0", "p1", "p2"]
    assert b[1]['png_lengths'] == [5, 6, 7] and b[1]['flip'] == [False, True, False] and b[1]['hw'] == (4, 6)
    assert b[1]['png_bytes'].numel() == 18 and torch.equal(b[3]['png_bytes'], b[1]['png_bytes'])
    assert b[4].shape == (3, 4, 6)


def test_product_path_refuses_cpu_tensors():
    import torch
    from openess_amd import hip
    with pytest.raises(RuntimeError):
        hip.masked_normalize(torch.zeros(4, 4))


def test_route_queries_run_on_the_host():
    """ABI 13: oess_conv2d_fwd_route / oess_convlstm_fused_route walk the launch's dispatch rules without a device; one known
    geometry per kernel family, and bad arguments come back as OESS_EINVAL like the launch's."""
    from openess_amd import _lib
    from tests.conv_route_cases import header_routes
    lib = _lib.load()
    R = header_routes()
    assert lib.oess_abi_version() == 13 and lib.oess_conv2d_route_count() == len(R) == 24

    def q(B, H, W, Cin, Cout, k, stride, pad, dil, bias=1, relu=0, res=0, f32=0, stats=0, ws=0, aligned=1):
        return lib.oess_conv2d_fwd_route(B, H, W, Cin, Cout, k, k, stride, pad, dil, bias, relu, res, f32, stats, Cin, (Cout + 7) // 8 * 8,
                                         (Cout + 7) // 8 * 8 if res else 0, aligned, ws)
    assert q(1, 33, 47, 8, 32, 5, 1, 2, 1) == R["SMALLCIN"]                                   # E2VID head
    assert q(2, 30, 42, 32, 64, 5, 2, 2, 1) == R["S2_HALO"]                                   # E2VID encoder
    assert q(1, 5, 7, 4096, 136, 3, 1, 1, 1) == R["FALLBACK_128"]                             # K >= 32768
    assert q(8, 28, 40, 1024, 256, 1, 1, 0, 1) == R["SMALLMAP_RING"]                          # DeepLabv3 OS16 1x1
    assert q(1, 9, 20, 64, 72, 3, 1, 1, 1) == R["HALO3X3"]
    assert q(8, 110, 160, 64, 256, 3, 1, 1, 1, bias=0, stats=1) == R["CONV3X3_W128"]
    assert q(8, 110, 160, 256, 1024, 1, 1, 0, 1, bias=0, stats=1) == R["CONV1X1_W128"]
    assert q(8, 110, 160, 256, 1024, 1, 1, 0, 1, res=1) == R["TILE256"]
    assert q(8, 110, 160, 64, 256, 1, 1, 0, 1) == R["RING32"]
    assert q(1, 9, 20, 64, 12, 3, 1, 1, 1, f32=1) == R["DMA32_FASTK"]
    # the ASPP geometry of test_round3_...: split-K with the workspace it asks for, one pass without
    need = lib.oess_conv2d_fwd_workspace_bytes(8, 28, 40, 2048, 256, 3, 3, 1, 12, 12, 1, 0)
    r = q(8, 28, 40, 2048, 256, 3, 1, 12, 12, bias=0, stats=1, ws=need)
    assert r & 0xff == R["SPLITK_FASTK"] and 2 <= r >> 8 <= 8 and need == (r >> 8) * 8960 * 256 * 4
    assert q(8, 28, 40, 2048, 256, 3, 1, 12, 12, bias=0, stats=1, ws=need - 1) == R["DMA128_FASTK"]
    assert lib.oess_convlstm_fused_route(1, 45, 60, 128, 128, 64, 3, 3, 1, 128) == R["HALO3X3_LSTM"]
    assert lib.oess_convlstm_fused_route(1, 45, 60, 128, 128, 64, 5, 5, 2, 128) == R["LSTM_FASTK"]
    assert lib.oess_conv2d_route_name(R["HALO3X3"]) == b"conv3x3_halo_kernel<0>"
    assert lib.oess_conv2d_route_name(r).startswith(b"split-K") and lib.oess_conv2d_route_name(0) == b"?"
    assert lib.oess_conv2d_route_name(-22) == b"?" and lib.oess_conv2d_route_name(25) == b"?"
    # bad arguments: Cin % 8, no pixels, a residual with an fp32 output, statistics with a bias, hidden size % 32, hidden stride < C
    assert q(1, 9, 20, 12, 72, 3, 1, 1, 1) == -22
    assert q(0, 9, 20, 64, 72, 3, 1, 1, 1) == -22
    assert q(1, 9, 20, 64, 72, 3, 1, 1, 1, res=1, f32=1) == -22
    assert q(1, 9, 20, 64, 72, 3, 1, 1, 1, bias=1, stats=1) == -22
    assert lib.oess_convlstm_fused_route(1, 45, 60, 128, 128, 48, 3, 3, 1, 128) == -22
    assert lib.oess_convlstm_fused_route(1, 45, 60, 128, 128, 64, 3, 3, 1, 32) == -22
