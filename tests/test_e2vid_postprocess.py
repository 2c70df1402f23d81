"""E2VID post-processing, host side: gkern against the reference's weights, argument checks of the C-ABI entry points
(they return OESS_EINVAL before any launch), the wrapper's refusal of host tensors, the PostProcessor's refusals and the CLI's
flag rule.  No GPU needed; tests/test_hip_e2vid_postprocess.py runs the kernels."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM = -22, -12


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "e2vid_post.npz")))


def test_gkern_bit_equal_to_reference(golden):
    from openess_amd.e2vid.utils.inference_utils import gkern
    for s, w in zip(golden["gkern_sigma"], golden["gkern_w"]):
        g = gkern(5, float(s))
        assert g.dtype == torch.float32 and g.shape == (5, 5)
        assert np.array_equal(g.numpy().view(np.uint32), w.view(np.uint32)), s


def test_postprocess_entry_points_reject_bad_arguments():
    from openess_amd import _lib
    lib = _lib.load()
    assert lib.oess_e2vid_postproc_state_bytes(10) >= 48 + 2 * 8 * 11
    assert lib.oess_e2vid_postproc_state_bytes(0) >= 48 + 2 * 8
    assert lib.oess_e2vid_postproc_state_bytes(-1) == 0 and lib.oess_e2vid_postproc_state_bytes(256) == 0
    w = (torch.ones(25) / 25).contiguous()
    img, out, state = 1 << 20, 2 << 20, 3 << 20            # never dereferenced: every call below fails its host-side checks
    sb = lib.oess_e2vid_postproc_state_bytes(10)

    def fixed(img=img, ist=35, rst=7, N=1, H=5, W=7, wp=w.data_ptr(), a=0.3, lo=0.0, hi=1.0, out=out):
        return lib.oess_e2vid_postprocess_f32(img, ist, rst, N, H, W, wp, a, lo, hi, out, None, None)

    def auto(img=img, ist=35, rst=7, N=1, H=5, W=7, wp=w.data_ptr(), a=0.3, fs=10, st=state, sbytes=sb, out=out):
        return lib.oess_e2vid_postprocess_auto_hdr_f32(img, ist, rst, N, H, W, wp, a, fs, st, sbytes, out, None, None)

    for call in (fixed, auto):
        assert call(img=None) == EINVAL
        assert call(out=None) == EINVAL
        assert call(wp=None) == EINVAL                      # weights are needed when the unsharp mask is on
        for bad in ({"N": 0}, {"H": 0}, {"W": 0}, {"N": -1}, {"H": -3}, {"W": -7}):
            assert call(**bad) == EINVAL, bad
        assert call(rst=6) == EINVAL                        # row stride < W
        assert call(N=2, ist=20) == EINVAL                  # images overlap
    assert fixed(lo=1.0, hi=1.0) == EINVAL                  # Imax <= Imin: the reference divides by zero
    assert fixed(lo=0.6, hi=0.5) == EINVAL
    assert fixed(lo=0.0, hi=float("nan")) == EINVAL
    assert auto(st=None) == EINVAL
    assert auto(fs=-1) == EINVAL
    assert auto(fs=256) == EINVAL
    assert auto(sbytes=sb - 8) == ENOMEM


def test_postprocess_wrapper_refuses_host_tensors():
    from openess_amd import hip
    from openess_amd.e2vid.utils.inference_utils import gkern
    x = torch.rand(1, 1, 8, 8)
    with pytest.raises(RuntimeError, match="CUDA/HIP tensors"):
        hip.e2vid_postprocess(x, gkern(), 0.3, bounds=(0.0, 1.0))
    with pytest.raises(ValueError, match="filter_size"):
        hip.E2VIDHdrState(256, "cpu")


def test_postprocessor_refuses_bilateral_filter_and_colour():
    from openess_amd.e2vid.image_reconstructor import PostProcessor
    with pytest.raises(NotImplementedError, match="bilateral"):
        PostProcessor("cpu", SimpleNamespace(bilateral_filter_sigma=1.0))
    with pytest.raises(NotImplementedError, match="colour"):
        PostProcessor("cpu", SimpleNamespace(color=True))
    with pytest.raises(ValueError, match="Imax"):
        PostProcessor("cpu", SimpleNamespace(Imin=0.5, Imax=0.5))


@pytest.mark.parametrize("flags", [["--auto_hdr"], ["--unsharp_mask_amount", "0.5"], ["--unsharp_mask_sigma", "2"], ["--Imin", "0.1"],
                                   ["--Imax", "0.9"], ["--auto_hdr_median_filter_size", "3"], ["--bilateral_filter_sigma", "0"]])
def test_cli_refuses_postprocess_flags_without_postprocess(flags, capsys):
    from openess_amd.e2vid import run_reconstruction as rr
    with pytest.raises(SystemExit) as e:
        rr.main(["-c", "random", "-i", "events.txt"] + flags)
    assert e.value.code == 2
    assert "--postprocess" in capsys.readouterr().err
