"""CPU-side checks of the fp32 E2VID inference path (K14): argument validation of the new C entry points (OESS_EINVAL before any
device work), the fp32 weight packings, the --precision flag, and what ImageReconstructor refuses with precision='fp32'."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from oracle.step import E2VID_LIGHTWEIGHT_CONFIG

FAKE = 4096          # a 16-byte aligned non-null address: every call below is refused on the host before it could be used


def _view(ptr, sb=0, sy=0, sx=0, sc=1):
    from openess_amd import _lib
    return _lib.F32View(ptr, sb, sy, sx, sc)


def test_fp32_entry_points_reject_bad_arguments():
    from openess_amd import _lib
    lib = _lib.load()
    by = ctypes.byref
    v, o = _view(FAKE, 1000, 100, 10), _view(FAKE, 1000, 100, 10)
    ok = dict(B=1, H=8, W=8, Cin=16, up=0, w=FAKE, b=None, Cout=32, R=3, S=3, stride=1, pad=1, act=1)

    def conv(inp=v, in2=None, res=None, out=o, **kw):
        a = dict(ok, **kw)
        return lib.oess_conv2d_fwd_f32(inp, in2, a['B'], a['H'], a['W'], a['Cin'], a['up'], a['w'], a['b'], a['Cout'], a['R'], a['S'],
                                       a['stride'], a['pad'], a['act'], res, out, None)
    # null pointers
    assert conv(inp=None, out=by(o)) == -22
    assert conv(inp=by(_view(None)), out=by(o)) == -22
    assert conv(inp=by(v), out=None) == -22
    assert conv(inp=by(v), out=by(o), w=None) == -22
    assert conv(inp=by(v), out=by(o), w=FAKE + 4) == -22                       # packed weights must be 16-byte aligned
    assert conv(inp=by(v), in2=by(_view(None)), out=by(o)) == -22
    assert conv(inp=by(v), res=by(_view(None)), out=by(o)) == -22
    # impossible geometries
    for bad in (dict(B=0), dict(H=0), dict(Cin=0), dict(Cout=0), dict(R=6, S=5), dict(stride=3), dict(pad=3), dict(act=3),
                dict(up=2), dict(R=5, S=5, pad=2, H=1, W=1, stride=1, Cin=16, Cout=32, B=-1)):
        assert conv(inp=by(v), out=by(o), **bad) == -22, bad
    assert conv(inp=by(v), out=by(o), R=5, S=5, pad=0, H=3, W=3) == -22       # output would be empty
    # transposed convolution
    assert lib.oess_conv_transpose2d_fwd_f32(None, None, 1, 4, 4, 16, FAKE, None, 32, 1, by(o), None) == -22
    assert lib.oess_conv_transpose2d_fwd_f32(by(v), None, 1, 4, 4, 16, FAKE, None, 32, 1, None, None) == -22
    assert lib.oess_conv_transpose2d_fwd_f32(by(v), None, 1, 4, 4, 16, FAKE, None, 0, 1, by(o), None) == -22
    assert lib.oess_conv_transpose2d_fwd_f32(by(v), None, 0, 4, 4, 16, FAKE, None, 32, 1, by(o), None) == -22
    assert lib.oess_conv_transpose2d_fwd_f32(by(v), None, 1, 4, 4, 16, FAKE, None, 32, 5, by(o), None) == -22
    # ConvLSTM step
    C = 16
    ws = lib.oess_convlstm_f32_workspace_bytes(64, C)
    assert ws == 64 * 4 * C * 4 and lib.oess_convlstm_f32_workspace_bytes(0, C) == 0

    def step(xh=by(v), w=FAKE, cell=FAKE, hid=by(o), wsp=FAKE, nbytes=ws, R=3, S=3, pad=1, zero=0, Cin=2 * C, Ch=C):
        return lib.oess_convlstm_step_f32(xh, 1, 8, 8, Cin, w, None, Ch, R, S, pad, zero, cell, hid, wsp, nbytes, None)
    for bad in (dict(xh=None), dict(w=None), dict(cell=None), dict(hid=None), dict(wsp=None), dict(pad=0), dict(R=3, S=5, pad=1),
                dict(zero=2), dict(Ch=0), dict(Cin=0), dict(wsp=FAKE + 8)):
        assert step(**bad) == -22, bad
    assert step(nbytes=ws - 4) == -12                                          # workspace too small: OESS_ENOMEM
    # size queries
    assert lib.oess_conv2d_f32_packed_floats(1, 5, 5, 5) == 128 * 32
    assert lib.oess_conv2d_f32_packed_floats(256, 256, 3, 3) == 2304 * 256
    assert lib.oess_conv2d_f32_packed_floats(32, 5, 6, 5) == 0 and lib.oess_conv2d_f32_packed_floats(0, 5, 5, 5) == 0
    assert lib.oess_conv_transpose2d_f32_packed_floats(32, 64) == (9 + 6 + 6 + 4) * 64 * 32
    assert lib.oess_conv_transpose2d_f32_packed_floats(32, 0) == 0


def test_fp32_weight_packings():
    """Row / column conventions of include/oess.h, checked element by element on the host."""
    from openess_amd import hip
    torch.manual_seed(0)
    w = torch.randn(3, 5, 5, 5)                            # Conv2d [Cout, Cin, R, S]
    p = hip.pack_conv_weight_f32(w)
    assert p.shape == (128, 32)
    for co, ci, r, s in ((0, 0, 0, 0), (2, 4, 4, 3), (1, 3, 2, 1)):
        assert p[(r * 5 + s) * 5 + ci, co] == w[co, ci, r, s]
    assert p[125:].abs().max() == 0 and p[:, 3:].abs().max() == 0
    wt = torch.randn(16, 40, 5, 5)                         # ConvTranspose2d [Cin, Cout, 5, 5]
    pt = hip.pack_conv_transpose_weight_f32(wt)
    Cp = 64
    off = 0
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        ny, nx = 3 - py, 3 - px
        blk = pt[off:off + ny * nx * 16 * Cp].reshape(ny * nx * 16, Cp)
        for ty, tx, ci, co in ((0, 0, 0, 0), (ny - 1, nx - 1, 15, 39), (1, 0, 7, 5)):
            assert blk[(ty * nx + tx) * 16 + ci, co] == wt[ci, co, py + 2 * ty, px + 2 * tx]
        assert blk[:, 40:].abs().max() == 0
        off += ny * nx * 16 * Cp
    assert off == pt.numel()


def test_precision_flag(monkeypatch):
    from openess_amd.e2vid import run_reconstruction as rr
    got = {}
    monkeypatch.setattr(rr, "load_model", lambda path: "model")
    monkeypatch.setattr(rr, "reconstruct", lambda *a, **kw: got.update(kw))
    rr.main(["-c", "random", "-i", "events.txt"])
    assert got["precision"] == "bf16"
    rr.main(["-c", "random", "-i", "events.txt", "--precision", "fp32"])
    assert got["precision"] == "fp32"
    with pytest.raises(SystemExit):
        rr.main(["-c", "random", "-i", "events.txt", "--precision", "fp16"])


def test_reconstruct_rejects_unknown_precision():
    from openess_amd.e2vid import run_reconstruction as rr
    with pytest.raises(ValueError, match="precision"):
        rr.reconstruct("no-such-file.txt", None, precision="fp16")


def _model(**cfg):
    from openess_amd.e2vid.model.model import E2VIDRecurrent
    return E2VIDRecurrent(dict(E2VID_LIGHTWEIGHT_CONFIG, **cfg)).eval()


def test_image_reconstructor_fp32_refusals():
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor
    fp32 = SimpleNamespace(precision='fp32')
    with pytest.raises(ValueError, match="precision"):
        ImageReconstructor(_model(), 32, 48, 5, torch.device('cpu'), SimpleNamespace(precision='fp16'))
    with pytest.raises(NotImplementedError, match="IN"):
        ImageReconstructor(_model(norm='IN'), 32, 48, 5, torch.device('cpu'), fp32)
    with pytest.raises(NotImplementedError, match="IN"):
        _model(norm='IN').forward_fp32(torch.zeros(1, 5, 32, 48), None)
    ev = torch.zeros(1, 5, 32, 48)
    # the bf16 schedule options have no fp32 form
    rec = ImageReconstructor(_model(), 32, 48, 5, torch.device('cpu'), fp32)
    with pytest.raises(ValueError, match="wavefront"):
        rec.update_reconstruction(ev, wavefront=object(), reconstruct=True)
    with pytest.raises(ValueError, match="need_latents"):
        rec.update_reconstruction(ev, need_latents=False)
    # states do not carry over between precisions, in either direction
    bf16_state = {'xh': [torch.zeros(1, 128, 16, 24, dtype=torch.bfloat16)] * 2, 'cur': 0, 'fresh': False,
                  'cell': torch.zeros(1, 16, 24, 64)}
    fp32_state = {'precision': 'fp32', 'xh': torch.zeros(1, 16, 24, 128), 'cell': torch.zeros(1, 16, 24, 64), 'fresh': False}
    rec.last_states_for_each_channel['grayscale'] = [bf16_state, None, None]
    with pytest.raises(ValueError, match="bf16"):
        rec.update_reconstruction(ev, reconstruct=True)
    with pytest.raises(ValueError, match="bf16"):
        _model().forward_fp32(ev, [bf16_state, None, None])
    rec16 = ImageReconstructor(_model(), 32, 48, 5, torch.device('cpu'))
    rec16.last_states_for_each_channel['grayscale'] = [fp32_state, None, None]
    with pytest.raises(ValueError, match="fp32"):
        rec16.update_reconstruction(ev, reconstruct=True)
    with pytest.raises(ValueError, match="fp32"):
        _model()(ev, [fp32_state, None, None], reconstruct=True)
