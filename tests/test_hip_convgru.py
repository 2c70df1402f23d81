"""K28: the ConvGRU kernels (openess_amd/csrc/convgru.hip), the ConvGRU mirror and a ConvGRU E2VID model end to end.

References: tests/convgru_reference.py (float64 restatement of one step, CPU), tests/convgru_cases.py (operands, the exact cases
and their integer expectations) and tests/golden/e2vid_convgru.npz (the reference's own E2VIDRecurrent with 'convgru' blocks,
tests/golden/gen_golden_convgru.py).  Bounds:
  bf16 launches, fp32 outputs (u, r*h before rounding, master h), each launch on its own operands: the fused ConvLSTM's
    fp32-cell bound (atol = rtol = 2e-2, tests/test_hip_conv.py, test_convlstm_fused_step_matches_torch) is 10^4 times what was
    measured, so the bound is four times the measured maximum instead: measured max |kernel - float64| on MI355X over the four
    geometries u 5.5e-7, r*h 6.7e-7, h 1.58e-6 (largest at 1x110x160x128) -> LAUNCH_BOUND = 6.4e-6 absolute (all values are
    O(1)).  Whole steps from the kernel's own state (a bf16 ulp flip of r*h is charged there: up to 2^-8 |r*h| |w| ~ 2.4e-4
    on a pre-activation) keep 2e-2; measured 3.2e-6.  bf16 outputs equal the bf16 rounding of the fp32 ones bit for bit.
  fp32 step: four times the deviation of torch fp32 on the CPU from float64 (tools/exp_convgru_bounds.py), per geometry.
  whole model: the ConvLSTM golden tests' bounds (tests/test_hip_nets.py: image 2e-2 absolute, latents 3e-2 relative;
    tests/test_hip_e2vid_fp32.py: 1e-4)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import convgru_cases as cases
from tests import convgru_reference as ref
from tests.synth import compact, fill_by_name

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = {'num_bins': 5, 'skip_type': 'sum', 'recurrent_block_type': 'convgru', 'num_encoders': 3,
       'base_num_channels': 32, 'num_residual_blocks': 2, 'use_upsample_conv': False, 'norm': 'BN'}
# tools/exp_convgru_bounds.py, step_fp32_vs_f64: torch fp32 on the CPU against float64; the test allows four times these
F32_CPU_DEV = {(2, 9, 11, 32): 7.199149272274497e-07, (1, 13, 10, 64): 1.263494240844043e-06}
LAUNCH_BOUND = 6.4e-6           # four times the measured maximum (module docstring)
EINVAL = -22


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def bf(t):
    """bf16 rounding, kept in fp32."""
    return t.bfloat16().float()


def nchw(t):
    """[B, H, W, C] device tensor -> fp32 [B, C, H, W] on the CPU."""
    return t.float().permute(0, 3, 1, 2).cpu()


def block(case, C, rounded=True):
    """A ConvGRU mirror on the GPU holding the case's weights (bf16-rounded: what the bf16 kernels multiply)."""
    from openess_amd.e2vid.model.submodules import ConvGRU
    blk = ConvGRU(C, C, 3)
    q = bf if rounded else (lambda t: t)
    with torch.no_grad():
        for gate, n in ((blk.update_gate, 'u'), (blk.reset_gate, 'r'), (blk.out_gate, 'o')):
            gate.weight.copy_(q(case['w' + n]))
            gate.bias.copy_(case['b' + n])
    return blk.cuda()


def weights(blk):
    g = lambda m: (m.weight.detach().cpu(), m.bias.detach().cpu())
    return g(blk.update_gate) + g(blk.reset_gate) + g(blk.out_gate)


def bf16_state(blk, x, h=None, poison=False):
    """A bf16 state with x in its x window; h (fp32 [B, C, H, W]) as the master with its bf16 rounding in the h window, or fresh."""
    from openess_amd import engine
    B, C, H, W = x.shape
    st = blk.new_state(B, H, W, torch.device('cuda'))
    if poison:
        for k in ('hxr', 'h32', 'u'):
            st[k].fill_(float('nan'))
    buf = engine.nhwc(st['hxr'])
    buf[..., C:2 * C] = x.cuda().permute(0, 2, 3, 1).bfloat16()
    if h is not None:
        st['h32'].copy_(h.cuda().permute(0, 2, 3, 1))
        buf[..., :C] = st['h32'].bfloat16()
        st['fresh'] = False
    return st, buf


@pytest.mark.parametrize("geom", cases.GEOMS)
def test_gates_and_output_launch_match_float64(geom):
    """Each launch against float64 on the operands it multiplies (bf16-rounded x, h, weights; the reset gate scales the fp32
    master).  The output launch's reference takes the kernel's own r*h and u, so a one-ulp flip in r*h is not charged twice."""
    B, H, W, C = geom
    c = cases.random_case(*geom)
    blk = block(c, C)
    wu, bu, wr, br, wo, bo = weights(blk)
    x, h = bf(c['x']), c['h']
    st, buf = bf16_state(blk, x, h)
    rh32 = torch.full((B, H, W, C), float('nan'), device='cuda')
    blk.step(st, rh_f32=rh32)
    torch.cuda.synchronize()
    u_ref, rh_ref = ref.gates(x, bf(h), h, wu, bu, wr, br)
    u_k, rh_k, rh_bf = nchw(st['u']), nchw(rh32), nchw(buf[..., 2 * C:])
    h_ref = ref.blend(x, rh_bf, h, u_k, wo, bo)
    h_k, h_bf = nchw(st['h32']), nchw(buf[..., :C])
    dev = {n: float((a.double() - b).abs().max()) for n, a, b in (('u', u_k, u_ref), ('rh', rh_k, rh_ref), ('h', h_k, h_ref))}
    print("convgru bf16 deviation from float64", geom, dev)
    for n, a, b in (('u', u_k, u_ref), ('rh', rh_k, rh_ref), ('h', h_k, h_ref)):
        assert dev[n] <= LAUNCH_BOUND, (n, dev)
    assert torch.equal(buf[..., 2 * C:], rh32.bfloat16())          # the r*h window is the rounding of the fp32 product, bit for bit
    assert torch.equal(buf[..., :C], st['h32'].bfloat16())         # and the bf16 copy of h that of the master
    assert torch.equal(nchw(buf[..., C:2 * C]), x)                 # the x window is read only


@pytest.mark.parametrize("geom", cases.EXACT_GEOMS)
def test_exact_cases_bit_for_bit(geom):
    """One-hot weights of magnitude 256 over every tap, +-128 biases, +-1 operands: u, r in {0, 1} and o in {-1, +1} exactly, so
    every output is an integer computed on the host (cases.exact_expected): indexing pinned bit for bit -- both gates, every
    32-block of channels, the ragged tile, every border, batch index > 0."""
    B, H, W, C = geom
    c = cases.exact_case(*geom)
    _, _, u, rh, _, hn = cases.exact_expected(c)
    blk = block(c, C)
    st, buf = bf16_state(blk, c['x'], c['h'])
    rh32 = torch.full((B, H, W, C), float('nan'), device='cuda')
    blk.step(st, rh_f32=rh32)
    torch.cuda.synchronize()
    assert torch.equal(nchw(st['u']), u.float())
    assert torch.equal(nchw(rh32), rh.float())
    assert torch.equal(nchw(buf[..., 2 * C:]), rh.float())
    assert torch.equal(nchw(st['h32']), hn.float())
    assert torch.equal(nchw(buf[..., :C]), hn.float())
    # the zero-state form (x alone, half the K loop): h = 0 in the integers
    _, _, u0, _, _, hn0 = cases.exact_expected(dict(c, h=torch.zeros_like(c['h'])))
    st0, buf0 = bf16_state(blk, c['x'], None, poison=True)
    blk.step(st0)
    torch.cuda.synchronize()
    assert torch.equal(nchw(st0['u']), u0.float()) and torch.equal(nchw(st0['h32']), hn0.float())
    assert torch.equal(nchw(buf0[..., :C]), hn0.float()) and float(buf0[..., 2 * C:].float().abs().max()) == 0.0


@pytest.mark.parametrize("geom", cases.EXACT_GEOMS)
def test_fp32_pointwise_kernels_exact(geom):
    """oess_convgru_gates_f32 / oess_convgru_blend_f32 alone on the exact cases' integer pre-activations, on the windows of a
    h | x | r*h buffer."""
    from openess_amd import hip
    B, H, W, C = geom
    c = cases.exact_case(*geom)
    pre_u, pre_r, u, rh, pre_o, hn = cases.exact_expected(c)
    nhwc = lambda t: t.float().permute(0, 2, 3, 1).contiguous().cuda()
    buf = torch.full((B, H, W, 3 * C), float('nan'), device='cuda')
    buf[..., :C] = nhwc(c['h'])
    hv, rv = buf[..., :C].permute(0, 3, 1, 2), buf[..., 2 * C:].permute(0, 3, 1, 2)
    pre = torch.cat([nhwc(pre_u), nhwc(pre_r)], 3).contiguous()
    u_k = torch.empty((B, H, W, C), device='cuda')
    hip.convgru_gates_f32(pre, hv, u_k, rv)
    assert torch.equal(nchw(u_k), u.float()) and torch.equal(rv.cpu(), rh.float())
    hip.convgru_blend_f32(nhwc(pre_o), u_k, hv, hv)                # in place in the h window
    assert torch.equal(hv.cpu(), hn.float())
    assert bool(torch.isnan(buf[..., C:2 * C]).all())               # the x window was not touched


@pytest.mark.parametrize("geom", cases.GEOMS[:3])
def test_three_recurrent_steps_from_a_fresh_state(geom):
    """ConvGRU.step three times from a fresh state whose buffers were filled with NaN, against the float64 restatement, which
    continues from the kernel's own state each step (as test_convlstm_fused_step_matches_torch does); the first step equals a
    step from an explicit all-zero state bit for bit and leaves no NaN anywhere."""
    from openess_amd import engine
    B, H, W, C = geom
    c = cases.random_case(*geom)
    blk = block(c, C)
    wu, bu, wr, br, wo, bo = weights(blk)
    x = bf(cases.random_case(*geom, seed=50)['x'])
    st, buf = bf16_state(blk, x, None, poison=True)
    zero, zbuf = bf16_state(blk, x, torch.zeros_like(x))
    assert st['fresh'] and not zero['fresh']
    blk.step(st)
    blk.step(zero)
    torch.cuda.synchronize()
    for k in ('hxr', 'h32', 'u'):
        assert not bool(torch.isnan(st[k].float()).any()), k
        assert torch.equal(st[k], zero[k]), k
    h_prev, hb_prev = torch.zeros_like(x), torch.zeros_like(x)
    for s in range(3):
        if s:
            x = bf(cases.random_case(*geom, seed=50 + s)['x'])
            buf[..., C:2 * C] = x.cuda().permute(0, 2, 3, 1).bfloat16()
            blk.step(st)
        want = ref.step(x, h_prev, wu, bu, wr, br, wo, bo, h_conv=hb_prev, round_rh=bf)[0]
        h_prev, hb_prev = nchw(st['h32']), nchw(engine.nhwc(st['hxr'])[..., :C])
        d = float((h_prev.double() - want).abs().max())
        print("convgru three steps", geom, s, d)
        assert torch.allclose(h_prev.double(), want, atol=2e-2, rtol=2e-2), (s, d)
        assert torch.equal(hb_prev, bf(h_prev))


@pytest.mark.parametrize("geom", cases.GEOMS_F32)
def test_step_f32_matches_float64(geom):
    """ConvGRU.step_f32 over three steps against float64 from the kernel's own fp32 state; bound: four times torch fp32's own
    deviation on the CPU on these cases (tools/exp_convgru_bounds.py)."""
    B, H, W, C = geom
    c = cases.random_case(*geom)
    blk = block(c, C, rounded=False)
    wu, bu, wr, br, wo, bo = weights(blk)
    st = blk.new_state_f32(B, H, W, torch.device('cuda'))
    st['hxr'].fill_(float('nan'))
    h_prev = torch.zeros_like(c['x'])
    bound = 4 * F32_CPU_DEV[geom]
    for s in range(3):
        x = cases.random_case(*geom, seed=77 + s)['x']
        blk.x_window(st).copy_(x.cuda())
        h = blk.step_f32(st)
        want = ref.step(x, h_prev, wu, bu, wr, br, wo, bo)[0]
        h_prev = h.cpu().contiguous()
        d = float((h_prev.double() - want).abs().max())
        print("convgru fp32 step", geom, s, d, "bound", bound)
        assert d <= bound, (s, d, bound)
    assert not bool(torch.isnan(st['hxr']).any())


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLDEN, "e2vid_convgru.npz")))


def golden_sub(g, key):
    return g[key + "__sub"] if key + "__sub" in g else compact(g[key])[0]


def model():
    from openess_amd.e2vid.model.model import E2VIDRecurrent
    m = E2VIDRecurrent(CFG).eval()
    fill_by_name(m, 11)
    return m.cuda()


def test_model_bf16_matches_reference_golden(g):
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor
    m = model()
    assert sorted(m.state_dict().keys()) == list(g["keys"])
    ev = torch.from_numpy(g["events"]).cuda()
    rec = ImageReconstructor(m, 32, 48, 5, torch.device("cuda"))
    for i in range(3):
        img, states, latent = rec.update_reconstruction(ev[:, 5 * i:5 * i + 5], reconstruct=True)
    assert img.shape == (2, 1, 32, 48) and img.dtype == torch.float32
    d_img = float(np.abs(img.cpu().numpy() - g["img"]).max())
    errs = {k: relerr(compact(latent[k].float().cpu().numpy())[0], golden_sub(g, f"latent{k}")) for k in (1, 2, 4, 8)}
    print("convgru model bf16: image", d_img, "latents", errs)
    assert d_img < 2e-2
    for k in (1, 2, 4, 8):
        assert tuple(latent[k].shape) == tuple(g[f"latent{k}__shape"] if f"latent{k}__shape" in g else g[f"latent{k}"].shape)
        assert errs[k] < 3e-2, k
    # the skew / fused-head request (need_latents=False on the calls whose latents are dropped) takes the plain order for a
    # ConvGRU model: same latents, bit for bit, no level left behind
    plain, asked = [ImageReconstructor(m, 32, 48, 5, torch.device("cuda")) for _ in range(2)]
    for i in range(3):
        _, _, lat_p = plain.update_reconstruction(ev, channel_slice=(5 * i, 5))
        _, st_a, lat_a = asked.update_reconstruction(ev, channel_slice=(5 * i, 5), need_latents=(i == 2))
    assert isinstance(st_a, list) and len(st_a) == 3
    for k in (1, 2, 4, 8):
        assert torch.equal(lat_p[k], lat_a[k]), k
    assert not m.unetrecurrent.events_fusable(ev, 5)
    # raw= handed over all the same (no caller does: events_fusable is False): plain order, same values
    x0 = rec.event_preprocessor.slice_to_nhwc8(ev, 0, 5)
    _, st_x, lat_x = m(x0, None)
    _, st_r, lat_r = m(None, None, need_head=False, raw=(ev, 0, 5, True), skew=True)
    for k in (1, 2, 4, 8):
        assert torch.equal(lat_x[k], lat_r[k]), k
    assert all(torch.equal(a['h32'], b['h32']) for a, b in zip(st_x, st_r))
    # a ConvLSTM state is refused
    from openess_amd.e2vid.model.model import E2VID_LIGHTWEIGHT_CONFIG, E2VIDRecurrent
    lstm = E2VIDRecurrent(E2VID_LIGHTWEIGHT_CONFIG).eval().cuda()
    x = rec.event_preprocessor.slice_to_nhwc8(ev, 0, 5)
    _, lstm_states, _ = lstm(x, None)
    with pytest.raises(ValueError, match="convlstm state"):
        m(x, lstm_states)
    with pytest.raises(ValueError, match="convgru state"):
        lstm(x, st_a)


def test_model_wavefront_request_matches_plain_order(g):
    """update_reconstruction forwards wavefront= for any model (the pre-training step does, between begin() and end()).  A
    ConvGRU model has no wavefront schedule: the reconstructor keeps everything, the slice kernel included, on the current stream,
    and a direct caller of forward that prepared x on the wavefront's level-0 stream is ordered behind it.  Same latents and
    states as the plain sequence, bit for bit, over a sequence that reuses the slice's allocation."""
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor
    from openess_amd.e2vid.wavefront import EncoderWavefront
    m = model()
    dev = torch.device("cuda")
    ev = torch.from_numpy(g["events"]).cuda()
    ev = torch.cat([ev, ev.flip(1)[:, :10] * 0.5], 1).contiguous()            # 5 sub-windows
    plain, asked = ImageReconstructor(m, 32, 48, 5, dev), ImageReconstructor(m, 32, 48, 5, dev)
    for i in range(5):
        _, st_p, lat_p = plain.update_reconstruction(ev, channel_slice=(5 * i, 5), need_latents=(i == 4))
    wf = EncoderWavefront(dev, m.num_encoders)
    wf.begin()
    for i in range(5):
        _, st_a, lat_a = asked.update_reconstruction(ev, channel_slice=(5 * i, 5), wavefront=wf, need_latents=(i == 4))
    wf.end(*lat_a.values())
    for k in (1, 2, 4, 8):
        assert torch.equal(lat_p[k], lat_a[k]), k
    for a, b in zip(st_p, st_a):
        assert torch.equal(a['h32'], b['h32']) and torch.equal(a['hxr'], b['hxr'])
    # forward itself, x prepared on the level-0 stream as the ConvLSTM schedule has it
    states, direct = None, None
    wf.begin()
    for i in range(5):
        with torch.cuda.stream(wf.streams[0]):
            x = plain.event_preprocessor.slice_to_nhwc8(ev, 5 * i, 5)
        _, states, direct = m(x, states, wavefront=wf, need_head=(i == 4), skew=True)
        del x
    wf.end(*direct.values())
    for k in (1, 2, 4, 8):
        assert torch.equal(lat_p[k], direct[k]), k


def test_model_fp32_matches_reference_golden(g):
    from types import SimpleNamespace
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor
    m = model()
    ev = torch.from_numpy(g["events"]).cuda()
    rec = ImageReconstructor(m, 32, 48, 5, torch.device("cuda"), SimpleNamespace(precision='fp32'))
    for i in range(3):
        img, states, latent = rec.update_reconstruction(ev[:, 5 * i:5 * i + 5], reconstruct=True)
    d_img = float(np.abs(img.cpu().numpy() - g["img"]).max())
    e8 = relerr(compact(latent[8].cpu().numpy())[0], golden_sub(g, "latent8"))
    es = []
    for i, st in enumerate(states):
        C = st['hxr'].shape[3] // 3
        es.append(relerr(compact(nchw(st['hxr'][..., :C]).numpy())[0], golden_sub(g, f"state{i}")))
    print("convgru model fp32: image", d_img, "latent8", e8, "states", es)
    assert d_img <= 1e-4 and e8 <= 1e-4
    assert all(e <= 1e-4 for e in es), es
    # a bf16 state is refused by the fp32 step
    bf16 = ImageReconstructor(m, 32, 48, 5, torch.device("cuda"))
    _, st16, _ = bf16.update_reconstruction(ev[:, :5])
    with pytest.raises(ValueError, match="bf16"):
        m.forward_fp32(ev[:, :5].contiguous(), st16)


def _gates_args(buf, C, w, u, rh, Cin=None, in_=None, k=3, pad=1, h_prev=None, stride=None):
    B, H, W, C3 = buf.shape
    in_ = buf if in_ is None else in_
    return (in_.data_ptr(), C3 if stride is None else stride, B, H, W, 2 * C if Cin is None else Cin, w.data_ptr(), None, C, k, k, pad,
            h_prev, u.data_ptr(), rh.data_ptr(), C3, None, None)


def test_entry_points_refuse_before_any_launch():
    """OESS_EINVAL and untouched outputs: an output inside the convolved window, C % 32 != 0, input_size != hidden_size, a 5 x 5
    gate, null pointers."""
    from openess_amd import _lib
    lib = _lib.load()
    B, H, W, C = 1, 6, 7, 32
    dev = 'cuda'
    buf = torch.zeros(B, H, W, 3 * C, device=dev, dtype=torch.bfloat16)
    w = torch.zeros(128 * 9 * 2 * C * 4, device=dev, dtype=torch.bfloat16)
    u = torch.full((B, H, W, 2 * C), 7.0, device=dev)
    h = torch.full((B, H, W, 2 * C), 5.0, device=dev)
    rh, inside = buf[..., 2 * C:], buf[..., C:2 * C]
    ok = _gates_args(buf, C, w, u, rh)
    bad = {
        'rh inside the window': _gates_args(buf, C, w, u, inside),
        'u inside the window': _gates_args(buf, C, w, buf, rh),
        'C % 32': _gates_args(buf, 48, w, u, rh),
        'input_size != hidden_size': _gates_args(buf, C, w, u, rh, Cin=2 * C + 8),
        '5 x 5': _gates_args(buf, C, w, u, rh, k=5, pad=2),
        'pad 0': _gates_args(buf, C, w, u, rh, pad=0),
        'null in': (None,) + ok[1:],
        'null weights': ok[:6] + (None,) + ok[7:],
        'null u': ok[:13] + (None,) + ok[14:],
        'null rh': ok[:14] + (None,) + ok[15:],
        'x alone with a previous state': _gates_args(buf, C, w, u, rh, Cin=C, in_=inside, h_prev=h.data_ptr()),
        'pixel stride % 8': _gates_args(buf, C, w, u, rh, stride=3 * C + 4),
    }
    for name, args in bad.items():
        assert lib.oess_convgru_gates_bf16(*args) == EINVAL, name
    hb = buf[..., :C]
    out_ok = (buf[..., C:].data_ptr(), 3 * C, B, H, W, 2 * C, w.data_ptr(), None, C, 3, 3, 1, u.data_ptr(), h.data_ptr(), h.data_ptr(),
              hb.data_ptr(), 3 * C, None)
    bad_out = {
        'h_bf16 inside the window': out_ok[:15] + (inside.data_ptr(),) + out_ok[16:],
        'h overlaps u': out_ok[:14] + (u.data_ptr(),) + out_ok[15:],
        'h overlaps h_prev without being it': out_ok[:14] + (h.data_ptr() + 16,) + out_ok[15:],
        'C % 32': out_ok[:8] + (48,) + out_ok[9:],
        'input_size != hidden_size': out_ok[:5] + (2 * C + 8,) + out_ok[6:],
        '5 x 5': out_ok[:9] + (5, 5, 2) + out_ok[12:],
        'null u': out_ok[:12] + (None,) + out_ok[13:],
        'null h': out_ok[:14] + (None,) + out_ok[15:],
        'null h_bf16': out_ok[:15] + (None,) + out_ok[16:],
    }
    for name, args in bad_out.items():
        assert lib.oess_convgru_out_bf16(*args) == EINVAL, name
    # fp32 pointwise entries: an output on an input, null pointers
    f = torch.full((B, H, W, 3 * C), 3.0, device=dev)
    V = lambda t: _lib.F32View(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2), t.stride(3))
    pre = torch.full((B, H, W, 2 * C), 1.0, device=dev)
    vh, vr, vx = V(f[..., :C]), V(f[..., 2 * C:]), V(f[..., C - 8:2 * C - 8])
    u32 = u[..., :C].contiguous()
    r = ctypes.byref
    assert lib.oess_convgru_gates_f32(pre.data_ptr(), r(vh), B, H, W, C, u32.data_ptr(), r(vx), None) == EINVAL     # rh straddles h
    assert lib.oess_convgru_gates_f32(pre.data_ptr(), r(vh), B, H, W, C, pre.data_ptr(), r(vr), None) == EINVAL     # u on pre
    assert lib.oess_convgru_gates_f32(None, r(vh), B, H, W, C, u32.data_ptr(), r(vr), None) == EINVAL
    assert lib.oess_convgru_gates_f32(pre.data_ptr(), r(vh), B, H, W, C, u32.data_ptr(), None, None) == EINVAL
    assert lib.oess_convgru_blend_f32(pre.data_ptr(), u32.data_ptr(), r(vh), B, H, W, C, r(vx), None) == EINVAL      # h straddles h_prev
    assert lib.oess_convgru_blend_f32(pre.data_ptr(), None, r(vh), B, H, W, C, r(vh), None) == EINVAL
    assert lib.oess_convgru_f32_workspace_bytes(0, C) == 0 and lib.oess_convgru_f32_workspace_bytes(10, C) == 10 * 4 * C * 4
    torch.cuda.synchronize()
    assert float(buf.float().abs().max()) == 0.0 and bool((u == 7.0).all()) and bool((h == 5.0).all())
    assert bool((f == 3.0).all()) and bool((pre == 1.0).all())
    # the model mirror reports a geometry the kernels do not take instead of falling back
    from openess_amd.e2vid.model.submodules import ConvGRU
    odd = ConvGRU(48, 48, 3).cuda()
    st = odd.new_state(1, 4, 4, torch.device(dev))
    st['hxr'].zero_()
    with pytest.raises(RuntimeError, match="oess_convgru_gates_bf16"):
        odd.step(st)


def test_offline_reconstruction_both_precisions(tmp_path):
    """reconstruct() on a small synthetic event file with a seeded ConvGRU model: frames of the sensor's shape in both
    precisions.  Bound between the two: tests/test_hip_e2vid_fp32.py has no assertion between the precisions of a model (its
    CLI case holds the fp32 frames to the fp32 oracle), so the bound is put together from the two golden bounds this file
    already applies to this network: the bf16 image is within 2e-2 of the reference (tests/test_hip_nets.py,
    test_e2vid_offline_reconstruction_image) and the fp32 image within 1e-4 (tests/test_hip_e2vid_fp32.py,
    test_fp32_matches_reference_golden_nets), so the two differ by at most 2.01e-2 of the grey scale = 5.13 levels, plus one for
    the two roundings to uint8: 6 levels."""
    from openess_amd.e2vid import run_reconstruction as rr
    rng = np.random.default_rng(5)
    W, H, n = 48, 32, 6000
    t = np.sort(rng.uniform(0.0, 0.2, n))
    ev = np.stack([t, rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n)], 1)
    path = str(tmp_path / "events.txt")
    with open(path, "w") as f:
        f.write(f"{W} {H}\n")
        for r in ev:
            f.write("%.9f %d %d %d\n" % (r[0], r[1], r[2], r[3]))
    frames = {}
    for precision in ('bf16', 'fp32'):
        frames[precision] = rr.reconstruct(path, model(), str(tmp_path / precision), window_size=2000, precision=precision)
        assert len(frames[precision]) == 3
        assert all(f.shape == (H, W) and f.dtype == np.uint8 for f in frames[precision])
        assert os.path.exists(os.path.join(str(tmp_path / precision), "frame_0000000002.png"))
    d = max(int(np.abs(a.astype(np.int64) - b.astype(np.int64)).max()) for a, b in zip(frames['bf16'], frames['fp32']))
    print("convgru offline bf16 vs fp32, grey levels", d)
    assert d <= 6
