"""GPU tests of the fp32 E2VID inference path (K14, openess_amd/csrc/conv_f32.hip): every kernel against float64 torch on the
CPU, the whole network against the reference's own goldens and the fp32 CPU oracle at fp32 tolerance (the bf16 path misses
these bounds by two orders of magnitude), the CLI end to end, repeatability and the absence of host synchronisation."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nets as on
from oracle.step import E2VID_LIGHTWEIGHT_CONFIG
from tests.synth import compact, fill_by_name

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _act64(y, act):
    return torch.relu(y) if act == 'relu' else torch.sigmoid(y) if act == 'sigmoid' else y


# geometry: (B, Cin, H, W, Cout, k, stride, act, with x2, with residual, input layout)
CONV_CASES = {
    "head_5x5_s1_cin5": (2, 5, 17, 23, 32, 5, 1, 'relu', False, False, 'nchw'),
    "enc_5x5_s2": (2, 32, 19, 25, 64, 5, 2, 'relu', False, False, 'cl'),
    "gates_3x3_s1": (1, 128, 15, 21, 256, 3, 1, None, False, False, 'cl'),
    "res_3x3_residual": (2, 64, 9, 13, 64, 3, 1, 'relu', False, True, 'cl'),
    "pred_1x1_cout1_skip": (2, 32, 11, 7, 1, 1, 1, 'sigmoid', True, False, 'cl'),
    "enc0_640x480": (1, 32, 480, 640, 64, 5, 2, 'relu', False, False, 'cl'),
}


@pytest.mark.parametrize("case", sorted(CONV_CASES))
def test_conv2d_f32_matches_float64(case):
    from openess_amd import hip
    B, Cin, H, W, Cout, k, st, act, two, res, layout = CONV_CASES[case]
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    x = torch.randn(B, Cin, H, W, generator=g)
    x2 = torch.randn(B, Cin, H, W, generator=g) if two else None
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    b = torch.randn(Cout, generator=g)
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    r = torch.randn(B, Cout, Ho, Wo, generator=g) if res else None
    dev = (lambda t: t.cuda()) if layout == 'nchw' else _cl
    y = hip.conv2d_f32(dev(x), hip.pack_conv_weight_f32(w.cuda()), b.cuda(), Cout, k, k, st, pad, act=act,
                       x2=None if x2 is None else dev(x2), residual=None if r is None else _cl(r))
    xin = x.double() + (x2.double() if two else 0)
    want = F.conv2d(xin, w.double(), b.double(), st, pad)
    if res:
        want = want + r.double()
    want = _act64(want, act)
    assert y.shape == want.shape
    assert relerr(y.cpu().numpy(), want.numpy()) <= 1e-5


@pytest.mark.parametrize("B,Cin,H,W,Cout", [(2, 64, 7, 9, 32), (1, 256, 5, 6, 128)])
def test_conv_transpose2d_f32_matches_float64(B, Cin, H, W, Cout):
    from openess_amd import hip
    g = torch.Generator().manual_seed(B * 100 + Cin)
    x, skip = torch.randn(B, Cin, H, W, generator=g), torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cin, Cout, 5, 5, generator=g) / (Cin * 6.25) ** 0.5
    b = torch.randn(Cout, generator=g)
    y = hip.conv_transpose2d_f32(_cl(x), hip.pack_conv_transpose_weight_f32(w.cuda()), b.cuda(), Cout, act='relu', x2=_cl(skip))
    want = torch.relu(F.conv_transpose2d(x.double() + skip.double(), w.double(), b.double(), 2, 2, 1))
    assert y.shape == want.shape == (B, Cout, 2 * H, 2 * W)
    assert relerr(y.cpu().numpy(), want.numpy()) <= 1e-5


@pytest.mark.parametrize("B,Cin,H,W,Cout", [(2, 64, 6, 10, 32), (1, 128, 5, 7, 64)])
def test_upsample_conv_f32_matches_float64(B, Cin, H, W, Cout):
    from openess_amd import hip
    g = torch.Generator().manual_seed(B * 7 + Cin)
    x, skip = torch.randn(B, Cin, H, W, generator=g), torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 5, 5, generator=g) / (Cin * 25) ** 0.5
    b = torch.randn(Cout, generator=g)
    y = hip.conv2d_f32(_cl(x), hip.pack_conv_weight_f32(w.cuda()), b.cuda(), Cout, 5, 5, 1, 2, act='relu', x2=_cl(skip),
                       upsample2x=True)
    up = F.interpolate(x.double() + skip.double(), scale_factor=2, mode='bilinear', align_corners=False)
    want = torch.relu(F.conv2d(up, w.double(), b.double(), 1, 2))
    assert y.shape == want.shape == (B, Cout, 2 * H, 2 * W)
    assert relerr(y.cpu().numpy(), want.numpy()) <= 1e-5


def test_convlstm_step_f32_matches_float64():
    """Two steps from a zero state (the first convolves the x half only) against the reference formula in float64."""
    from openess_amd.e2vid.model.submodules import RecurrentConvLayer
    torch.manual_seed(5)
    layer = RecurrentConvLayer(32, 64, kernel_size=5, stride=2, padding=2).eval()
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(torch.randn_like(p) / (p[0].numel() ** 0.5 if p.dim() > 1 else 4.0))
    xs = [torch.randn(2, 32, 21, 27) for _ in range(2)]
    layer.cuda()
    st = None
    got = []
    for x in xs:
        h, st = layer.forward_f32(_cl(x), st)
        got.append((h.cpu().numpy().copy(), st['cell'].permute(0, 3, 1, 2).cpu().numpy().copy()))
    c, G = layer.conv.conv2d, layer.recurrent_block.Gates
    h64 = c64 = None
    for i, x in enumerate(xs):
        with torch.no_grad():
            y = torch.relu(F.conv2d(x.double(), c.weight.double().cpu(), c.bias.double().cpu(), 2, 2))
            gates = F.conv2d(torch.cat([y, h64 if h64 is not None else torch.zeros_like(y)], 1), G.weight.double().cpu(),
                             G.bias.double().cpu(), padding=1)
        if h64 is None:
            h64, c64 = torch.zeros_like(y), torch.zeros_like(y)
        i_, f_, o_, g_ = gates.chunk(4, 1)
        c64 = torch.sigmoid(f_) * c64 + torch.sigmoid(i_) * torch.tanh(g_)
        h64 = torch.sigmoid(o_) * torch.tanh(c64)
        assert relerr(got[i][0], h64.numpy()) <= 1e-5, i
        assert relerr(got[i][1], c64.numpy()) <= 1e-5, i


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLDEN, "nets.npz")))


@pytest.fixture(scope="module")
def keys():
    return json.load(open(os.path.join(GOLDEN, "nets_keys.json")))


@pytest.fixture(scope="module")
def gpre():
    return dict(np.load(os.path.join(GOLDEN, "e2vid_pre.npz")))


def _fp32_reconstructor(H, W, seed=11, cfg=None, options=None):
    from types import SimpleNamespace
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor
    from openess_amd.e2vid.model.model import E2VIDRecurrent
    m = E2VIDRecurrent(cfg or E2VID_LIGHTWEIGHT_CONFIG).eval()
    fill_by_name(m, seed)
    m.cuda()
    opts = SimpleNamespace(precision='fp32', **(options or {}))
    return m, ImageReconstructor(m, H, W, m.num_bins, torch.device("cuda"), opts)


def test_fp32_matches_reference_golden_nets(g):
    _, rec = _fp32_reconstructor(32, 48)
    ev = torch.from_numpy(g["e2vid_events"]).cuda()
    for i in range(3):
        img, _, latent = rec.update_reconstruction(ev[:, 5 * i:5 * i + 5], reconstruct=True)
    assert img.shape == (2, 1, 32, 48) and img.dtype == torch.float32
    assert np.abs(img.cpu().numpy() - g["e2vid_img"]).max() <= 1e-4
    sub, _, _ = compact(latent[8].cpu().numpy())
    refsub = g["e2vid_latent8__sub"] if "e2vid_latent8__sub" in g else compact(g["e2vid_latent8"])[0]
    assert relerr(sub, refsub) <= 1e-4


def test_fp32_with_padding_matches_reference_golden(gpre):
    _, rec = _fp32_reconstructor(30, 44)
    assert rec.crop.needs_pad
    ev = torch.from_numpy(gpre["rec_events"]).cuda()
    for i in range(3):
        img, states, latent = rec.update_reconstruction(ev[:, 5 * i:5 * i + 5], reconstruct=True)
    for k in (1, 2, 4, 8):
        got = latent[k].cpu().numpy()
        assert got.shape == gpre[f"rec_latent_{k}"].shape and latent[k].dtype == torch.float32
        assert relerr(got, gpre[f"rec_latent_{k}"]) <= 1e-4, k
    c2 = states[2]['cell'].permute(0, 3, 1, 2).cpu().numpy()
    assert c2.shape == gpre["rec_state_c_2"].shape and relerr(c2, gpre["rec_state_c_2"]) <= 1e-4
    want = gpre["rec_img"]
    got = img.cpu().numpy()
    if got.shape != want.shape:
        cp = rec.crop
        want = want[:, :, cp.iy0:cp.iy1, cp.ix0:cp.ix1]
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-4
    # the fused channel-slice form feeds the network the same values
    _, rec2 = _fp32_reconstructor(30, 44)
    for i in range(3):
        img2, _, _ = rec2.update_reconstruction(ev.contiguous(), channel_slice=(5 * i, 5), reconstruct=True)
    assert torch.equal(img2, img)


def test_fp32_larger_size_matches_oracle(keys):
    """1 x 5 x 180 x 240 (padded to 184 x 240), three recurrent steps, against the fp32 CPU oracle."""
    _, rec = _fp32_reconstructor(180, 240)
    torch.manual_seed(4)
    evs = [(torch.randn(1, 5, 180, 240) * (torch.rand(1, 5, 180, 240) > 0.8)) for _ in range(3)]
    ref = on.E2VIDRecurrent(E2VID_LIGHTWEIGHT_CONFIG, full=True).eval()
    fill_by_name(ref, 11, keys["e2vid"])
    st = None
    for ev in evs:
        img, _, _ = rec.update_reconstruction(ev.cuda(), reconstruct=True)
        with torch.no_grad():
            img_ref, st, _ = ref(rec.crop.pad(on.event_preprocess(ev)), st)
    cp = rec.crop
    want = img_ref[:, :, cp.iy0:cp.iy1, cp.ix0:cp.ix1].numpy()
    got = img.cpu().numpy()
    assert got.shape == (1, 1, 184, 240)
    assert np.abs(got[:, :, cp.iy0:cp.iy1, cp.ix0:cp.ix1] - want).max() <= 1e-4


def _torch_unet_fp32(m, x, states):
    """UNetRecurrent (norm None, skip_sum, UpsampleConvLayer decoders) written out in torch fp32 (unet.py:146-170 and
    submodules.py of the reference)."""
    u = m.unetrecurrent

    def conv(c, t):
        return F.conv2d(t, c.weight, c.bias, c.stride, c.padding)
    head = torch.relu(conv(u.head.conv2d, x))
    h, blocks, new = head, [], []
    for i, e in enumerate(u.encoders):
        y = torch.relu(conv(e.conv.conv2d, h))
        hp, cp = states[i] if states is not None else (torch.zeros_like(y), torch.zeros_like(y))
        i_, f_, o_, g_ = conv(e.recurrent_block.Gates, torch.cat([y, hp], 1)).chunk(4, 1)
        c = torch.sigmoid(f_) * cp + torch.sigmoid(i_) * torch.tanh(g_)
        h = torch.sigmoid(o_) * torch.tanh(c)
        blocks.append(h)
        new.append((h, c))
    for rb in u.resblocks:
        h = torch.relu(conv(rb.conv2, torch.relu(conv(rb.conv1, h))) + h)
    for i, d in enumerate(u.decoders):
        up = F.interpolate(h + blocks[u.num_encoders - i - 1], scale_factor=2, mode='bilinear', align_corners=False)
        h = torch.relu(conv(d.conv2d, up))
    return torch.sigmoid(conv(u.pred.conv2d, h + head)), new


def test_fp32_upsample_conv_checkpoint_matches_torch():
    """A checkpoint config with use_upsample_conv: True (the reference's default) and norm None."""
    cfg = dict(E2VID_LIGHTWEIGHT_CONFIG, use_upsample_conv=True, norm=None, num_residual_blocks=1)
    m, rec = _fp32_reconstructor(32, 48, seed=7, cfg=cfg)
    ref = type(m)(cfg).eval()
    ref.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    torch.manual_seed(8)
    st = None
    for _ in range(2):
        ev = torch.randn(1, 5, 32, 48) * (torch.rand(1, 5, 32, 48) > 0.7)
        img, _, _ = rec.update_reconstruction(ev.cuda(), reconstruct=True)
        with torch.no_grad():
            want, st = _torch_unet_fp32(ref, on.event_preprocess(ev), st)
    assert img.shape == want.shape
    assert np.abs(img.cpu().numpy() - want.numpy()).max() <= 1e-4


def _events_file(tmp_path):
    rng = np.random.default_rng(5)
    W, H, n = 48, 32, 6000
    t = np.sort(rng.uniform(0.0, 0.2, n))
    ev = np.stack([t, rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n)], 1)
    path = str(tmp_path / "events.txt")
    with open(path, "w") as f:
        f.write(f"{W} {H}\n")
        for r in ev:
            f.write("%.9f %d %d %d\n" % (r[0], r[1], r[2], r[3]))
    return path, W, H


def _oracle_images(path, W, H, model):
    from oracle import events as oe
    ref = on.E2VIDRecurrent(E2VID_LIGHTWEIGHT_CONFIG, full=True).eval()
    fill_by_name(ref, 11, sorted(model.state_dict().keys()))
    st, out = None, []
    ev_read = np.loadtxt(path, skiprows=1)
    with torch.no_grad():
        for k in range(3):
            grid = torch.from_numpy(oe.e2vid_voxel_grid(ev_read[k * 2000:(k + 1) * 2000].copy(), 5, W, H))[None]
            img, st, _ = ref(on.event_preprocess(grid), st)
            out.append(img)
    return out


def _agree(got, want):
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    return d.max() <= 1 and (d == 0).mean() >= 0.999


def test_run_reconstruction_cli_fp32_end_to_end(tmp_path):
    from openess_amd.e2vid import run_reconstruction as rr
    from openess_amd.e2vid.image_reconstructor import PostProcessor
    path, W, H = _events_file(tmp_path)
    torch.manual_seed(1205)
    want = None
    for post in (False, True):
        out = str(tmp_path / ("pp" if post else "plain"))
        import openess_amd.e2vid.run_reconstruction as mod
        orig = mod.load_model

        def load(p):
            m = orig(p)
            fill_by_name(m, 11)
            return m
        mod.load_model = load
        try:
            argv = ["-c", "random", "-i", path, "-o", out, "-N", "2000", "--precision", "fp32"] + (["--postprocess"] if post else [])
            frames = rr.main(argv)
        finally:
            mod.load_model = orig
        assert len(frames) == 3 and frames[0].shape == (H, W) and frames[0].dtype == np.uint8
        from PIL import Image
        png = [np.asarray(Image.open(os.path.join(out, "reconstruction", f"frame_{k:010d}.png"))) for k in range(3)]
        if want is None:
            want = _oracle_images(path, W, H, load("random"))
        for k in range(3):
            assert np.array_equal(png[k], frames[k])
            if post:
                ref = PostProcessor(torch.device("cuda")).process_u8(want[k].cuda())[0].cpu().numpy()
            else:
                ref = (want[k][0, 0].clamp(0, 1) * 255.0).round().to(torch.uint8).numpy()
            assert _agree(frames[k], ref), k


def test_fp32_repeatable_and_sync_free(g):
    ev = torch.from_numpy(g["e2vid_events"]).cuda()
    outs = []
    for _ in range(2):
        _, rec = _fp32_reconstructor(32, 48)
        for i in range(3):
            img, states, latent = rec.update_reconstruction(ev[:, 5 * i:5 * i + 5], reconstruct=True)
        outs.append((img.clone(), latent[8].clone(), states[1]['cell'].clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # a frame of the fp32 path makes no host synchronisation (weights already packed by the frames above)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        rec.update_reconstruction(ev[:, 0:5], reconstruct=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ exact view / geometry surface
# Integer operands (activations in [-2, 2], weights in {-1, 0, 1}, integer bias and residual) make every product and partial sum
# of a v_mfma_f32_32x32x2_f32 chain an integer far below 2^24: the fp32 result is exact in any order and is compared with the
# float64 CPU reference by torch.equal.  The bilinear x2 weights are 0, 1/4, 3/4 and 1, so upsampled integers stay exact too.

def _iv(g, shape, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _nonzero_floors(pre, want):
    """conditions on the reference alone, so that equality is not vacuous: at least half of the pre-activation reference is
    non-zero, and (a ReLU zeroes the negative half of a symmetric result) at least a quarter of what is compared"""
    assert float(want.abs().max()) < 2 ** 24
    assert float((pre != 0).double().mean()) >= 0.5 and float((want != 0).double().mean()) >= 0.25


def _place(t, layout):
    """logical [B, C, H, W] CPU tensor -> CUDA tensor of the same logical shape stored as `layout`"""
    B, C, H, W = t.shape
    nhwc = t.permute(0, 2, 3, 1).cuda()
    if layout == 'cl':
        return _cl(t)
    if layout == 'nchw':
        return t.cuda().contiguous()
    if layout == 'crop':            # a window of a larger NHWC map
        big = torch.full((B, H + 5, W + 4, C), 9.0, device="cuda")
        big[:, 2:2 + H, 3:3 + W] = nhwc
        return big[:, 2:2 + H, 3:3 + W].permute(0, 3, 1, 2)
    if layout == 'off4':            # dense NHWC whose base is 4 bytes off 16-byte alignment
        v = torch.zeros(t.numel() + 1, device="cuda")[1:].view(B, H, W, C)
        v.copy_(nhwc)
        assert v.data_ptr() % 16 == 4
        return v.permute(0, 3, 1, 2)
    if layout == 'slice':           # a channel slice of a wider NHWC buffer
        big = torch.full((B, H, W, C + 8), 9.0, device="cuda")
        big[..., 4:4 + C] = nhwc
        return big[..., 4:4 + C].permute(0, 3, 1, 2)
    raise ValueError(layout)


def _out_view(layout, B, C, H, W):
    """(out argument, buffer to check for untouched neighbours)"""
    if layout is None:
        return None, None
    if layout == 'nchw':
        return torch.full((B, C, H, W), float("nan"), device="cuda"), None
    big = torch.full((B, H, W, C + 8), -7.0, device="cuda")
    return big[..., 4:4 + C].permute(0, 3, 1, 2), big


def _neighbours_untouched(big, C):
    return big is None or (bool((big[..., :4] == -7.0).all()) and bool((big[..., 4 + C:] == -7.0).all()))


# (B, Cin, H, W, Cout, R, S, stride, pad, act, x layout, x2 layout, residual layout, output layout)
EXACT_CONV_CASES = {
    "k3x5_pad0_cin12_cout33": (2, 12, 9, 11, 33, 3, 5, 1, 0, 'relu', 'cl', None, None, None),
    "k1x5_pad0_cin24_cout65_nchw_out": (1, 24, 7, 12, 65, 1, 5, 1, 0, None, 'cl', None, None, 'nchw'),
    "k3x3_pad2_cin1_cout3_nchw": (2, 1, 6, 7, 3, 3, 3, 1, 2, 'relu', 'nchw', None, 'nchw', None),
    "k5x5_pad4_cin12": (1, 12, 5, 6, 33, 5, 5, 1, 4, None, 'cl', None, None, None),
    "s2_pad0_even": (1, 12, 10, 12, 33, 3, 3, 2, 0, None, 'cl', None, None, None),
    "s2_pad0_odd_3x5_res_nchw_out_slice": (2, 24, 9, 13, 65, 3, 5, 2, 0, 'relu', 'cl', None, 'nchw', 'slice'),
    "crop_window_cin16_out_slice": (2, 16, 8, 9, 32, 3, 3, 1, 1, 'relu', 'crop', None, None, 'slice'),
    "crop_window_cin12_cout3": (1, 12, 8, 9, 3, 3, 3, 1, 1, None, 'crop', None, None, None),
    "x2_base_off_alignment": (2, 16, 7, 9, 65, 3, 3, 1, 1, 'relu', 'cl', 'off4', 'cl', 'nchw'),
    "nchw_in_cin24": (1, 24, 6, 8, 33, 3, 3, 1, 1, None, 'nchw', 'nchw', None, 'nchw'),
    "slice_in_cin16_s2": (1, 16, 7, 7, 65, 3, 3, 2, 0, 'relu', 'slice', 'cl', None, None),
}


@pytest.mark.parametrize("case", sorted(EXACT_CONV_CASES))
def test_conv2d_f32_views_and_geometry_exact(case):
    from openess_amd import hip
    B, Cin, H, W, Cout, R, S, st, pad, act, xl, x2l, rl, ol = EXACT_CONV_CASES[case]
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    x = _iv(g, (B, Cin, H, W))
    x2 = _iv(g, (B, Cin, H, W)) if x2l else None
    w = _iv(g, (Cout, Cin, R, S), -1, 1)
    b = _iv(g, (Cout,))
    Ho, Wo = (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1
    r = _iv(g, (B, Cout, Ho, Wo)) if rl else None
    pre = F.conv2d(x.double() + (x2.double() if x2l else 0), w.double(), b.double(), st, pad) + (r.double() if rl else 0)
    want = _act64(pre, act)
    assert want.shape == (B, Cout, Ho, Wo)
    _nonzero_floors(pre, want)
    out, big = _out_view(ol, B, Cout, Ho, Wo)
    y = hip.conv2d_f32(_place(x, xl), hip.pack_conv_weight_f32(w.cuda()), b.cuda(), Cout, R, S, st, pad, act=act,
                       x2=_place(x2, x2l) if x2l else None, residual=_place(r, rl) if rl else None, out=out)
    assert y.shape == want.shape
    assert torch.equal(y.cpu().double(), want), f"{int((y.cpu().double() != want).sum())} of {want.numel()} outputs differ"
    assert _neighbours_untouched(big, Cout)


def test_conv2d_f32_unaligned_x2_equals_aligned_x2():
    """an in2 that is dense but 4 bytes off 16-byte alignment falls to the element loader and gives the vector path's answer"""
    from openess_amd import hip
    g = torch.Generator().manual_seed(41)
    x, x2 = _iv(g, (2, 32, 6, 9)), _iv(g, (2, 32, 6, 9))
    packed, b = hip.pack_conv_weight_f32(_iv(g, (33, 32, 3, 3), -1, 1).cuda()), _iv(g, (33,)).cuda()
    ya = hip.conv2d_f32(_cl(x), packed, b, 33, 3, 3, 1, 1, act='relu', x2=_cl(x2))
    yb = hip.conv2d_f32(_cl(x), packed, b, 33, 3, 3, 1, 1, act='relu', x2=_place(x2, 'off4'))
    assert torch.equal(ya, yb)


@pytest.mark.parametrize("B,Cin,H,W,Cout,xl", [(2, 16, 5, 7, 33, 'cl'), (1, 12, 1, 6, 3, 'cl'), (1, 16, 3, 1, 32, 'nchw')])
def test_upsample_conv_f32_odd_extents_exact(B, Cin, H, W, Cout, xl):
    from openess_amd import hip
    g = torch.Generator().manual_seed(B * 11 + Cin + H)
    x, skip = _iv(g, (B, Cin, H, W)), _iv(g, (B, Cin, H, W))
    w, b = _iv(g, (Cout, Cin, 3, 3), -1, 1), _iv(g, (Cout,))
    y = hip.conv2d_f32(_place(x, xl), hip.pack_conv_weight_f32(w.cuda()), b.cuda(), Cout, 3, 3, 1, 1, act='relu', x2=_place(skip, xl),
                       upsample2x=True)
    up = F.interpolate(x.double() + skip.double(), scale_factor=2, mode='bilinear', align_corners=False)
    pre = F.conv2d(up, w.double(), b.double(), 1, 1)
    want = torch.relu(pre)
    assert y.shape == want.shape == (B, Cout, 2 * H, 2 * W)
    _nonzero_floors(pre, want)
    assert torch.equal(y.cpu().double(), want), f"{int((y.cpu().double() != want).sum())} of {want.numel()} outputs differ"


@pytest.mark.parametrize("B,Cin,H,W,Cout,two", [(2, 8, 3, 5, 40, False), (1, 24, 1, 1, 1, False), (2, 24, 4, 3, 40, True),
                                                (1, 8, 1, 1, 1, True)])
def test_conv_transpose2d_f32_ragged_channels_exact(B, Cin, H, W, Cout, two):
    from openess_amd import hip
    g = torch.Generator().manual_seed(B * 100 + Cin + Cout)
    x = _iv(g, (B, Cin, H, W))
    skip = _iv(g, (B, Cin, H, W)) if two else None
    w, b = _iv(g, (Cin, Cout, 5, 5), -1, 1), _iv(g, (Cout,))
    out = torch.full((B, Cout, 2 * H, 2 * W), float("nan"), device="cuda")          # an NCHW output view
    y = hip.conv_transpose2d_f32(_cl(x), hip.pack_conv_transpose_weight_f32(w.cuda()), b.cuda(), Cout, act='relu',
                                 x2=_cl(skip) if two else None, out=out)
    pre = F.conv_transpose2d(x.double() + (skip.double() if two else 0), w.double(), b.double(), 2, 2, 1)
    want = torch.relu(pre)
    assert y.shape == want.shape == (B, Cout, 2 * H, 2 * W)
    _nonzero_floors(pre, want)
    assert torch.equal(y.cpu().double(), want), f"{int((y.cpu().double() != want).sum())} of {want.numel()} outputs differ"


def test_convlstm_step_f32_hidden_channel_slice_odd_extents():
    """B > 1, odd H and W, xh the whole cat(x, h) buffer and the hidden output a channel slice of a second one (neighbours
    asserted untouched), from a non-zero cell; sigmoid / tanh are not exact, so the existing 1e-5 bound applies."""
    from openess_amd import hip
    g = torch.Generator().manual_seed(19)
    B, H, W, Cx, C, k = 3, 7, 9, 16, 32, 3
    xh = torch.randn(B, Cx + C, H, W, generator=g)
    wt = torch.randn(4 * C, Cx + C, k, k, generator=g) / ((Cx + C) * k * k) ** 0.5
    b = torch.randn(4 * C, generator=g)
    c0 = torch.randn(B, H, W, C, generator=g)
    cell = c0.cuda().contiguous()
    nxt = torch.full((B, H, W, Cx + C), -7.0, device="cuda")
    h = hip.convlstm_step_f32(_cl(xh), hip.pack_conv_weight_f32(wt.cuda()), b.cuda(), C, k, 1, cell, nxt[..., Cx:].permute(0, 3, 1, 2))
    i_, f_, o_, g_ = F.conv2d(xh.double(), wt.double(), b.double(), padding=1).chunk(4, 1)
    c64 = torch.sigmoid(f_) * c0.double().permute(0, 3, 1, 2) + torch.sigmoid(i_) * torch.tanh(g_)
    h64 = torch.sigmoid(o_) * torch.tanh(c64)
    assert relerr(h.cpu().numpy(), h64.numpy()) <= 1e-5
    assert relerr(cell.permute(0, 3, 1, 2).cpu().numpy(), c64.numpy()) <= 1e-5
    assert bool((nxt[..., :Cx] == -7.0).all())
