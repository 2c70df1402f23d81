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
