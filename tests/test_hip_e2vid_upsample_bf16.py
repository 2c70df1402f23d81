"""GPU tests of upsample-conv E2VID models in bf16: the network against a torch fp32 restatement of the reference's
UNetRecurrent (unet.py:146-170), the transposed-decoder model's image bit for bit against the walk that calls its decoders as
before K30, the command line end to end against its own --precision fp32, and the online reconstruction source."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nets as on
from oracle.step import E2VID_LIGHTWEIGHT_CONFIG
from tests.synth import fill_by_name

pytestmark = pytest.mark.gpu
H, W = 32, 48


def _cfg(norm):
    return dict(E2VID_LIGHTWEIGHT_CONFIG, use_upsample_conv=True, norm=norm)


def _model(cfg, seed=11):
    from openess_amd.e2vid.model.model import E2VIDRecurrent
    m = E2VIDRecurrent(cfg).eval()
    fill_by_name(m, seed)
    return m


def _reconstructor(m, precision='bf16'):
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor
    return ImageReconstructor(m.cuda(), H, W, m.num_bins, torch.device("cuda"), SimpleNamespace(precision=precision))


def _events(seed, n=3, B=2):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, 5, H, W, generator=g) * (torch.rand(B, 5, H, W, generator=g) > 0.7) for _ in range(n)]


def cos(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


def _torch_unet_fp32(m, x, states):
    """UNetRecurrent (ConvLSTM, skip_sum, UpsampleConvLayer decoders, norm None or eval-mode BatchNorm) written out in torch
    fp32: unet.py:146-170 and submodules.py of the reference (_torch_unet_fp32 of tests/test_hip_e2vid_fp32.py plus the norms:
    ConvLayer conv -> BN -> act, ResidualBlock conv-bn-relu-conv-bn + x -> relu, the prediction layer conv -> BN, no act)."""
    u = m.unetrecurrent

    def conv(c, t):
        return F.conv2d(t, c.weight, c.bias, c.stride, c.padding)

    def bn(b, t):
        return F.batch_norm(t, b.running_mean, b.running_var, b.weight, b.bias, False, 0.0, b.eps)

    def layer(l, t, act=True):
        y = conv(l.conv2d, t)
        if l.norm == 'BN':
            y = bn(l.norm_layer, y)
        return torch.relu(y) if act else y
    head = layer(u.head, x)
    h, blocks, new = head, [], []
    for i, e in enumerate(u.encoders):
        y = layer(e.conv, h)
        hp, cp = states[i] if states is not None else (torch.zeros_like(y), torch.zeros_like(y))
        i_, f_, o_, g_ = conv(e.recurrent_block.Gates, torch.cat([y, hp], 1)).chunk(4, 1)
        c = torch.sigmoid(f_) * cp + torch.sigmoid(i_) * torch.tanh(g_)
        h = torch.sigmoid(o_) * torch.tanh(c)
        blocks.append(h)
        new.append((h, c))
    for rb in u.resblocks:
        y = conv(rb.conv1, h)
        y = torch.relu(bn(rb.bn1, y) if rb.norm == 'BN' else y)
        y = conv(rb.conv2, y)
        h = torch.relu((bn(rb.bn2, y) if rb.norm == 'BN' else y) + h)
    for i, d in enumerate(u.decoders):
        up = F.interpolate(h + blocks[u.num_encoders - i - 1], scale_factor=2, mode='bilinear', align_corners=False)
        h = layer(d, up)
    return torch.sigmoid(layer(u.pred, h + head, act=False)), new


@pytest.mark.parametrize("norm", ['BN', None])
def test_upsample_conv_model_bf16_matches_torch_fp32(norm):
    """Three recurrent steps through a bf16 ImageReconstructor.  Bounds: the project's own for the transposed sibling
    (test_e2vid_offline_reconstruction_image): max abs error < 2e-2 on the sigmoid image, cosine of the mean-removed images
    > 0.995.  The figures are printed before the assertion and recorded in DESIGN.md K30."""
    from openess_amd.e2vid.model.submodules import UpsampleConvLayer
    cfg = _cfg(norm)
    m = _model(cfg)
    ref = _model(cfg)
    assert all(isinstance(d, UpsampleConvLayer) for d in m.unetrecurrent.decoders)
    rec = _reconstructor(m)
    st = None
    for ev in _events(8):
        img, _, _ = rec.update_reconstruction(ev.cuda(), reconstruct=True)
        with torch.no_grad():
            want, st = _torch_unet_fp32(ref, on.event_preprocess(ev), st)
    assert img.shape == want.shape == (2, 1, H, W) and img.dtype == torch.float32
    got, want = img.cpu().numpy(), want.numpy()
    err, c = float(np.abs(got - want).max()), cos(got - got.mean(), want - want.mean())
    print(f"upsample-conv E2VID bf16, norm={norm}: max |img - torch fp32| = {err:.3e}, cosine = {c:.5f}, "
          f"image range [{want.min():.3f}, {want.max():.3f}]")
    assert want.max() - want.min() > 0.1                     # a real image, not a constant
    assert err < 2e-2
    assert c > 0.995


def _walk_as_before(m, x, states):
    """UNetRecurrent.forward(..., reconstruct=True) in the plain order from the model's own pieces, every decoder called the way
    the network called it before K30: decoder(x + skip)."""
    from openess_amd import engine
    u = m.unetrecurrent
    states = states if states is not None else [None] * u.num_encoders
    head = u.head(x)
    x, blocks, new = head, [], []
    for enc, st in zip(u.encoders, states):
        st = enc.run_conv(x, st)
        x = enc.recurrent_block.step(st)
        blocks.append(x)
        new.append(st)
    for rb in u.resblocks:
        x = rb(x)
    for i, dec in enumerate(u.decoders):
        x = dec(x + blocks[u.num_encoders - i - 1])
    logits = engine.conv2d_infer(x + head, u.pred._packed(x.shape[1]), 1, 1, 1, 0, 1, out_f32=True)
    return torch.sigmoid(logits.float()), new


def test_transposed_decoder_model_keeps_its_bits():
    from openess_amd.e2vid.model.submodules import TransposedConvLayer
    m, m2 = _model(E2VID_LIGHTWEIGHT_CONFIG), _model(E2VID_LIGHTWEIGHT_CONFIG)
    assert all(isinstance(d, TransposedConvLayer) for d in m.unetrecurrent.decoders)
    rec, rec2 = _reconstructor(m), _reconstructor(m2)
    st = None
    for ev in _events(21):
        img, _, _ = rec.update_reconstruction(ev.cuda(), reconstruct=True)
        with torch.no_grad():
            x = rec2.event_preprocessor.slice_to_nhwc8(ev.cuda().contiguous(), 0, 5)
            want, st = _walk_as_before(m2, x, st)
        assert torch.equal(img, want)
    assert float(img.max() - img.min()) > 0.1


def _events_file(tmp_path):
    rng = np.random.default_rng(5)
    Ws, Hs, n = 48, 32, 6000
    t = np.sort(rng.uniform(0.0, 0.2, n))
    ev = np.stack([t, rng.integers(0, Ws, n), rng.integers(0, Hs, n), rng.integers(0, 2, n)], 1)
    path = str(tmp_path / "events.txt")
    with open(path, "w") as f:
        f.write(f"{Ws} {Hs}\n")
        for r in ev:
            f.write("%.9f %d %d %d\n" % (r[0], r[1], r[2], r[3]))
    return path, Ws, Hs


def test_run_reconstruction_cli_default_precision_end_to_end(tmp_path):
    """A checkpoint in the reference's format with use_upsample_conv: True through the command line in the default precision
    (bf16): one PNG per window plus timestamps.txt, every frame within 6 grey levels of the --precision fp32 run on the same
    checkpoint (0.02 * 255 = 5.1 for the image bound above, plus one for the two roundings to uint8)."""
    from PIL import Image
    from openess_amd.e2vid import run_reconstruction as rr
    cfg = _cfg('BN')
    ckpt = str(tmp_path / "upsample_conv.pth.tar")
    torch.save({'arch': 'E2VIDRecurrent', 'model': cfg, 'state_dict': _model(cfg).state_dict()}, ckpt)
    path, Ws, Hs = _events_file(tmp_path)
    n_win = -(-6000 // int(Ws * Hs * 0.35))                   # the reference's default window: 0.35 events per pixel; the last is short
    runs = {}
    for name, extra in (("bf16", []), ("fp32", ["--precision", "fp32"])):
        out = str(tmp_path / name)
        frames = rr.main(["-c", ckpt, "-i", path, "-o", out] + extra)
        folder = os.path.join(out, "reconstruction")
        pngs = sorted(f for f in os.listdir(folder) if f.endswith(".png"))
        assert len(frames) == n_win and pngs == [f"frame_{k:010d}.png" for k in range(n_win)]
        assert len(np.loadtxt(os.path.join(folder, "timestamps.txt"))) == n_win
        for k in range(n_win):
            assert frames[k].shape == (Hs, Ws) and frames[k].dtype == np.uint8
            assert np.array_equal(np.asarray(Image.open(os.path.join(folder, pngs[k]))), frames[k])
        runs[name] = np.stack(frames).astype(np.int64)
    d = np.abs(runs["bf16"] - runs["fp32"])
    print(f"CLI bf16 against fp32: max grey-level difference {int(d.max())} over {n_win} frames, "
          f"fp32 levels span {int(runs['fp32'].min())} .. {int(runs['fp32'].max())}")
    assert runs["fp32"].max() - runs["fp32"].min() > 25
    assert d.max() <= 6


def test_online_recon_image_runs_the_upsample_conv_model_in_bf16():
    from openess_amd.e2vid.image_reconstructor import PostProcessor
    from openess_amd.training.base_trainer_ov import online_recon_image
    m = _model(_cfg('BN'))
    rec = _reconstructor(m)
    post = PostProcessor(torch.device("cuda"))
    vox = torch.cat(_events(33), 1).cuda().contiguous()      # [2, 3 * 5, 32, 48]
    aug = {'flip': [0, 1], 'brightness': [1.0, 1.1], 'contrast': [1.0, 0.9], 'noise_seed': [0, 0]}
    empty = {'grayscale': None}
    a = online_recon_image(rec, post, vox, 3, 5, aug)
    assert rec.last_states_for_each_channel == empty
    b = online_recon_image(rec, post, vox, 3, 5, aug)
    assert rec.last_states_for_each_channel == empty
    assert a.shape == (2, 3, H, W) and a.dtype == torch.float32 and a.is_cuda and bool(torch.isfinite(a).all())
    assert torch.equal(a, b)
    assert len(torch.unique(a)) > 16
