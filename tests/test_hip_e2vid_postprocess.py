"""E2VID post-processing on the MI355X: oess_e2vid_postprocess_* against the reference's PostProcessor run on the
CPU (tests/golden/e2vid_post.npz), against the same arithmetic as torch ops on the same GPU, through the crop view of
reconstruct(), run to run, without host synchronisation, and end to end through reconstruct() / the CLI.

Byte tolerance: within 1 everywhere and equal on >= 99.9 % of the pixels.  The blur is the only place where the order of the
arithmetic is not pinned (the library convolution's summation order is unknown); without it the bytes are compared exactly."""
import os
from collections import deque
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from openess_amd import hip
from openess_amd.e2vid.image_reconstructor import PostProcessor
from openess_amd.e2vid.utils.inference_utils import gkern

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "e2vid_post.npz")))


def _opts(a=0.3, s=1.0, imin=0.0, imax=1.0, auto=False, fsize=10):
    return SimpleNamespace(unsharp_mask_amount=a, unsharp_mask_sigma=s, Imin=imin, Imax=imax, auto_hdr=bool(auto),
                           auto_hdr_median_filter_size=int(fsize))


def _close_bytes(got, want, what):
    got, want = np.asarray(got).astype(np.int32), np.asarray(want).astype(np.int32)
    assert got.shape == want.shape, what
    d = np.abs(got - want)
    assert d.max() <= 1, (what, int(d.max()))
    assert (d == 0).mean() >= 0.999, (what, float((d == 0).mean()))


class TorchPost:
    """The reference's UnsharpMaskFilter + IntensityRescaler (e2vid/utils/inference_utils.py:90-129, 234-252) restated as the same
    torch ops, run on the GPU (the reference's default use_gpu=True)."""

    def __init__(self, o):
        self.o = o
        self.kernel = gkern(5, o.unsharp_mask_sigma).unsqueeze(0).unsqueeze(0).cuda()
        self.bounds = deque()
        self.Imin, self.Imax = o.Imin, o.Imax

    def __call__(self, img):
        a = self.o.unsharp_mask_amount
        if a > 0:
            blurred = F.conv2d(img, self.kernel, padding=2)
            img = (1 + a) * img - a * blurred
        if self.o.auto_hdr:
            Imin = np.clip(torch.min(img).item(), 0.0, 0.45)
            Imax = np.clip(torch.max(img).item(), 0.55, 1.0)
            if len(self.bounds) > self.o.auto_hdr_median_filter_size:
                self.bounds.popleft()
            self.bounds.append((Imin, Imax))
            self.Imin = np.median([lo for lo, hi in self.bounds])
            self.Imax = np.median([hi for lo, hi in self.bounds])
        img = 255.0 * (img - self.Imin) / (self.Imax - self.Imin)
        img.clamp_(0.0, 255.0)
        b = img.byte()
        return b[:, 0], b.float().div(255)


def test_postprocess_matches_reference_fixture(golden):
    for name in golden["cases"]:
        a, s, imin, imax, auto, fsize = golden[f"case_{name}_opts"]
        post = PostProcessor(torch.device("cuda"), _opts(a, s, imin, imax, auto, fsize))
        x, want, wb = golden[f"case_{name}_in"], golden[f"case_{name}_u8"], golden[f"case_{name}_bounds"]
        got = []
        for t in range(x.shape[0]):
            got.append(post.process_u8(torch.from_numpy(x[t]).cuda()).cpu().numpy())
            if auto:
                lo, hi = post.current_bounds()
                assert abs(lo - wb[t, 0]) <= 1e-6 and abs(hi - wb[t, 1]) <= 1e-6, (name, t, lo, hi, wb[t])
        _close_bytes(np.stack(got), want, name)


@pytest.mark.parametrize("auto,fsize", [(False, 10), (True, 10), (True, 3), (True, 0)])
@pytest.mark.parametrize("a,s", [(0.3, 1.0), (1.0, 2.5)])
def test_postprocess_matches_torch_ops_on_device(auto, fsize, a, s):
    g = torch.Generator().manual_seed(31 + fsize)
    o = _opts(a, s, 0.0, 1.0, auto, fsize)
    post, ref = PostProcessor(torch.device("cuda"), o), TorchPost(o)
    for t in range(12 if auto else 2):
        N, H, W = (1, 440, 640) if t % 3 else (2, 121, 203)
        lo, hi = 0.05 + 0.35 * torch.rand(1, generator=g).item(), 0.6 + 0.3 * torch.rand(1, generator=g).item()
        x = (lo + (hi - lo) * torch.rand(N, 1, H, W, generator=g)).cuda()
        if not auto:
            x = x * 1.4 - 0.2                                  # exercise the clamp
        u8, f32 = hip.e2vid_postprocess(x, post.gaussian_kernel, a, **({"hdr_state": post.hdr_state} if auto else {"bounds": (0.0, 1.0)}),
                                        want_f32=True)
        ru8, _ = ref(x)
        _close_bytes(u8.cpu().numpy(), ru8.cpu().numpy(), (auto, fsize, a, t))
        # the float output is torch's byte.float().div(255) on the device, bit for bit
        assert torch.equal(f32, u8[:, None].float().div(255)), t
        if auto:
            lo_b, hi_b = post.current_bounds()
            assert abs(lo_b - ref.Imin) <= 1e-6 and abs(hi_b - ref.Imax) <= 1e-6, (t, lo_b, hi_b, ref.Imin, ref.Imax)


@pytest.mark.parametrize("auto", [False, True])
def test_postprocess_without_unsharp_mask_is_exact(auto):
    """amount = 0 skips the blur: nothing is left whose order is unpinned, so the bytes equal the torch ops exactly (this pins the
    reciprocal multiply of torch's division by a host scalar, and the float64 medians)."""
    g = torch.Generator().manual_seed(5)
    o = _opts(0.0, 1.0, 0.1, 0.85, auto, 3)
    post, ref = PostProcessor(torch.device("cuda"), o), TorchPost(o)
    for t in range(6):
        x = (0.1 + 0.3 * t / 6 + 0.6 * torch.rand(2, 1, 240, 320, generator=g)).cuda()
        u8 = post.process_u8(x)
        ru8, _ = ref(x)
        assert torch.equal(u8, ru8), t
        if auto:
            assert post.current_bounds() == (float(ref.Imin), float(ref.Imax)), t


@pytest.mark.parametrize("auto", [False, True])
def test_postprocess_crop_view_equals_contiguous_copy(auto):
    g = torch.Generator().manual_seed(7)
    full = torch.rand(1, 1, 448, 640, generator=g).cuda()
    views = [full[:, :, 4:444, 0:640], full[:, :, 3:440, 5:634]]
    big = torch.rand(3, 1, 64, 96, generator=g).cuda()
    views.append(big[:, :, 2:61, 3:90])                          # N > 1: image stride of the padded map
    posts = [PostProcessor(torch.device("cuda"), _opts(auto=auto, fsize=3)) for _ in range(2)]
    for v in views * 2:
        assert v.stride(3) == 1
        a, fa = hip.e2vid_postprocess(v, posts[0].gaussian_kernel, 0.3,
                                      **({"hdr_state": posts[0].hdr_state} if auto else {"bounds": (0.0, 1.0)}), want_f32=True)
        b, fb = hip.e2vid_postprocess(v.contiguous(), posts[1].gaussian_kernel, 0.3,
                                      **({"hdr_state": posts[1].hdr_state} if auto else {"bounds": (0.0, 1.0)}), want_f32=True)
        assert torch.equal(a, b) and torch.equal(fa, fb)
        assert posts[0].current_bounds() == posts[1].current_bounds()


def test_postprocess_is_repeatable():
    g = torch.Generator().manual_seed(11)
    xs = [(0.1 + 0.2 * torch.rand(1).item() + 0.7 * torch.rand(8, 1, 480, 640, generator=g)).cuda() for _ in range(5)]
    runs = []
    for _ in range(2):
        post = PostProcessor(torch.device("cuda"), _opts(auto=True, fsize=3))
        runs.append([(post.process_u8(x).clone(), post.current_bounds()) for x in xs])
    for (a, ba), (b, bb) in zip(*runs):
        assert torch.equal(a, b) and ba == bb


def test_auto_hdr_makes_no_host_synchronisation():
    post = PostProcessor(torch.device("cuda"), _opts(auto=True, fsize=10))
    xs = [torch.rand(1, 1, 440, 640, device="cuda") for _ in range(4)]
    outs = [torch.empty(1, 440, 640, dtype=torch.uint8, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        with pytest.raises(RuntimeError):                        # the mode is live on this build: a .item() is caught
            xs[0].sum().item()
        for x, o in zip(xs, outs):
            hip.e2vid_postprocess(x, post.gaussian_kernel, 0.3, hdr_state=post.hdr_state, out_u8=o)
            post.process_u8(x)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()


def _events_file(tmp_path, W, H, n, seed=5):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0.0, 0.2, n))
    ev = np.stack([t, rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n)], 1)
    path = str(tmp_path / "events.txt")
    with open(path, "w") as f:
        f.write(f"{W} {H}\n")
        for r in ev:
            f.write("%.9f %d %d %d\n" % (r[0], r[1], r[2], r[3]))
    return path


def _raw_cropped_frames(path, model, n_per):
    """The reconstructor's fp32 frames, cropped as reconstruct() crops them (same kernels -> the same bits)."""
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor
    from openess_amd.e2vid.utils.event_readers import FixedSizeEventReader
    from openess_amd.e2vid.utils.inference_utils import events_to_voxel_grid_pytorch
    with open(path) as f:
        W, H = (int(v) for v in f.readline().split())
    dev = torch.device("cuda")
    model = model.to(dev).eval()
    rec = ImageReconstructor(model, H, W, model.num_bins, dev)
    out, start = [], 0
    for win in FixedSizeEventReader(path, num_events=n_per, start_index=0):
        grid = events_to_voxel_grid_pytorch(win, num_bins=model.num_bins, width=W, height=H, device=dev)
        img, _, _ = rec.update_reconstruction(grid.unsqueeze(0), start + win.shape[0], win[-1, 0], reconstruct=True)
        if rec.crop.needs_pad:
            img = img[:, :, rec.crop.iy0:rec.crop.iy1, rec.crop.ix0:rec.crop.ix1]
        out.append(img.clone())
        start += win.shape[0]
    return out


def _pngs(folder):
    from PIL import Image
    names = sorted(n for n in os.listdir(folder) if n.endswith(".png"))
    return [np.array(Image.open(os.path.join(folder, n))) for n in names]


def test_reconstruct_with_postprocessor_end_to_end(tmp_path):
    from openess_amd.e2vid import run_reconstruction as rr
    W, H = 44, 30                                                # padded to 48 x 32: the frames reach the kernel as crop views
    path = _events_file(tmp_path, W, H, 8000)
    raw = _raw_cropped_frames(path, rr.load_model('random'), 2000)
    assert len(raw) == 4 and raw[0].shape == (1, 1, H, W)
    for o in (_opts(), _opts(a=1.0, s=2.5, auto=True, fsize=2)):
        frames = rr.reconstruct(path, rr.load_model('random'), str(tmp_path / "pp"), window_size=2000,
                                postprocessor=PostProcessor(torch.device("cuda"), o))
        ref = TorchPost(o)
        want = [ref(r)[0][0].cpu().numpy() for r in raw]
        _close_bytes(np.stack(frames), np.stack(want), "reconstruct")
        _close_bytes(np.stack(_pngs(str(tmp_path / "pp"))), np.stack(want), "png")
    # the CLI: --postprocess --auto_hdr with the reference defaults
    out = tmp_path / "cli"
    rr.main(["-c", "random", "-i", path, "-o", str(out), "-N", "2000", "--postprocess", "--auto_hdr"])
    folder = str(out / "reconstruction")
    assert sorted(os.listdir(folder)) == [f"frame_{k:010d}.png" for k in range(4)] + ["timestamps.txt"]
    ref = TorchPost(_opts(auto=True, fsize=10))
    _close_bytes(np.stack(_pngs(folder)), np.stack([ref(r)[0][0].cpu().numpy() for r in raw]), "cli")
    # without --postprocess the CLI writes what reconstruct() writes without a post-processor
    plain = tmp_path / "plain"
    rr.main(["-c", "random", "-i", path, "-o", str(plain), "-N", "2000"])
    want = rr.reconstruct(path, rr.load_model('random'), None, window_size=2000)
    got = _pngs(str(plain / "reconstruction"))
    assert len(got) == len(want) == 4 and all(np.array_equal(a, b) for a, b in zip(got, want))
