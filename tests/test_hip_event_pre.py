"""GPU tests of EventPreprocessor's hot-pixel removal and flip inside the event kernels.
Exact cases: inputs are multiples of 2^-8 with |v| <= 8 (tests/event_pre_cases.py), so every sum and sum of squares is exact in
double whatever the order, and every new entry point has to be BIT-EQUAL to the option-less entry point fed
torch.flip(zeroed copy, [2, 3]) -- the statistics doubles included.  General inputs: the flip only permutes, and the float64
restatement / the reference's own fixture are met within the bound of the existing EventPreprocessor golden test
(tests/test_hip_nets.py: rtol 2e-5, atol 2e-6 in fp32; 1e-2 for the bf16 NHWC8 form).  End to end: an ImageReconstructor with
the options on raw events == one without on the torch-preprocessed tensor, on every route; the trainers run with the options."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml

from tests import event_pre_cases as ec

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL, ATOL = 2e-5, 2e-6                     # tests/test_hip_nets.py::test_event_preprocessor_matches_reference_golden
COMBOS = ("hot", "flip", "both", "nonorm", "allhot")
# the issue's shapes (vector path 16 x 24, scalar path 13 x 19) and two that give the statistics / apply kernels a second
# workgroup per plane on each path (HW / 4 > 512 resp. HW > 512 pixel groups)
SHAPES = [(2, 16, 24, 5), (2, 13, 19, 5), (1, 16, 24, 10), (2, 48, 64, 5), (2, 45, 47, 0)]


def _case(combo, ev, c0, extra=()):
    """-> (mask uint8 [H, W] on the device | None, flip, normalize)."""
    H, W = ev.shape[2:]
    if combo == "allhot":                    # every non-zero pixel of the slice is hot: nnz == 0, the inactive branch
        return (ev[:, c0:c0 + 5] != 0).any(0).any(0).to(torch.uint8).contiguous(), True, True
    mask = ec.hot_mask(H, W, extra).to(ev.device) if combo != "flip" else None
    return mask, combo != "hot", combo != "nonorm"


# ------------------------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("B,H,W,c0", SHAPES)
@pytest.mark.parametrize("combo", COMBOS)
def test_stats_apply_and_nhwc8_equal_the_option_less_kernels_on_the_composed_tensor(B, H, W, c0, combo):
    from openess_amd import hip
    ev = ec.exact_events(100 * H + W + B, (B, 15, H, W), DEV)
    keep = ev.clone()
    mask, flip, normalize = _case(combo, ev, c0)
    pre = hip.EventPre(mask, flip)
    sl = ec.torch_pre(ev, mask, flip, c0, 5)                               # [B, 5, H, W]: zeroed copy, then torch.flip
    whole = ec.torch_pre(ev, mask, flip)
    # statistics: single slice and all slices in one launch; the doubles themselves
    got = hip.masked_stats_slice(ev, c0, 5, pre=pre)[:3]
    want = hip.masked_stats_slice(sl, 0, 5)[:3]
    assert torch.equal(got, want), (got, want)
    if combo == "allhot":
        assert float(got[2]) == 0.0
    else:
        assert float(got[2]) > 0
    got_all = hip.masked_stats_slices(ev, 5, pre=pre)[:, :3]
    assert torch.equal(got_all, hip.masked_stats_slices(whole, 5)[:, :3]) and torch.equal(got_all[c0 // 5], want)
    x64 = sl.double()
    assert float(want[0]) == float(x64.sum()) and float(want[1]) == float((x64 * x64).sum()) and float(want[2]) == float((sl != 0).sum())
    # fp32 NCHW apply: the slice and the whole tensor
    out = hip.masked_normalize_slice(ev, c0, 5, pre=pre, normalize=normalize)
    assert torch.equal(out, hip.masked_normalize_slice(sl, 0, 5) if normalize else sl)
    if combo == "allhot":
        assert float(out.abs().max()) == 0.0
    if normalize:
        assert torch.equal(hip.masked_normalize(ev, pre=pre), hip.masked_normalize(whole))
    # NHWC8 bf16 re-layout
    y = hip.event_slice_to_nhwc8(ev, c0, 5, normalize=normalize, pre=pre)
    assert torch.equal(y, hip.event_slice_to_nhwc8(sl, 0, 5, normalize=normalize))
    assert torch.equal(ev, keep)                                           # the caller's tensor is only read


def _head_weights(seed):
    """bf16-exact seeded weights of the head (5 of 8 input channels) and encoder 0."""
    from openess_amd import hip
    g = torch.Generator().manual_seed(seed)
    wh = torch.zeros(32, 8, 5, 5)
    wh[:, :5] = torch.randint(-8, 9, (32, 5, 5, 5), generator=g).float() / 64.0
    we = torch.randint(-8, 9, (64, 32, 5, 5), generator=g).float() / 128.0
    bh = torch.randint(-8, 9, (32,), generator=g).float() / 16.0
    be = torch.randint(-8, 9, (64,), generator=g).float() / 16.0
    return hip.pack_conv_weight(wh.to(DEV)), bh.to(DEV), hip.pack_conv_weight(we.to(DEV)), be.to(DEV)


@pytest.mark.parametrize("B,H,W,c0", [(2, 32, 48, 5), (2, 40, 56, 5), (1, 40, 56, 10)])
@pytest.mark.parametrize("combo", COMBOS)
def test_fused_head_enc0_equals_the_option_less_kernel_on_the_composed_tensor(B, H, W, c0, combo):
    """32 x 48: whole 8 x 16 output patches; 40 x 56 (20 x 28 outputs): ragged ones.  Hot pixels on the borders of the 16 x 32
    input patches, at the image corners, and (the mirrored border) where the flip puts a patch border."""
    from openess_amd import hip
    ev = ec.exact_events(7 * H + W + B, (B, 15, H, W), DEV)
    keep = ev.clone()
    borders = ((15, 31), (16, 32), (15, 32), (16, 31), (H - 16, W - 32), (H - 17, W - 33), (31, 5), (H - 1, 31), (16, 0))
    mask, flip, normalize = _case(combo, ev, c0, tuple((y, x) for y, x in borders if 0 <= y < H and 0 <= x < W))
    pre = hip.EventPre(mask, flip)
    ph, bh, pe, be = _head_weights(H)
    sl = ec.torch_pre(ev, mask, flip, c0, 5)
    want = hip.e2vid_events_head_enc0(sl, 0, 5, normalize, ph, bh, True, pe, be, True)
    got = hip.e2vid_events_head_enc0(ev, c0, 5, normalize, ph, bh, True, pe, be, True, pre=pre)
    assert got.shape == (B, H // 2, W // 2, 64) and torch.equal(got, want)
    if combo != "allhot":
        assert not torch.equal(got, hip.e2vid_events_head_enc0(ev, c0, 5, normalize, ph, bh, True, pe, be, True))
    # into a channel slice of a wider buffer, as the ConvLSTM's cat(x, h) buffer takes it
    buf = torch.full((B, H // 2, W // 2, 128), 3.0, device=DEV, dtype=torch.bfloat16)
    hip.e2vid_events_head_enc0(ev, c0, 5, normalize, ph, bh, True, pe, be, True, out=buf[..., :64], pre=pre)
    assert torch.equal(buf[..., :64], want) and float((buf[..., 64:] - 3).abs().max()) == 0
    assert torch.equal(ev, keep)


# ------------------------------------------------------------------------------------------------------------------ general inputs
@pytest.mark.parametrize("H,W", [(16, 24), (13, 19), (48, 64)])
def test_general_inputs_flip_only_permutes_and_float64_is_met(H, W):
    from openess_amd import hip
    ev = ec.general_events(H * W, (2, 15, H, W), DEV)
    mask = ec.hot_mask(H, W).to(DEV)
    rows = [(int(x), int(y)) for y, x in mask.nonzero().cpu().tolist()]
    for c0 in (0, 10):
        a = hip.masked_normalize_slice(ev, c0, 5, pre=hip.EventPre(mask, False))
        b = hip.masked_normalize_slice(ev, c0, 5, pre=hip.EventPre(mask, True))
        assert torch.equal(b, torch.flip(a, [2, 3]))
        want = ec.restate_f64(ev[:, c0:c0 + 5].cpu().numpy(), rows, True, False)
        np.testing.assert_allclose(b.cpu().numpy(), want, rtol=RTOL, atol=ATOL)
        ya = hip.event_slice_to_nhwc8(ev, c0, 5, pre=hip.EventPre(mask, False))
        yb = hip.event_slice_to_nhwc8(ev, c0, 5, pre=hip.EventPre(mask, True))
        assert torch.equal(yb, torch.flip(ya, [2, 3])) and float(yb[:, 5:].abs().max()) == 0
        np.testing.assert_allclose(yb[:, :5].float().cpu().numpy(), want, rtol=1e-2, atol=1e-2)
    wa = hip.masked_normalize(ev, pre=hip.EventPre(mask, False))
    wb = hip.masked_normalize(ev, pre=hip.EventPre(None, True))
    assert torch.equal(hip.masked_normalize(ev, pre=hip.EventPre(mask, True)), torch.flip(wa, [2, 3]))
    np.testing.assert_allclose(wb.cpu().numpy(), ec.restate_f64(ev.cpu().numpy(), None, True, False), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("size", ec.SIZES)
@pytest.mark.parametrize("combo", sorted(ec.COMBOS))
def test_event_preprocessor_matches_the_reference_fixture(size, combo, tmp_path):
    """EventPreprocessor(options) on the GPU against the output of the reference's own (tests/golden/gen_golden_e2vid_hotflip.py)."""
    from openess_amd.e2vid.utils.inference_utils import EventPreprocessor
    g = dict(np.load(ec.GOLDEN))
    hot, flip, nonorm = ec.COMBOS[combo]
    f = tmp_path / "hot.txt"
    np.savetxt(f, g[f"rows_{size}"], fmt="%d", delimiter=",")
    pre = EventPreprocessor(SimpleNamespace(hot_pixels_file=str(f) if hot else None, flip=flip, no_normalize=nonorm))
    x = torch.from_numpy(g[f"in_{size}"]).to(DEV)
    got = pre(x)
    np.testing.assert_allclose(got.cpu().numpy(), g[f"out_{size}_{combo}"], rtol=RTOL, atol=ATOL)
    assert np.array_equal(x.cpu().numpy(), g[f"in_{size}"])                # not mutated (the reference zeroes its argument)
    y = pre.slice_to_nhwc8(x.contiguous(), 0, 5).float().cpu().numpy()
    np.testing.assert_allclose(y[:, :5], g[f"out_{size}_{combo}"], rtol=1e-2, atol=1e-2)
    assert np.abs(y[:, 5:]).max() == 0


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def e2vid():
    from oracle.step import E2VID_LIGHTWEIGHT_CONFIG
    from openess_amd.e2vid.model.model import E2VIDRecurrent
    from tests.synth import fill_by_name
    m = E2VIDRecurrent(E2VID_LIGHTWEIGHT_CONFIG).eval()
    fill_by_name(m, 11)
    return m.to(DEV)


def _hot_file(tmp_path, mask):
    f = tmp_path / f"hot_{mask.shape[0]}x{mask.shape[1]}.txt"
    rows = [(x, y) for y, x in mask.nonzero().cpu().tolist()]
    np.savetxt(f, np.array(rows + rows[:1]), fmt="%d", delimiter=",")      # (a duplicate row)
    return str(f)


def _cells(states):
    return [s['cell' if 'cell' in s else 'cell_tiled'].clone() for s in states]


def _run(model, H, W, ev, route, opts):
    """Three sub-windows from empty states on `route` -> (latents of the last, cell states, image | None)."""
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor
    rec = ImageReconstructor(model, H, W, 5, torch.device(DEV), SimpleNamespace(precision='fp32' if route == 'fp32' else 'bf16', **opts))
    if route == 'plain':
        rec.skew = False
    for i in range(3):
        kw = {} if route in ('plain', 'fp32') else {'need_latents': i == 2}
        _, states, lat = rec.update_reconstruction(ev, channel_slice=(5 * i, 5), **kw)
    lat = {k: v.clone() for k, v in lat.items() if v is not None}
    cells = _cells(states)
    img, _, _ = rec.update_reconstruction(ev, channel_slice=(10, 5), reconstruct=True)
    return lat, cells, img.clone()


@pytest.mark.parametrize("route,H,W", [("fused", 32, 48), ("plain", 32, 48), ("fused", 44, 60), ("fp32", 32, 48), ("fp32", 44, 60)])
def test_reconstructor_with_options_equals_one_without_on_the_preprocessed_tensor(route, H, W, e2vid, tmp_path):
    """fused: sub-windows 0, 1 drop their latents (fused head + encoder-0 kernel on the skewed schedule at 32 x 48; 44 x 60 is
    padded by reflection after the preprocessing, so it takes the NHWC8 kernel); plain: every call keeps its latents, skew off
    (the NHWC8 kernel); fp32: the fp32 NCHW apply.  Latents, cell states and the reconstructed image are bit-equal."""
    ev = ec.exact_events(H + W, (2, 15, H, W), DEV)
    keep = ev.clone()
    mask = ec.hot_mask(H, W, ((15, 31), (16, 32), (7, 9))).to(DEV)
    opts = {'hot_pixels_file': _hot_file(tmp_path, mask), 'flip': True}
    composed = ec.torch_pre(ev, mask, True)
    want = _run(e2vid, H, W, composed, route, {})
    got = _run(e2vid, H, W, ev, route, opts)
    assert set(got[0]) == set(want[0]) and len(got[1]) == len(want[1]) == 3
    for k in want[0]:
        assert torch.equal(got[0][k], want[0][k]), k
    for a, b in zip(got[1], want[1]):
        assert torch.equal(a, b)
    assert got[2].shape[-2:] == want[2].shape[-2:] and torch.equal(got[2], want[2]) and bool(torch.isfinite(got[2]).all())
    assert torch.equal(ev, keep)
    plain = _run(e2vid, H, W, ev, route, {})
    assert not torch.equal(plain[2], got[2])                               # the options do something
    # repeated, and on a side stream
    again = _run(e2vid, H, W, ev, route, opts)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _run(e2vid, H, W, ev, route, opts)
    torch.cuda.current_stream().wait_stream(side)
    for r in (again, other):
        assert all(torch.equal(r[0][k], want[0][k]) for k in want[0]) and torch.equal(r[2], want[2])
        assert all(torch.equal(a, b) for a, b in zip(r[1], want[1]))


def test_reference_contract_call_and_hot_only_and_flip_only(e2vid, tmp_path):
    """update_reconstruction(tensor of one sub-window) without channel_slice, with each option alone."""
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor
    H, W = 32, 48
    ev = ec.exact_events(5, (2, 5, H, W), DEV)
    mask = ec.hot_mask(H, W).to(DEV)
    for opts, m, flip in (({'hot_pixels_file': _hot_file(tmp_path, mask)}, mask, False), ({'flip': True}, None, True)):
        for precision in ('bf16', 'fp32'):
            a = ImageReconstructor(e2vid, H, W, 5, torch.device(DEV), SimpleNamespace(precision=precision, **opts))
            b = ImageReconstructor(e2vid, H, W, 5, torch.device(DEV), SimpleNamespace(precision=precision))
            ia, _, la = a.update_reconstruction(ev, reconstruct=True)
            ib, _, lb = b.update_reconstruction(ec.torch_pre(ev, m, flip), reconstruct=True)
            assert torch.equal(ia, ib) and torch.equal(la[8], lb[8])


# ------------------------------------------------------------------------------------------------------------------ trainers
CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")
BLOCK = [(x, y) for y in range(10, 14) for x in range(20, 41)]           # 84 hot pixels in one block: some carry events for sure


def _block_file(tmp_path):
    f = tmp_path / "hot_block.txt"
    np.savetxt(f, np.array(BLOCK), fmt="%d", delimiter=",")
    return str(f)


def _zeroed(vox):
    z = vox.clone()
    for x, y in BLOCK:
        z[:, :, y, x] = 0
    return z


def test_finetune_trainer_runs_with_a_hot_pixel_file_and_its_latents_are_the_hand_composed_ones(tmp_path):
    import train
    from openess_amd.config.settings import Settings
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor
    train.seed_everything()
    s = Settings(os.path.join(CFG, "finetune_dsec_synthetic.yaml"), generate_log=False)
    s.ckpt_dir = str(tmp_path)
    s.config_option = 'frame2voxel'
    s.if_finetuning, s.if_linear_probing, s.if_supervised_only = True, False, False
    s.e2vid_config.hot_pixels_file = _block_file(tmp_path)
    tr, _ = train.build_trainer(s)
    assert len(tr.reconstructor.event_preprocessor.hot_pixel_locations) == len(BLOCK)
    K, nwin, (H, W) = s.semseg_num_classes, s.nr_events_data_b, s.img_size_b
    torch.manual_seed(4)
    ev = ec.exact_events(9, (2, nwin * 5, H, W), DEV)
    gt = torch.randint(0, K, (2, H // 4, W // 4)).repeat_interleave(4, 1).repeat_interleave(4, 2).to(DEV)
    losses, _, total = tr.train_step((ev, gt, torch.rand(2, 3, H, W, device=DEV), gt, gt, None))
    assert np.isfinite(float(total))
    got = {k: v.clone() for k, v in tr._latents(ev).items()}
    plain = ImageReconstructor(tr.front_end_sensor_b, tr.input_height, tr.input_width, s.nr_temporal_bins_b, tr.device)

    def latents(x):
        plain.last_states_for_each_channel = {'grayscale': None}
        for i in range(nwin):
            _, _, lat = plain.update_reconstruction(x, channel_slice=(i * 5, 5), need_latents=(i == nwin - 1))
        return {k: v.clone() for k, v in lat.items()}
    want, without = latents(_zeroed(ev)), latents(ev)
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
        # the difference from the option-less run sits exactly where the hand-composed run puts it
        assert torch.equal(got[k] != without[k], want[k] != without[k])
    assert not torch.equal(got[1], without[1])


def test_online_recon_batch_runs_with_a_hot_pixel_file_and_slot_2_is_the_hand_composed_one(tmp_path, monkeypatch):
    import openess_amd.e2vid.run_reconstruction as mod
    import train
    from openess_amd.config.settings import Settings
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor, PostProcessor
    from openess_amd.training.base_trainer_ov import online_recon_image
    from tests import online_recon_cases as oc
    from tests.synth import fill_by_name
    from tests.test_hip_online_recon import PRETRAIN, _host_batch, _voxels
    orig = mod.load_model
    monkeypatch.setattr(mod, 'load_model', lambda path: fill_by_name(orig(path), oc.FILL_SEED))
    hw = (64, 96)
    cfg = yaml.load(open(os.path.join(oc.CFG, PRETRAIN)), yaml.Loader)
    cfg['dataset']['DSEC_events']['shape'] = list(hw)
    cfg['model']['data_augmentation_train'] = False
    path = tmp_path / "settings.yaml"
    path.write_text(yaml.dump(cfg))
    train.seed_everything()
    s = Settings(str(path), generate_log=False)
    s.ckpt_dir = str(tmp_path)
    s.e2vid_config.hot_pixels_file = _block_file(tmp_path)
    tr, _ = train.build_trainer(s)
    host = _host_batch(tr)
    got = tr.prepare_batch(host, 'train')[2]
    assert got.shape == (oc.B, 3) + hw and bool(torch.isfinite(got).all())
    vox = _voxels(tr, host[2])
    rec = ImageReconstructor(tr.recon_model, hw[0], hw[1], oc.BINS, tr.device, SimpleNamespace(precision='bf16'))
    post = PostProcessor(tr.device)
    want = online_recon_image(rec, post, _zeroed(vox), oc.NWIN, oc.BINS, host[2]['aug'])
    without = online_recon_image(rec, post, vox, oc.NWIN, oc.BINS, host[2]['aug'])
    assert torch.equal(got, want)
    assert torch.equal(got != without, want != without) and not torch.equal(got, without)
