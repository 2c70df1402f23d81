"""GPU tests of the fp32 SemSegE2VID evaluation path (K15, openess_amd/csrc/semseg_f32.hip + the K14 convolutions): the
InstanceNorm and upsample + concat kernels against float64 torch on the CPU (relerr <= 1e-5, gathers exact), the decoder
against the reference's own goldens and the float64 oracle (relerr <= 1e-4: the bounds tests/test_hip_e2vid_fp32.py holds the
fp32 kernels to; the bf16 decoder misses them by two orders of magnitude), the trainers' fp32 validation, repeatability,
the absence of host synchronisation, and tools/eval_precision.py."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import losses as ol
from oracle import nets as on
from oracle.step import E2VID_LIGHTWEIGHT_CONFIG, OracleSupervisedStep
from tests.synth import compact, damp_residual, fill_by_name

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
CFG = os.path.join(HERE, "configs")


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _report(name, value, bound):
    print(f"[semseg_fp32] {name}: {value:.3e} (bound {bound:.0e})", flush=True)
    return value


# ------------------------------------------------------------------------------------------------------------ InstanceNorm
# (B, C, H, W, relu, residual, layout)
NORM_CASES = {
    "plain_b2_odd": (2, 64, 33, 47, False, False, 'cl'),
    "relu_b2_odd": (2, 64, 33, 47, True, False, 'cl'),
    "residual_b2_odd": (2, 64, 33, 47, False, True, 'cl'),
    "decoder_256_4x6": (1, 256, 4, 6, False, True, 'cl'),
    "decoder_256_60x80": (1, 256, 60, 80, True, False, 'cl'),
    "decoder_32_480x640": (1, 32, 480, 640, True, False, 'cl'),
    "one_pixel_row": (2, 128, 1, 5, True, False, 'cl'),
    "nchw_c11": (2, 11, 9, 13, False, True, 'nchw'),
    "nchw_c70_relu": (1, 70, 17, 5, True, False, 'nchw'),
}


def _norm64(x, relu, res):
    y = F.instance_norm(x.double(), eps=1e-5)
    if res is not None:
        y = y + res.double()
    return torch.relu(y) if relu else y


@pytest.mark.parametrize("case", sorted(NORM_CASES))
def test_instance_norm_f32_matches_float64(case):
    from openess_amd import hip
    B, C, H, W, relu, res, layout = NORM_CASES[case]
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    x = torch.randn(B, C, H, W, generator=g) * (0.5 + torch.rand(1, C, 1, 1, generator=g)) + torch.randn(1, C, 1, 1, generator=g)
    r = torch.randn(B, C, H, W, generator=g) if res else None
    dev = (lambda t: t.cuda().contiguous()) if layout == 'nchw' else _cl
    y = hip.instance_norm_f32(dev(x), relu=relu, residual=None if r is None else dev(r))
    want = _norm64(x, relu, r)
    assert y.shape == want.shape and y.dtype == torch.float32
    assert _report(case, relerr(y.cpu().numpy(), want.numpy()), 1e-5) <= 1e-5


def test_instance_norm_f32_large_mean_is_stable():
    """Per-channel mean ~ 10, std ~ 1: E[x^2] - E[x]^2 in fp32 loses about four digits of the variance here; the shifted
    per-thread sums merged with Chan's update do not.  torch's own fp32 CPU instance_norm is at 2e-7 from float64 on such
    an input, so the ordinary 1e-5 bound holds."""
    from openess_amd import hip
    g = torch.Generator().manual_seed(77)
    for B, C, H, W in ((2, 64, 60, 80), (1, 32, 240, 320), (2, 12, 31, 29)):
        x = torch.randn(B, C, H, W, generator=g) + 10.0 * torch.where(torch.rand(1, C, 1, 1, generator=g) > 0.5, 1.0, -1.0)
        x = x + torch.randn(1, C, 1, 1, generator=g)
        want = _norm64(x, False, None)
        y = hip.instance_norm_f32(_cl(x))
        assert _report(f"offset {B}x{C}x{H}x{W}", relerr(y.cpu().numpy(), want.numpy()), 1e-5) <= 1e-5


@pytest.mark.parametrize("relu,res", [(True, False), (False, True)])
def test_instance_norm_f32_channel_slice_views(relu, res):
    """Input and output are channel slices of wider NHWC buffers; the neighbouring channels stay as they were; in place too."""
    from openess_amd import hip
    g = torch.Generator().manual_seed(5 + relu)
    B, C, H, W = 2, 32, 13, 9
    x = torch.randn(B, C, H, W, generator=g) * 2 + 1
    r = torch.randn(B, C, H, W, generator=g) if res else None
    big_in = torch.full((B, H, W, C + 8), 9.0, device="cuda")
    big_in[..., 4:4 + C] = x.permute(0, 2, 3, 1).cuda()
    big_out = torch.full((B, H, W, C + 16), -7.0, device="cuda")
    xin, out = big_in[..., 4:4 + C].permute(0, 3, 1, 2), big_out[..., 8:8 + C].permute(0, 3, 1, 2)
    y = hip.instance_norm_f32(xin, relu=relu, residual=None if r is None else _cl(r), out=out)
    want = _norm64(x, relu, r)
    assert y.data_ptr() == out.data_ptr()
    assert relerr(y.cpu().numpy(), want.numpy()) <= 1e-5
    assert bool((big_out[..., :8] == -7.0).all()) and bool((big_out[..., 8 + C:] == -7.0).all())
    assert bool((big_in[..., :4] == 9.0).all()) and bool((big_in[..., 4 + C:] == 9.0).all())
    assert torch.equal(big_in[..., 4:4 + C].permute(0, 3, 1, 2).cpu(), x)
    # in place on the slice: same bits as out of place, neighbours untouched
    hip.instance_norm_f32(xin, relu=relu, residual=None if r is None else _cl(r), out=xin)
    assert torch.equal(xin, y)
    assert bool((big_in[..., :4] == 9.0).all()) and bool((big_in[..., 4 + C:] == 9.0).all())


# ------------------------------------------------------------------------------------------------------ upsample + concat
def _iv(g, shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


@pytest.mark.parametrize("B,C,H,W,Cs,layout", [(2, 16, 5, 7, 8, 'cl'), (1, 16, 4, 6, 0, 'cl'), (2, 6, 3, 5, 5, 'nchw'), (1, 8, 1, 1, 4, 'cl'),
                                               (1, 128, 30, 40, 128, 'cl')])
def test_upsample_concat_f32_gather_is_exact(B, C, H, W, Cs, layout):
    """Nearest gathering and concatenation move values: the buffer equals torch's, and so does a 1 x 1 identity convolution
    of it on the MFMA kernel (small integers: every product and sum exact)."""
    from openess_amd import hip
    g = torch.Generator().manual_seed(B * 31 + C + Cs)
    x = _iv(g, (B, C, H, W))
    skip = _iv(g, (B, Cs, 2 * H, 2 * W)) if Cs else None
    dev = (lambda t: t.cuda().contiguous()) if layout == 'nchw' else _cl
    want = F.interpolate(x, scale_factor=2, mode='nearest')
    want = torch.cat([want, skip], 1) if Cs else want
    if layout == 'cl' and Cs:            # the skip is a channel slice of a wider buffer, like an E2VID latent (h half of cat(x, h))
        wide = torch.full((B, 2 * H, 2 * W, 2 * Cs), 5.0, device="cuda")
        wide[..., Cs:] = skip.permute(0, 2, 3, 1).cuda()
        sk = wide[..., Cs:].permute(0, 3, 1, 2)
    else:
        sk = None if skip is None else dev(skip)
    y = hip.upsample2x_concat_f32(dev(x), sk)
    assert y.shape == want.shape and torch.equal(y.cpu(), want)
    Ct = C + Cs
    eye = torch.eye(Ct)[:, :, None, None]
    z = hip.conv2d_f32(y, hip.pack_conv_weight_f32(eye.cuda()), None, Ct, 1, 1)
    assert torch.equal(z.cpu(), want)
    assert float((want != 0).float().mean()) > 0.5


@pytest.mark.parametrize("B,C,H,W,Cs,Cout", [(2, 32, 6, 10, 32, 64), (1, 64, 5, 7, 0, 32), (1, 16, 3, 5, 16, 33), (2, 128, 4, 6, 128, 128)])
def test_upsample_concat_conv3x3_f32_matches_float64(B, C, H, W, Cs, Cout):
    from openess_amd import hip
    g = torch.Generator().manual_seed(B * 13 + C + Cs + Cout)
    x = torch.randn(B, C, H, W, generator=g)
    skip = torch.randn(B, Cs, 2 * H, 2 * W, generator=g) if Cs else None
    w = torch.randn(Cout, C + Cs, 3, 3, generator=g) / ((C + Cs) * 9) ** 0.5
    b = torch.randn(Cout, generator=g)
    cat = hip.upsample2x_concat_f32(_cl(x), None if skip is None else _cl(skip))
    y = hip.conv2d_f32(cat, hip.pack_conv_weight_f32(w.cuda()), b.cuda(), Cout, 3, 3, 1, 1)
    up = F.interpolate(x.double(), scale_factor=2, mode='nearest')
    up = torch.cat([up, skip.double()], 1) if Cs else up
    want = F.conv2d(up, w.double(), b.double(), 1, 1)
    assert y.shape == want.shape == (B, Cout, 2 * H, 2 * W)
    assert relerr(y.cpu().numpy(), want.numpy()) <= 1e-5


# ------------------------------------------------------------------------------------------------------------ the decoder
@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLDEN, "nets.npz")))


@pytest.fixture(scope="module")
def keys():
    return json.load(open(os.path.join(GOLDEN, "nets_keys.json")))


def _decoder(keys, seed=12, **kw):
    from openess_amd.models.style_networks import SemSegE2VID
    net = SemSegE2VID(256, 11, skip_connect=True, skip_type='concat', text_embeddings_path=None, **kw)
    # the linear probe is not among the golden keys: with it, every key is filled (indices differ from the golden's, values repeat)
    fill_by_name(net, seed, None if kw.get('if_linear_probing') else keys["semseg"])
    return net.cuda().eval()


def _check_compact(g, key, arr):
    assert tuple(g[key + "__shape"]) == arr.shape, (key, arr.shape)
    sub, s, a = compact(arr)
    assert _report(key + " sample", relerr(sub, g[key + "__sub"]), 1e-4) <= 1e-4
    scale = float(g[key + "__abs"])
    assert abs(float(s) - float(g[key + "__sum"])) <= 1e-4 * scale and abs(float(a) - scale) <= 1e-4 * scale


def test_decoder_fp32_matches_reference_golden(g, keys):
    net = _decoder(keys)
    assert sorted(net.state_dict().keys()) == keys["semseg"]
    lat = {k: _cl(torch.from_numpy(g[f"semseg_lat{k}"])) for k in (1, 2, 4, 8)}
    out, x256 = net.forward_fp32(lat)
    assert set(out) == {1, 2, 4, 8} and out[8] is lat[8]
    assert out[1].dtype == out[4].dtype == x256.dtype == torch.float32
    assert _report("out4", relerr(out[4].cpu().numpy(), g["semseg_out4"]), 1e-4) <= 1e-4
    _check_compact(g, "semseg_logits", out[1].cpu().numpy())
    _check_compact(g, "semseg_x256", x256.cpu().numpy())
    assert out[2].shape == (2, 64, 16, 24)
    # materialize_ch256=False: same logits, no 256-channel map
    net2 = _decoder(keys, materialize_ch256=False)
    out2, none = net2.forward_fp32(lat)
    assert none is None and torch.equal(out2[1], out[1])
    with pytest.raises(NotImplementedError, match="pooled"):
        _decoder(keys, materialize_ch256='pooled').forward_fp32(lat)
    with pytest.raises(ValueError, match="fp32 latents"):
        net.forward_fp32({k: v.bfloat16() for k, v in lat.items()})


def test_decoder_fp32_linear_probe_matches_float64_oracle(g, keys):
    net = _decoder(keys, seed=21, if_linear_probing=True)
    fill_by_name(net, 21)
    ref = OracleSupervisedStep("frame2voxel", 11, 3, 5, True).net
    fill_by_name(ref, 21, sorted(net.state_dict().keys()))
    ref.double().eval()
    lat = {k: torch.from_numpy(g[f"semseg_lat{k}"]) for k in (1, 2, 4, 8)}
    with torch.no_grad():
        want = ref.linear_probe(ref({k: v.double() for k, v in lat.items()})[0][1])
    out, _ = net.forward_fp32({k: _cl(v) for k, v in lat.items()})
    assert out[1].shape == want.shape
    assert _report("linear probe logits", relerr(out[1].cpu().numpy(), want.numpy()), 1e-4) <= 1e-4


def _models(seed_front, seed_back, linear_probing=False):
    """(E2VID, decoder) on the device and their float64 oracle twins on the CPU, from identical weights."""
    from openess_amd.e2vid.model.model import E2VIDRecurrent
    from openess_amd.models.style_networks import SemSegE2VID
    front = E2VIDRecurrent(E2VID_LIGHTWEIGHT_CONFIG).eval()
    back = SemSegE2VID(256, 11, skip_connect=True, skip_type='concat', text_embeddings_path='', materialize_ch256=False,
                       if_linear_probing=linear_probing)
    ref = OracleSupervisedStep("frame2voxel", 11, 3, 5, linear_probing)
    for m, r, seed in ((front, ref.front, seed_front), (back, ref.net, seed_back)):
        fill_by_name(m, seed)
        fill_by_name(r, seed, sorted(m.state_dict().keys()))
        damp_residual(m), damp_residual(r)
        r.double().eval()
    return front.cuda(), back.cuda().eval(), ref


def _oracle_logits(ref, ev, pad=None):
    """float64 logits of the oracle for fp32 events [B, nwin * 5, H, W] (pad: the reconstructor's reflection padding)."""
    states = None
    with torch.no_grad():
        for i in range(ev.shape[1] // 5):
            x = on.event_preprocess(ev[:, 5 * i:5 * i + 5].double())
            _, states, latent = ref.front(pad(x) if pad is not None else x, states)
        lg = ref.net(latent)[0][1]
        return ref.net.linear_probe(lg) if ref.linear_probing else lg


@pytest.mark.parametrize("B,H,W", [(2, 30, 44), (1, 480, 640)])
def test_events_to_logits_fp32_matches_float64_oracle(B, H, W):
    """Three recurrent windows through ImageReconstructor(precision='fp32'), then forward_fp32, against oracle.nets in float64."""
    from types import SimpleNamespace
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor
    front, back, ref = _models(11, 12)
    rec = ImageReconstructor(front, H, W, 5, torch.device("cuda"), SimpleNamespace(precision='fp32'))
    assert rec.crop.needs_pad == (H % 8 != 0)
    torch.manual_seed(H)
    ev = (torch.randn(B, 15, H, W) * (torch.rand(B, 15, H, W) > 0.8)).contiguous()
    evc = ev.cuda()
    for i in range(3):
        _, _, latent = rec.update_reconstruction(evc, channel_slice=(5 * i, 5))
    out, _ = back.forward_fp32(latent)
    want = _oracle_logits(ref, ev, rec.crop.pad if rec.crop.needs_pad else None)
    assert out[1].shape == want.shape == (B, 11, (H + 7) // 8 * 8, (W + 7) // 8 * 8)
    assert _report(f"events->logits {B}x{H}x{W}", relerr(out[1].cpu().numpy(), want.numpy()), 1e-4) <= 1e-4


def test_forward_fp32_repeatable_and_sync_free(g, keys):
    lat = {k: _cl(torch.from_numpy(g[f"semseg_lat{k}"])) for k in (1, 2, 4, 8)}
    outs = []
    for _ in range(2):
        net = _decoder(keys, if_linear_probing=True)
        out, x256 = net.forward_fp32(lat)
        outs.append((out[1].clone(), out[2].clone(), out[4].clone(), x256.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        out, _ = net.forward_fp32(lat)                 # operands already packed by the forward above
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert torch.equal(out[1], outs[0][0])


# ------------------------------------------------------------------------------------------------------------ the trainers
TRAINER_SEEDS = {'front_sensor_b': 11, 'back_end': 12}      # the seeds of the golden E2VID / decoder weights
MARGIN = 3e-4                        # of the largest |logit|: each of the top two may move by 1e-4 of it within the network bound
MAX_LEFT_OUT = 0.01


def _trainer(linear_probing, tmp_path, eval_precision=None):
    import train
    from openess_amd.config.settings import Settings
    train.seed_everything()
    s = Settings(os.path.join(CFG, "finetune_dsec_synthetic.yaml"), generate_log=False)
    s.ckpt_dir = str(tmp_path)
    s.config_option = "frame2voxel"
    s.if_finetuning, s.if_linear_probing, s.if_supervised_only = not linear_probing, linear_probing, False
    if eval_precision is not None:
        s.eval_precision = eval_precision
    trainer, _ = train.build_trainer(s)
    ref = OracleSupervisedStep("frame2voxel", s.semseg_num_classes, s.nr_events_data_b, 5, linear_probing, lr=s.lr_voxel)
    for name, m in trainer.models_dict.items():
        fill_by_name(m, TRAINER_SEEDS[name])
        fill_by_name(ref.modules()[name], TRAINER_SEEDS[name], sorted(m.state_dict().keys()))
        damp_residual(m), damp_residual(ref.modules()[name])
    return trainer, s, ref


def _val_batch(s, B=2):
    K, nwin, (H, W) = s.semseg_num_classes, s.nr_events_data_b, s.img_size_b
    torch.manual_seed(4)
    ev = (torch.randn(B, nwin * 5, H, W) * (torch.rand(B, nwin * 5, H, W) > 0.7)).contiguous()
    gt = torch.randint(0, K, (B, H // 4, W // 4)).repeat_interleave(4, 1).repeat_interleave(4, 2)
    gt[0, :5] = 255
    return ev, gt


def _clear_pixels(logits64):
    """pixels whose top-two margin is at least MARGIN of the largest |logit| (a condition on the oracle alone)"""
    top = logits64.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) >= MARGIN * float(logits64.abs().max())


@pytest.mark.parametrize("linear_probing", [False, True])
def test_trainer_fp32_validation_matches_float64_oracle(linear_probing, tmp_path):
    trainer, s, ref = _trainer(linear_probing, tmp_path, 'fp32')
    assert trainer.eval_precision == 'fp32' and trainer.reconstructor_fp32.precision == 'fp32'
    ev, gt = _val_batch(s)
    for m in ref.modules().values():
        m.double().eval()
    want = _oracle_logits(ref, ev)
    clear = _clear_pixels(want)
    left_out = 1.0 - float(clear.double().mean())
    print(f"[semseg_fp32] trainer lp={linear_probing}: left out {left_out:.4%} of the pixels (cap {MAX_LEFT_OUT:.0%})", flush=True)
    assert left_out <= MAX_LEFT_OUT
    gt_kept = torch.where(clear, gt, torch.full_like(gt, 255))
    for m in trainer.models_dict.values():
        m.eval()
    trainer.resetValidationStatistics()
    with torch.no_grad():
        losses, _ = trainer.val_step((ev.cuda(), gt_kept.cuda(), None), 'sensor_b', 0, -1, None)
    cm = trainer.metrics_semseg_b.metrics_acc.view(11, 11).cpu().numpy()
    cm_ref = ol.confusion_matrix(want.argmax(1).numpy(), gt_kept.numpy(), 11)
    assert cm.sum() == int((gt_kept != 255).sum()) > 0
    assert np.array_equal(cm, cm_ref)
    assert bool(torch.isfinite(losses['semseg_sensor_b_loss']))
    with torch.no_grad():
        lg = trainer.val_logits((ev.cuda(), gt.cuda(), None))
    assert lg.dtype == torch.float32
    assert _report(f"trainer logits lp={linear_probing}", relerr(lg.cpu().numpy(), want.numpy()), 1e-4) <= 1e-4


def test_fp32_validation_shares_no_state_with_the_default_path(tmp_path):
    """The default val_step is bit-equal before and after an fp32 trainer existed and ran in the process, and a train_step
    after an fp32 val_step equals a train_step without it, bit for bit."""
    def batch(s):
        ev, gt = _val_batch(s)
        return (ev.cuda(), gt.cuda(), None, gt.cuda(), gt.cuda(), None)

    def default_val(tr, b):
        for m in tr.models_dict.values():
            m.eval()
        with torch.no_grad():
            return tr.val_logits(b).clone()

    def step(tr, b):
        losses, _, total = tr.train_step(b)
        return total.clone(), [p.detach().clone() for p in tr.task_backend.parameters()]

    t0, s, _ = _trainer(False, tmp_path)
    assert t0.eval_precision == 'bf16' and not hasattr(t0, 'reconstructor_fp32')
    b = batch(s)
    val_before = default_val(t0, b)
    loss_plain, params_plain = step(t0, b)
    t1, s1, _ = _trainer(False, tmp_path, 'fp32')
    # the default (bf16) logits from the fp32 trainer's own bf16 path, before and after its fp32 validation ran
    for m in t1.models_dict.values():
        m.eval()
    with torch.no_grad():
        bf16_first = t1.val_logits(b, 'bf16').clone()
        t1.resetValidationStatistics()
        t1.val_step(b[:3], 'sensor_b', 0, -1, None)
        tr_val = t1.val_logits(b, 'bf16').clone()
    assert torch.equal(bf16_first, val_before) and torch.equal(tr_val, val_before)
    loss_after, params_after = step(t1, b)
    assert torch.equal(loss_after, loss_plain)
    for p, q in zip(params_after, params_plain):
        assert torch.equal(p, q)
    # and a bf16-only trainer built after the fp32 one validates to the same bits
    t2, s2, _ = _trainer(False, tmp_path)
    assert torch.equal(default_val(t2, b), val_before)


def test_eval_precision_tool_reports_and_matches_val_epochs(tmp_path, capsys):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import eval_precision as tool
    out = tool.main(["--warmup", "0"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1]
    rec = json.loads(line)
    assert rec == json.loads(json.dumps(out))
    for k in ("bf16", "fp32", "argmax_agreement", "logits_rel_rms", "bf16_ms", "fp32_ms", "labelled_pixels", "batches"):
        assert k in rec, k
    for p in ("bf16", "fp32"):
        assert set(rec[p]) == {"miou", "acc"} and 0.0 <= rec[p]["miou"] <= 100.0 and rec[p + "_ms"] > 0
    assert 0.0 <= rec["argmax_agreement"] <= 1.0 and 0.0 < rec["logits_rel_rms"] < 1.0 and rec["labelled_pixels"] > 0
    print("[semseg_fp32] eval_precision:", line, flush=True)
    trainer, s = tool.build(tool.DEFAULT, ckpt_dir=str(tmp_path))
    assert trainer.eval_precision == 'fp32'
    summary = trainer.valEpochs()
    assert float(summary['miou']) == rec["fp32"]["miou"] and float(summary['acc']) == rec["fp32"]["acc"]
