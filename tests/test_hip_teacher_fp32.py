"""GPU tests of the fp32 image-teacher path (K17: batchnorm_f32.hip, DilationFeatureExtractor.forward_fp32):

* the train-mode BatchNorm kernel against float64 F.batch_norm(training=True) on the CPU: output, save_mean, save_var and both
  running statistics, relerr (max-abs over max-abs) <= LAYER_BOUND = 1e-5, the project's bound for fp32 layers;
* train-mode Bottlenecks and the whole teacher against the float64 oracle and the reference's own golden;
* what the fp32 forward shares with the bf16 one (nothing), and tools/eval_teacher_precision.py.

THE OFFSET INPUT.  One input has a per-channel offset and unit spread, to show that nothing cancels.  Measured first: torch's own
fp32 CPU batch_norm against float64 on that input (offset +-K alternating over the channels, the five shapes below), worst shape:
K = 100: 3.40e-6, K = 50: 1.41e-6, K = 30: 9.3e-7.  A quarter of the bound is 2.5e-6, which K = 100 alone exceeds, so the offset
is K = 50.

THE NETWORK BOUNDS.  Measured on the CPU before any GPU run: relerr of the fp32 oracle (the reference's arithmetic) against the
float64 oracle, same weights (fill_by_name seeds 13 / 14), same inputs, BatchNorm in train mode unless said otherwise:

    teacherwc_img (golden, 2 x 3 x 96 x 128), damped weights      features 5.02e-6    every running statistic <= 1.2e-7
    the same in eval mode                                         features 7.1e-7     (random weights: 7.6e-7)
    random weights, 2 x 3 x 96 x 128, block by block with the float64 activation as each block's input:
        stem 8.0e-7, the 16 blocks 2.6e-7 .. 6.9e-7, head 1.30e-6
    teacher_img (golden, 2 x 3 x 32 x 48), bn1.running_mean       4.2e-8
    Bottleneck(dilation 2 / 4, with / without downsample), 9 x 11  2.1e-7 .. 3.3e-7

Four times the value (the margin the different summation order of the MFMA's K chain earns), with a floor of 1e-5:
WC_BOUND = 4 x 5.02e-6 = 2.0e-5 for the end-to-end train-mode features (against float64 and against the golden alike); every
other comparison falls under the floor, NET_BOUND = 1e-5."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nets as on
from tests.synth import compact, damp_residual, fill_by_name

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

LAYER_BOUND = 1e-5
NET_BOUND = 1e-5
WC_BOUND = 2.0e-5
OFFSET = 50.0
SHAPES = [(2, 6, 7, 9), (2, 64, 5, 8), (1, 256, 3, 5), (2, 2048, 2, 3), (3, 64, 33, 47)]
LAYOUTS = ("nhwc", "nchw", "slice")


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def _report(name, value, bound):
    print(f"[teacher_fp32] {name}: {value:.3e} (bound {bound:.1e})", flush=True)
    return value


def _place(t, layout, fill=-7.0):
    """A logical [B, C, H, W] CPU tensor on the GPU as NHWC dense, as NCHW, or as a channel slice of a wider NHWC tensor.
    Returns (the view, the wider tensor or None)."""
    if layout == "nhwc":
        return t.cuda().contiguous(memory_format=torch.channels_last), None
    if layout == "nchw":
        return t.cuda().contiguous(), None
    B, C, H, W = t.shape
    big = torch.full((B, H, W, C + 8), fill, device="cuda")
    view = big[..., 4:4 + C].permute(0, 3, 1, 2)
    view.copy_(t)
    return view, big


def _untouched(big, C, fill=-7.0):
    return big is None or (bool((big[..., :4] == fill).all()) and bool((big[..., 4 + C:] == fill).all()))


def _params(C, g):
    return dict(weight=torch.rand(C, generator=g) + 0.5, bias=torch.randn(C, generator=g), running_mean=torch.randn(C, generator=g),
                running_var=torch.rand(C, generator=g) + 0.5, momentum=0.1, eps=1e-5)


def _reference(x, p, relu, res):
    """float64 F.batch_norm(training=True) on the CPU: (out, batch mean, biased variance, running_mean, running_var)."""
    rm, rv = p["running_mean"].double().clone(), p["running_var"].double().clone()
    x64 = x.double()
    y = F.batch_norm(x64, rm, rv, p["weight"].double(), p["bias"].double(), True, p["momentum"], p["eps"])
    if res is not None:
        y = y + res.double()
    if relu:
        y = torch.relu(y)
    return y, x64.mean(dim=(0, 2, 3)), x64.var(dim=(0, 2, 3), unbiased=False), rm, rv


def _check(tag, x, p, layout, relu, res, in_place):
    from openess_amd import hip
    want = _reference(x, p, relu, res)
    xd, xbig = _place(x, layout)
    rd = None if res is None else _place(res, layout)[0]
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in p.items()}
    out, obig = (xd, xbig) if in_place else _place(torch.full_like(x, float("nan")), layout)
    y, mean, var = hip.batch_norm_train_f32(xd, dev, relu=relu, residual=rd, out=out, return_stats=True)
    assert y.data_ptr() == out.data_ptr() and y.shape == want[0].shape and y.dtype == torch.float32
    got = (y, mean, var, dev["running_mean"], dev["running_var"])
    for name, a, b in zip(("out", "save_mean", "save_var", "running_mean", "running_var"), got, want):
        e = _report(f"{tag} {name}", relerr(a.cpu().numpy(), b.numpy()), LAYER_BOUND)
        assert e <= LAYER_BOUND, (tag, name, e)
    assert _untouched(obig, x.shape[1]) and _untouched(xbig, x.shape[1])
    if not in_place:
        assert torch.equal(xd.cpu(), x)                       # the input is read only


# ------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_batch_norm_train_matches_float64(shape, layout):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape) + len(layout))
    x = torch.randn(shape, generator=g) * (0.5 + torch.rand(1, C, 1, 1, generator=g)) + torch.randn(1, C, 1, 1, generator=g)
    res = torch.randn(shape, generator=g)
    p = _params(C, g)
    tag = "x".join(map(str, shape)) + " " + layout
    _check(tag + " plain", x, p, layout, False, None, False)
    _check(tag + " res+relu", x, p, layout, True, res, False)
    _check(tag + " in place", x, p, layout, False, None, True)
    _check(tag + " in place res+relu", x, p, layout, True, res, True)


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_batch_norm_train_does_not_cancel_on_an_offset_input(shape):
    """Unit spread on a per-channel offset of +-OFFSET (module docstring: torch's own fp32 CPU kernel is at 1.41e-6 here)."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    sign = 1.0 - 2.0 * (torch.arange(C) % 2).float()
    x = torch.randn(shape, generator=g) + OFFSET * sign[None, :, None, None]
    p = _params(C, g)
    x32 = F.batch_norm(x, None, None, p["weight"], p["bias"], True, 0.1, 1e-5)
    x64 = F.batch_norm(x.double(), None, None, p["weight"].double(), p["bias"].double(), True, 0.1, 1e-5)
    own = _report("torch fp32 CPU on the offset input", relerr(x32.numpy(), x64.numpy()), LAYER_BOUND / 4)
    assert own <= LAYER_BOUND / 4
    tag = "x".join(map(str, shape)) + f" offset {OFFSET:g}"
    _check(tag, x, p, "nhwc", False, None, False)
    _check(tag + " res+relu", x, p, "nhwc", True, torch.randn(shape, generator=g), False)


def test_batch_norm_train_gamma_beta_and_running_statistics_are_optional():
    from openess_amd import hip
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 12, 5, 7, generator=g) * 3 + 1
    want = F.batch_norm(x.double(), None, None, None, None, True, 0.1, 1e-3)
    y = hip.batch_norm_train_f32(x.cuda(), dict(weight=None, bias=None, running_mean=None, running_var=None, momentum=0.1, eps=1e-3))
    assert _report("no affine, no running statistics", relerr(y.cpu().numpy(), want.numpy()), LAYER_BOUND) <= LAYER_BOUND
    with pytest.raises(ValueError, match="more than 1 value"):
        hip.batch_norm_train_f32(torch.zeros(1, 4, 1, 1, device="cuda"), torch.nn.BatchNorm2d(4).cuda())


@pytest.mark.parametrize("shape,layout", [((3, 64, 33, 47), "nhwc"), ((2, 6, 7, 9), "nchw"), ((2, 2048, 2, 3), "slice")])
def test_two_calls_are_bit_identical_and_count_batches(shape, layout):
    from openess_amd import hip
    g = torch.Generator().manual_seed(7)
    x, _ = _place(torch.randn(shape, generator=g) * 2 + 3, layout)
    res, _ = _place(torch.randn(shape, generator=g), layout)
    runs = []
    for _ in range(2):
        bn = torch.nn.BatchNorm2d(shape[1]).cuda().train()
        assert int(bn.num_batches_tracked) == 0
        y, m, v = hip.batch_norm_train_f32(x, bn, relu=True, residual=res, return_stats=True)
        assert int(bn.num_batches_tracked) == 1
        runs.append([t.clone() for t in (y, m, v, bn.running_mean, bn.running_var)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    hip.batch_norm_train_f32(x, bn)
    hip.batch_norm_train_f32(x, bn)
    assert int(bn.num_batches_tracked) == 3
    assert not torch.equal(bn.running_mean, runs[0][3])


# ------------------------------------------------------------------------------------------------------------ the blocks
@pytest.mark.parametrize("dilation", [2, 4])
@pytest.mark.parametrize("downsample", [False, True], ids=["identity", "downsample"])
def test_train_mode_bottleneck_matches_float64_oracle(dilation, downsample):
    from openess_amd.models import _resnet
    inplanes, planes = (64, 32) if downsample else (128, 32)
    down = ref_down = None
    if downsample:
        down = torch.nn.Sequential(_resnet.conv1x1(inplanes, planes * 4), torch.nn.BatchNorm2d(planes * 4))
        ref_down = torch.nn.Sequential(torch.nn.Conv2d(inplanes, planes * 4, 1, bias=False), torch.nn.BatchNorm2d(planes * 4))
    blk = _resnet.Bottleneck(inplanes, planes, 1, down, dilation=dilation)
    ref = on.Bottleneck(inplanes, planes, 1, ref_down, dilation)
    assert sorted(blk.state_dict()) == sorted(ref.state_dict())
    fill_by_name(blk, 40 + dilation)
    fill_by_name(ref, 40 + dilation)
    blk.cuda().train()
    ref.double().train()
    g = torch.Generator().manual_seed(dilation)
    x = torch.relu(torch.randn(2, inplanes, 9, 11, generator=g))
    with torch.no_grad():
        want = ref(x.double())
        y = blk.forward_train_fp32(x.cuda().contiguous(memory_format=torch.channels_last))
    tag = f"bottleneck d{dilation} {'downsample' if downsample else 'identity'}"
    assert _report(tag, relerr(y.cpu().numpy(), want.numpy()), NET_BOUND) <= NET_BOUND
    rb = dict(ref.named_buffers())
    for name, b in blk.named_buffers():
        if "running" in name:
            assert _report(f"{tag} {name}", relerr(b.cpu().numpy(), rb[name].numpy()), NET_BOUND) <= NET_BOUND
        else:
            assert int(b) == int(rb[name]) == 1


# ------------------------------------------------------------------------------------------------------------ the network
@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLDEN, "nets.npz")))


@pytest.fixture(scope="module")
def keys():
    return json.load(open(os.path.join(GOLDEN, "nets_keys.json")))


def _teacher(damp):
    from openess_amd.models.image_model import DilationFeatureExtractor
    t = DilationFeatureExtractor(None)
    fill_by_name(t.encoder, 13)
    fill_by_name(t.decoder[0], 14)
    if damp:
        damp_residual(t.encoder)
    return t.cuda().train()


def _oracle(keys, damp):
    ref = on.DilationFeatureExtractor()
    fill_by_name(ref.encoder, 13, keys["teacher_encoder"])
    fill_by_name(ref.decoder[0], 14)
    if damp:
        damp_residual(ref.encoder)
    return ref.double().train()


@pytest.fixture(scope="module")
def wc_oracle(g, keys):
    """The float64 oracle on the well-conditioned golden case, computed once: the train-mode features, the buffers after that
    one forward, and the eval-mode features from the ORIGINAL running statistics."""
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    img = torch.from_numpy(g["teacherwc_img"])
    ref = _oracle(keys, True)
    with torch.no_grad():
        ev = copy.deepcopy(ref).eval()(img.double())
        tr = ref(img.double())
    return {"img": img, "train": tr.numpy(), "eval": ev.numpy(), "buffers": {k: v.clone() for k, v in ref.encoder.named_buffers()}}


def test_teacher_fp32_matches_float64_oracle_and_reference_golden(g, keys, wc_oracle):
    t = _teacher(True)
    assert sorted(t.encoder.state_dict().keys()) == keys["teacher_encoder"]
    feat = t.forward_fp32(wc_oracle["img"].cuda())
    assert feat.dtype == torch.float32 and feat.shape == wc_oracle["train"].shape == (2, 256, 96, 128)
    f = feat.cpu().numpy()
    assert _report("wc features vs float64", relerr(f, wc_oracle["train"]), WC_BOUND) <= WC_BOUND
    key = "teacherwc_feat"
    assert tuple(g[key + "__shape"]) == f.shape
    sub, s, a = compact(f)
    assert _report("wc features vs golden sample", relerr(sub, g[key + "__sub"]), WC_BOUND) <= WC_BOUND
    scale = float(g[key + "__abs"])
    assert abs(float(s) - float(g[key + "__sum"])) <= WC_BOUND * scale and abs(float(a) - scale) <= WC_BOUND * scale
    # one call moved every running statistic one momentum step, as the oracle's one forward did
    worst = 0.0
    for name, b in t.encoder.named_buffers():
        want = wc_oracle["buffers"][name]
        if "running" in name:
            worst = max(worst, relerr(b.cpu().numpy(), want.numpy()))
        else:
            assert int(b) == int(want) == 1, name
    assert _report("wc running statistics after one call, worst", worst, NET_BOUND) <= NET_BOUND
    # the bf16 network on the same weights is orders of magnitude away: the fp32 path is not the bf16 one in disguise
    with torch.no_grad():
        fb = _teacher(True)(wc_oracle["img"].cuda())
    assert relerr(fb.float().cpu().numpy(), wc_oracle["train"]) > 10 * WC_BOUND


def test_eval_mode_teacher_fp32_matches_float64_eval_oracle(wc_oracle):
    t = _teacher(True).eval()
    before = [b.clone() for b in t.buffers()]
    feat = t.forward_fp32(wc_oracle["img"].cuda())
    assert _report("wc eval features vs float64", relerr(feat.cpu().numpy(), wc_oracle["eval"]), NET_BOUND) <= NET_BOUND
    for a, b in zip(t.buffers(), before):
        assert torch.equal(a, b)                              # the folded path moves nothing


def test_random_weight_teacher_fp32_block_by_block(g, keys):
    """As tests/test_hip_nets.py::test_teacher_forward: the random-weight net amplifies rounding block by block, so every block
    takes the float64 ORACLE's activation as its input."""
    from openess_amd.models import _resnet
    t, ref = _teacher(False), _oracle(keys, False)
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    torch.manual_seed(5)
    img = torch.rand(2, 3, 96, 128)
    cl = lambda a: a.float().cuda().contiguous(memory_format=torch.channels_last)    # noqa: E731
    with torch.no_grad():
        e, r = t.encoder, ref.encoder
        rr = r.maxpool(torch.relu(r.bn1(r.conv1(img.double()))))
        from openess_amd import hip
        x = hip.max_pool_3x3s2_f32(_resnet.conv_bn_train_f32(e.conv1, e.bn1, img.cuda(), relu=True))
        assert _report("stem", relerr(x.cpu().numpy(), rr.numpy()), NET_BOUND) <= NET_BOUND
        for ln in ("layer1", "layer2", "layer3", "layer4"):
            for i, (blk, rblk) in enumerate(zip(getattr(e, ln), getattr(r, ln))):
                nxt = rblk(rr)
                y = blk.forward_train_fp32(cl(rr))
                assert _report(f"{ln}.{i}", relerr(y.cpu().numpy(), nxt.numpy()), NET_BOUND) <= NET_BOUND, (ln, i)
                rr = nxt
        want = F.normalize(ref.decoder(rr), p=2, dim=1)
        head = t.head_fp32(cl(rr))
        assert _report("head", relerr(head.cpu().numpy(), want.numpy()), NET_BOUND) <= NET_BOUND
    # reference golden: running-stat update of the stem BN (momentum 0.1) on the golden image
    t2 = _teacher(False)
    t2.forward_fp32(torch.from_numpy(g["teacher_img"]).cuda())
    e = relerr(t2.encoder.bn1.running_mean.cpu().numpy(), g["teacher_bn1_running_mean_after"])
    assert _report("teacher_bn1_running_mean_after", e, NET_BOUND) <= NET_BOUND


# ------------------------------------------------------------------------------------------------------------ isolation
def test_forward_fp32_leaves_the_bf16_forward_alone_and_steps_the_buffers_once(g):
    img = torch.from_numpy(g["teacherwc_img"]).cuda()
    t = _teacher(True)
    with torch.no_grad():
        before = t(img).clone()                               # train mode: batch statistics, so the output ignores the buffers
    stats = {n: b.clone() for n, b in t.encoder.named_buffers()}
    a = t.forward_fp32(img).clone()
    with torch.no_grad():
        after = t(img)
    assert torch.equal(before, after)
    # a fresh teacher gives the same fp32 bits: no state of the bf16 forward reached the fp32 one
    t2 = _teacher(True)
    assert torch.equal(t2.forward_fp32(img), a)
    # exactly one momentum step per fp32 call: r1 = 0.9 r0 + 0.1 s  =>  r2 = 0.9 r1 + 0.1 s  (s: the same batch)
    r1 = {n: b.clone() for n, b in t2.encoder.named_buffers()}
    t2.forward_fp32(img)
    t0 = _teacher(True)
    for n, b in t2.encoder.named_buffers():
        r0 = dict(t0.encoder.named_buffers())[n]
        if "running" in n:
            want = 0.9 * r1[n].double() + (r1[n].double() - 0.9 * r0.double())
            assert relerr(b.cpu().numpy(), want.cpu().numpy()) <= NET_BOUND, n
            assert not torch.equal(b, r1[n])
        else:
            assert int(b) == 2 and int(r1[n]) == 1 and int(r0) == 0
    # the bf16 forward counted its own two batches and the fp32 call one
    assert int(t.encoder.bn1.num_batches_tracked) == 3 and int(stats["bn1.num_batches_tracked"]) == 1
    # eval mode: the bf16 output depends on the buffers, and an fp32 eval call leaves them, and it, alone
    t.eval()
    with torch.no_grad():
        eb = t(img).clone()
    t.forward_fp32(img)
    with torch.no_grad():
        assert torch.equal(t(img), eb)


# ------------------------------------------------------------------------------------------------------------ the tool
def test_eval_teacher_precision_tool_reports(capsys):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import eval_teacher_precision as tool
    out = tool.main(["--batch", "2", "--height", "64", "--width", "96", "--batches", "1", "--warmup", "1"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1]
    rec = json.loads(line)
    assert rec == json.loads(json.dumps(out)) and rec["size"] == "2x3x64x96"
    for k in ("pixel_cos_mean", "pixel_cos_min", "superpixel_cos_mean", "superpixel_cos_min", "rel_rms", "bf16_ms", "fp32_ms"):
        assert k in rec, k
    assert -1.0 <= rec["pixel_cos_min"] <= rec["pixel_cos_mean"] <= 1.0 + 1e-9
    assert -1.0 <= rec["superpixel_cos_min"] <= rec["superpixel_cos_mean"] <= 1.0 + 1e-9
    assert rec["pixel_cos_mean"] > 0.99 and 0.0 < rec["rel_rms"] < 0.2       # damped weights: bf16 storage is not amplified
    assert rec["bf16_ms"] > 0 and rec["fp32_ms"] > 0 and rec["superpixels"] > 0
    print("[teacher_fp32] eval_teacher_precision:", line, flush=True)
