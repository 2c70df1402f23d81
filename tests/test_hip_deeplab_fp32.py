"""GPU tests of the fp32 DeepLabv3-R50 inference path (K16: conv_f32.hip's dilated / large-tap entry, deeplab_f32.hip):

* layer kernels against float64 torch on the CPU, relerr (max-abs over max-abs) <= 1e-5, the bound K14 / K15 hold for the same
  MFMA; the max pool exactly; the old conv entry against the new one at dilation 1, bit for bit;
* the network against the reference's own golden and against oracle.nets.DeepLabV3 in float64, both output_stride branches;
* the frame2recon trainers' val_logits(..., precision='fp32'), shared state, repeatability.

THE NETWORK BOUND.  Measured on the CPU before any GPU run: relerr of the fp32 oracle (the reference's arithmetic) against the
float64 oracle, same weights (fill_by_name seed 15, random, NOT damped), same inputs:

    deeplab_img (golden, 2 x 3 x 64 x 96)   logits 7.9e-7   feats 7.0e-7
    wc_image()[:2] (224 x 320), OS 8        logits 1.33e-6  feats 8.7e-7
    wc_image()[:2] (224 x 320), OS 16       logits 9.2e-7   feats 7.8e-7
    trainer batch (2 x 3 x 64 x 96)         fine-tune 8.1e-7, linear probe 6.0e-7

Four times the largest (the margin the different summation order of the MFMA's K chain earns) is 5.3e-6, below the floor of
1e-5, so the bound of every network comparison, against float64 and against the reference's golden alike, is NET_BOUND = 1e-5.
The oracle's fp32 error is far below 1e-3: no damped weights are needed.
Top-two margin of the confusion-matrix test: 3 x NET_BOUND of the largest |logit|; on the float64 oracle alone that leaves out
0.016 % (fine-tune) and 0 % (linear probe) of the pixels of the seed-15 trainer batch, under the 1 % cap."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import losses as ol
from oracle import nets as on
from oracle.step import OracleSupervisedStep
from tests.conv_route_cases import ROUTE_CASES
from tests.synth import compact, fill_by_name, wc_image

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
CFG = os.path.join(HERE, "configs")

LAYER_BOUND = 1e-5
NET_BOUND = 1e-5
MARGIN = 3 * NET_BOUND
MAX_LEFT_OUT = 0.01
SEED = 15


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _report(name, value, bound):
    print(f"[deeplab_fp32] {name}: {value:.3e} (bound {bound:.1e})", flush=True)
    return value


# ------------------------------------------------------------------------------------------------------------ the stem
@pytest.mark.parametrize("B,H,W,layout", [(2, 33, 47, 'nchw'), (1, 64, 96, 'nchw'), (2, 31, 30, 'cl'), (1, 7, 5, 'nchw')])
def test_stem_7x7_stride2_matches_float64(B, H, W, layout):
    from openess_amd import hip
    g = torch.Generator().manual_seed(H * 7 + W)
    x = torch.rand(B, 3, H, W, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
    b = torch.randn(64, generator=g)
    xd = _cl(x) if layout == 'cl' else x.cuda()
    y = hip.conv2d_f32(xd, hip.pack_conv_weight_f32(w.cuda()), b.cuda(), 64, 7, 7, stride=2, pad=3, act='relu')
    want = torch.relu(F.conv2d(x.double(), w.double(), b.double(), 2, 3))
    assert y.shape == want.shape and y.dtype == torch.float32
    assert _report(f"stem {B}x{H}x{W} {layout}", relerr(y.cpu().numpy(), want.numpy()), LAYER_BOUND) <= LAYER_BOUND


# ------------------------------------------------------------------------------------------------------------ dilated 3x3
# (B, H, W, Cin, Cout, dilation, variant)
DILATED_CASES = {
    "d2_14x20_res": (2, 14, 20, 64, 64, 2, 'res'),
    "d4_28x40_slice": (1, 28, 40, 64, 32, 4, 'slice'),
    "d6_14x20_slice": (2, 14, 20, 128, 256, 6, 'slice'),
    "d12_28x40_res": (1, 28, 40, 64, 64, 12, 'res'),
    "d12_14x20_plain": (2, 14, 20, 64, 40, 12, 'plain'),
    "d18_14x20_plain": (2, 14, 20, 64, 64, 18, 'plain'),
    "d18_28x40_slice": (1, 28, 40, 32, 64, 18, 'slice'),
    "d24_28x40_slice": (1, 28, 40, 32, 64, 24, 'slice'),
    "d36_28x40_res": (2, 28, 40, 64, 48, 36, 'res'),
    "d24_14x20_centre_only": (1, 14, 20, 64, 64, 24, 'plain'),
    "d36_14x20_centre_only": (2, 14, 20, 64, 64, 36, 'res'),
    "d12_5x7_centre_only": (2, 5, 7, 128, 32, 12, 'slice'),
    "d2_c24_elementwise": (1, 9, 11, 24, 40, 2, 'res'),
    "d6_nchw_input": (1, 14, 20, 16, 32, 6, 'nchw'),
}


@pytest.mark.parametrize("case", sorted(DILATED_CASES))
def test_dilated_conv3x3_matches_float64(case):
    from openess_amd import hip
    B, H, W, Cin, Cout, d, variant = DILATED_CASES[case]
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    b = torch.randn(Cout, generator=g)
    res = torch.randn(B, Cout, H, W, generator=g) if variant == 'res' else None
    want = F.conv2d(x.double(), w.double(), b.double(), 1, d, d)
    if res is not None:
        want = torch.relu(want + res.double())
    out = big = None
    if variant == 'slice':                 # an ASPP branch: the output is a channel slice of the wider concat buffer
        big = torch.full((B, H, W, Cout + 24), -7.0, device="cuda")
        out = big[..., 8:8 + Cout].permute(0, 3, 1, 2)
    xd = x.cuda() if variant == 'nchw' else _cl(x)
    y = hip.conv2d_f32(xd, hip.pack_conv_weight_f32(w.cuda()), b.cuda(), Cout, 3, 3, pad=d, dilation=d,
                       act='relu' if res is not None else None, residual=None if res is None else _cl(res), out=out)
    assert y.shape == want.shape
    assert _report(case, relerr(y.cpu().numpy(), want.numpy()), LAYER_BOUND) <= LAYER_BOUND
    if big is not None:
        assert y.data_ptr() == out.data_ptr()
        assert bool((big[..., :8] == -7.0).all()) and bool((big[..., 8 + Cout:] == -7.0).all())
    if "centre_only" in case:              # the map is smaller than the rate: the conv is the centre tap's 1 x 1
        c = F.conv2d(x.double(), w.double()[:, :, 1:2, 1:2], b.double())
        assert relerr(want.numpy(), (torch.relu(c + res.double()) if res is not None else c).numpy()) <= 1e-12


def test_dilated_conv_stride2_and_wide_padding_match_float64():
    """What the generalised argument checks admit beyond DeepLabv3: stride 2 with a dilation, and pad > dilation (R - 1) / 2."""
    from openess_amd import hip
    g = torch.Generator().manual_seed(8)
    for B, H, W, Cin, Cout, k, s, p, d in ((2, 15, 17, 32, 48, 3, 2, 2, 2), (1, 9, 11, 16, 32, 3, 1, 5, 2), (1, 12, 10, 16, 32, 5, 1, 4, 3),
                                           (1, 6, 8, 16, 32, 1, 1, 2, 1)):
        x = torch.randn(B, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, k, k, generator=g) / (k * k * Cin) ** 0.5
        y = hip.conv2d_f32(_cl(x), hip.pack_conv_weight_f32(w.cuda()), None, Cout, k, k, stride=s, pad=p, dilation=d)
        want = F.conv2d(x.double(), w.double(), None, s, p, d)
        assert y.shape == want.shape
        assert _report(f"k{k} s{s} p{p} d{d}", relerr(y.cpu().numpy(), want.numpy()), LAYER_BOUND) <= LAYER_BOUND


# ------------------------------------------------------------------------------------------------------------ the pools
@pytest.mark.parametrize("B,C,H,W,layout", [(2, 64, 33, 47, 'cl'), (1, 64, 32, 48, 'cl'), (2, 6, 7, 9, 'nchw'), (1, 8, 1, 1, 'cl'),
                                            (1, 12, 2, 5, 'cl'), (2, 64, 220, 320, 'cl')])
def test_maxpool_f32_is_exact(B, C, H, W, layout):
    from openess_amd import hip
    g = torch.Generator().manual_seed(B + C + H + W)
    x = torch.randn(B, C, H, W, generator=g) - 3.0             # mostly negative: a zero padding would win, -inf does not
    y = hip.max_pool_3x3s2_f32(_cl(x) if layout == 'cl' else x.cuda())
    want = F.max_pool2d(x, 3, 2, 1)
    assert y.shape == want.shape and torch.equal(y.cpu(), want)
    big = torch.full((B, want.shape[2], want.shape[3], C + 8), 5.0, device="cuda")
    out = big[..., 4:4 + C].permute(0, 3, 1, 2)
    hip.max_pool_3x3s2_f32(_cl(x), out=out)
    assert torch.equal(out.cpu(), want) and bool((big[..., :4] == 5.0).all()) and bool((big[..., 4 + C:] == 5.0).all())


@pytest.mark.parametrize("B,C,H,W,layout", [(8, 2048, 28, 40, 'cl'), (2, 2048, 14, 20, 'cl'), (2, 256, 55, 80, 'cl'), (2, 11, 9, 13, 'nchw'),
                                            (1, 70, 1, 1, 'cl'), (3, 36, 4, 6, 'cl')])
def test_global_avg_pool_f32_matches_float64(B, C, H, W, layout):
    from openess_amd import hip
    g = torch.Generator().manual_seed(C + H)
    x = torch.relu(torch.randn(B, C, H, W, generator=g)) * (0.5 + torch.rand(1, C, 1, 1, generator=g)) + torch.rand(1, C, 1, 1, generator=g)
    xd = _cl(x) if layout == 'cl' else x.cuda()
    y = hip.global_avg_pool_f32(xd)
    want = x.double().mean(dim=(2, 3), keepdim=True)
    assert y.shape == want.shape and y.dtype == torch.float32
    assert _report(f"avg pool {B}x{C}x{H}x{W}", relerr(y.cpu().numpy(), want.numpy()), LAYER_BOUND) <= LAYER_BOUND
    assert torch.equal(hip.global_avg_pool_f32(xd), y)


def test_aspp_pooling_branch_matches_float64():
    from openess_amd.models.deeplabv3 import ASPPPooling
    g = torch.Generator().manual_seed(3)
    m = ASPPPooling(256, 64)
    fill_by_name(m, 7)
    m.cuda().eval()
    x = torch.relu(torch.randn(2, 256, 14, 20, generator=g))
    big = torch.zeros((2, 14, 20, 128), device="cuda")
    out = m.forward_fp32(_cl(x), out=big[..., 64:].permute(0, 3, 1, 2))
    import copy
    m64 = copy.deepcopy(m).cpu().double()
    with torch.no_grad():
        y = F.relu(m64[2](m64[1](x.double().mean(dim=(2, 3), keepdim=True)))).expand(-1, -1, 14, 20)
    assert _report("ASPP pooling branch", relerr(out.cpu().numpy(), y.numpy()), LAYER_BOUND) <= LAYER_BOUND
    assert bool((big[..., :64] == 0).all())


# ------------------------------------------------------------------------------------------------------------ parity
def _old_takes(geom):
    B, H, W, Cin, Cout, k, stride, pad, dil = geom
    return dil == 1 and k * k <= 25 and pad < k and stride in (1, 2) and (H + 2 * pad - k) >= 0 and (W + 2 * pad - k) >= 0


PARITY = [(name, geom) for name, geom, _, _ in ROUTE_CASES if _old_takes(geom)]


def test_parity_cases_cover_the_route_table():
    assert len(PARITY) >= 25 and {g[5] for _, g in PARITY} >= {1, 2, 3, 5} and {g[6] for _, g in PARITY} == {1, 2}


@pytest.mark.parametrize("name,geom", PARITY, ids=[n for n, _ in PARITY])
def test_old_entry_equals_new_entry_at_dilation_1(name, geom):
    """oess_conv2d_fwd_f32 and oess_conv2d_dilated_fwd_f32(dilation = 1): the same bits, with bias, residual and ReLU."""
    from openess_amd import _lib, hip
    lib = _lib.load()
    B, H, W, Cin, Cout, k, stride, pad, _ = geom
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = _cl(torch.randn(B, Cin, H, W, generator=g))
    w = hip.pack_conv_weight_f32((torch.randn(Cout, Cin, k, k, generator=g) / (k * k * Cin) ** 0.5).cuda())
    b = torch.randn(Cout, generator=g).cuda()
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    res = _cl(torch.randn(B, Cout, Ho, Wo, generator=g))
    old = hip.conv2d_f32(x, w, b, Cout, k, k, stride=stride, pad=pad, act='relu', residual=res)
    new = torch.full((B, Ho, Wo, Cout), float('nan'), device="cuda").permute(0, 3, 1, 2)
    vx, vr, vo = hip._f32_view(x, "x"), hip._f32_view(res, "res"), hip._f32_view(new, "out")
    r = ctypes.byref
    _lib.check(lib.oess_conv2d_dilated_fwd_f32(r(vx), None, B, H, W, Cin, 0, w.data_ptr(), b.data_ptr(), Cout, k, k, stride, pad, 1, 1,
                                               r(vr), r(vo), torch.cuda.current_stream().cuda_stream), "oess_conv2d_dilated_fwd_f32")
    assert old.shape == new.shape and bool(torch.isfinite(new).all()) and torch.equal(old, new)
    assert float((old > 0).float().mean()) > 0.2


# ------------------------------------------------------------------------------------------------------------ the network
@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLDEN, "nets.npz")))


@pytest.fixture(scope="module")
def keys():
    return json.load(open(os.path.join(GOLDEN, "nets_keys.json")))


def _net(output_stride, keys, **kw):
    from openess_amd.models.deeplabv3 import deeplabv3_resnet50
    net = deeplabv3_resnet50(num_classes=11, text_embeddings_path=None, output_stride=output_stride, pretrained_backbone='', **kw)
    fill_by_name(net, SEED)
    return net.cuda().eval()


def _check_compact(g, key, arr, bound):
    assert tuple(g[key + "__shape"]) == arr.shape, (key, arr.shape)
    sub, s, a = compact(arr)
    assert _report(key + " sample", relerr(sub, g[key + "__sub"]), bound) <= bound
    scale = float(g[key + "__abs"])
    assert abs(float(s) - float(g[key + "__sum"])) <= bound * scale and abs(float(a) - scale) <= bound * scale


def test_network_fp32_matches_reference_golden(g, keys):
    net = _net(32, keys)
    assert sorted(net.state_dict().keys()) == keys["deeplab"]
    lg, ft = net.forward_fp32(torch.from_numpy(g["deeplab_img"]).cuda())
    assert lg.dtype == ft.dtype == torch.float32
    _check_compact(g, "deeplab_eval_logits", lg.cpu().numpy(), NET_BOUND)
    _check_compact(g, "deeplab_eval_feats", ft.cpu().numpy(), NET_BOUND)


@pytest.mark.parametrize("output_stride", [8, 16])
def test_network_fp32_matches_float64_oracle(output_stride, keys):
    net = _net(output_stride, keys)
    ref = on.DeepLabV3(11, output_stride)
    fill_by_name(ref, SEED, keys["deeplab"])
    ref.double().eval()
    img = torch.from_numpy(wc_image())[:2]
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    with torch.no_grad():
        lr, fr = ref(img.double())
    lg, ft = net.forward_fp32(img.cuda())
    assert lg.shape == lr.shape == (2, 11, 224, 320) and ft.shape == fr.shape == (2, 256, 224, 320)
    e_l = _report(f"OS{output_stride} logits", relerr(lg.cpu().numpy(), lr.numpy()), NET_BOUND)
    e_f = _report(f"OS{output_stride} feats", relerr(ft.cpu().numpy(), fr.numpy()), NET_BOUND)
    assert e_l <= NET_BOUND and e_f <= NET_BOUND
    # the bf16 network on the same weights is orders of magnitude away: the fp32 path is not the bf16 one in disguise
    with torch.no_grad():
        lb, _ = net(img.cuda())
    assert relerr(lb.float().cpu().numpy(), lr.numpy()) > 100 * NET_BOUND


def test_forward_fp32_is_repeatable_and_leaves_the_bf16_forward_alone(g, keys):
    img = torch.from_numpy(g["deeplab_img"]).cuda()
    net = _net(32, keys, if_linear_probing=True)
    with torch.no_grad():
        before = [t.clone() for t in net(img)]
    a = [t.clone() for t in net.forward_fp32(img)]
    b = [t.clone() for t in net.forward_fp32(img)]
    c = [t.clone() for t in _net(32, keys, if_linear_probing=True).forward_fp32(img)]
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    with torch.no_grad():
        after = net(img)
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    net.train()
    with pytest.raises(NotImplementedError, match="train mode"):
        net.forward_fp32(img)


# ------------------------------------------------------------------------------------------------------------ the trainers
def _trainer(linear_probing, tmp_path):
    import train
    from openess_amd.config.settings import Settings
    train.seed_everything()
    s = Settings(os.path.join(CFG, "finetune_dsec_synthetic.yaml"), generate_log=False)
    s.ckpt_dir = str(tmp_path)
    s.config_option = "frame2recon"
    s.if_finetuning, s.if_linear_probing, s.if_supervised_only = not linear_probing, linear_probing, False
    trainer, _ = train.build_trainer(s)
    ref = OracleSupervisedStep("frame2recon", s.semseg_num_classes, s.nr_events_data_b, 5, linear_probing, lr=s.lr_recon,
                               output_stride=s.output_stride)
    m = trainer.models_dict['model_recon']
    fill_by_name(m, SEED)
    fill_by_name(ref.net, SEED, sorted(m.state_dict().keys()))
    return trainer, s, ref


def _val_batch(s, B=2):
    K, (H, W) = s.semseg_num_classes, s.img_size_b
    torch.manual_seed(4)
    img = torch.rand(B, 3, H, W)
    gt = torch.randint(0, K, (B, H // 4, W // 4)).repeat_interleave(4, 1).repeat_interleave(4, 2)
    gt[0, :5] = 255
    return img, gt


@pytest.mark.parametrize("linear_probing", [False, True])
def test_trainer_fp32_val_logits_match_float64_oracle(linear_probing, tmp_path):
    trainer, s, ref = _trainer(linear_probing, tmp_path)
    assert trainer.eval_precision == 'bf16'
    img, gt = _val_batch(s)
    ref.net.double().eval()
    with torch.no_grad():
        want = ref.logits((None, None, img.double()))
    top = want.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) >= MARGIN * float(want.abs().max())
    left_out = 1.0 - float(clear[gt != 255].double().mean())
    print(f"[deeplab_fp32] trainer lp={linear_probing}: left out {left_out:.4%} of the labelled pixels (cap {MAX_LEFT_OUT:.0%})", flush=True)
    assert left_out <= MAX_LEFT_OUT
    model = trainer.models_dict['model_recon']
    model.train()
    modes = [m.training for m in model.modules()]
    with torch.no_grad():
        lg = trainer.val_logits((None, gt.cuda(), img.cuda()), precision='fp32')
    assert [m.training for m in model.modules()] == modes and model.training
    assert lg.dtype == torch.float32 and lg.shape == want.shape
    assert _report(f"trainer logits lp={linear_probing}", relerr(lg.cpu().numpy(), want.numpy()), NET_BOUND) <= NET_BOUND
    gt_kept = torch.where(clear, gt, torch.full_like(gt, 255))
    trainer.resetValidationStatistics()
    trainer.metrics_semseg_b.update_batch(lg.argmax(dim=1), gt_kept.cuda())
    cm = trainer.metrics_semseg_b.metrics_acc.view(11, 11).cpu().numpy()
    cm_ref = ol.confusion_matrix(want.argmax(1).numpy(), gt_kept.numpy(), 11)
    assert cm.sum() == int((gt_kept != 255).sum()) > 0
    assert np.array_equal(cm, cm_ref)


def test_fp32_val_logits_share_no_state_with_training_or_bf16_validation(tmp_path):
    def batch(s):
        img, gt = _val_batch(s)
        return (None, gt.cuda(), img.cuda(), gt.cuda(), gt.cuda(), None)

    def bf16_val(tr, b):
        tr.models_dict['model_recon'].eval()
        with torch.no_grad():
            return tr.val_logits(b).clone()

    def step(tr, b):
        torch.manual_seed(9)                 # the dropout mask of the step: the same in both trainers
        _, _, total = tr.train_step(b)
        return total.clone(), [p.detach().clone() for p in tr.model_recon.parameters()]

    t0, s, _ = _trainer(False, tmp_path)
    b = batch(s)
    val_plain = bf16_val(t0, b)
    loss_plain, params_plain = step(t0, b)
    val_plain_after = bf16_val(t0, b)

    t1, _, _ = _trainer(False, tmp_path)
    assert torch.equal(bf16_val(t1, b), val_plain)
    params_before = [p.detach().clone() for p in t1.model_recon.parameters()]
    buffers_before = [x.detach().clone() for x in t1.model_recon.buffers()]
    t1.model_recon.train()
    with torch.no_grad():
        first = t1.val_logits(b, 'fp32').clone()
    assert t1.model_recon.training
    for p, q in zip(t1.model_recon.parameters(), params_before):
        assert torch.equal(p, q)
    for p, q in zip(t1.model_recon.buffers(), buffers_before):
        assert torch.equal(p, q)
    assert torch.equal(bf16_val(t1, b), val_plain)
    loss_after, params_after = step(t1, b)
    assert torch.equal(loss_after, loss_plain)
    for p, q in zip(params_after, params_plain):
        assert torch.equal(p, q)
    assert torch.equal(bf16_val(t1, b), val_plain_after)
    # the step moved the weights and the running statistics: the fp32 operands are re-packed, the logits move
    with torch.no_grad():
        second = t1.val_logits(b, 'fp32')
        assert not torch.equal(second, first) and torch.equal(t1.val_logits(b, 'fp32'), second)


def test_linear_probe_train_step_repacks_the_frozen_network(tmp_path, monkeypatch):
    """Linear probing freezes every parameter of the backbone and the head, so no parameter version moves in a training step; the
    train-mode norm kernels still move the running statistics, through raw pointers.  The step's batch counter is what the fp32
    operand key sees: the step re-packs every folded conv, the features follow the new statistics, a second call packs nothing."""
    from openess_amd import hip
    trainer, s, _ = _trainer(True, tmp_path)
    img, gt = _val_batch(s)
    b = (None, gt.cuda(), img.cuda(), gt.cuda(), gt.cuda(), None)
    model = trainer.models_dict['model_recon']
    frozen = [p for n, p in model.named_parameters() if not n.startswith('linear_probe')]
    assert frozen and not any(p.requires_grad for p in frozen)
    calls = []
    real = hip.pack_conv_weight_f32
    monkeypatch.setattr(hip, "pack_conv_weight_f32", lambda w: (calls.append(tuple(w.shape)), real(w))[1])

    def feats():
        model.eval()
        return model.forward_fp32(b[2])[1].clone()

    first = feats()
    packed_once = list(calls)
    assert (64, 3, 7, 7) in packed_once and torch.equal(feats(), first) and calls == packed_once
    before = [p.detach().clone() for p in frozen]
    stats = [x.detach().clone() for n, x in model.named_buffers() if n.endswith('running_mean')]
    trainer.train_step(b)
    for p, q in zip(frozen, before):
        assert torch.equal(p, q)
    means = [x for n, x in model.named_buffers() if n.endswith('running_mean')]
    assert all(not torch.equal(x, y) for x, y in zip(means, stats))
    second = feats()
    te = tuple(model.classifier.text_embeddings.shape) + (1, 1)             # no BatchNorm behind it: the one operand that stays
    assert sorted(calls[len(packed_once):]) == sorted(c for c in packed_once if c != te) and packed_once.count(te) == 1
    assert not torch.equal(second, first)
    n = len(calls)
    assert torch.equal(feats(), second) and len(calls) == n


def test_eval_precision_tool_reports_frame2recon(capsys):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import eval_precision as tool
    out = tool.main(["--warmup", "0", "--config-option", "frame2recon"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1]
    rec = json.loads(line)
    assert rec == json.loads(json.dumps(out))
    for k in ("bf16", "fp32", "argmax_agreement", "logits_rel_rms", "bf16_ms", "fp32_ms", "labelled_pixels", "batches"):
        assert k in rec, k
    for p in ("bf16", "fp32"):
        assert set(rec[p]) == {"miou", "acc"} and 0.0 <= rec[p]["miou"] <= 100.0 and rec[p + "_ms"] > 0
    assert 0.0 <= rec["argmax_agreement"] <= 1.0 and 0.0 < rec["logits_rel_rms"] < 1.0 and rec["labelled_pixels"] > 0
    print("[deeplab_fp32] eval_precision frame2recon:", line, flush=True)
