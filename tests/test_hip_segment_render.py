"""GPU tests of K35's kernel: oess_segment_render (hip.segment_render) against the restatement of tests/segment_render_reference.py
on the shapes of tests/segment_render_cases.py, in fp32 and bf16, dense and as a channel slice of a wider NaN-filled buffer.

  labels      array_equal to the restatement and torch.equal to hip.argmax_labels (min_conf = 0); +-inf, NaN and ties as K31
  confidence  against the float64 restatement on pixels whose class values are all finite, within CONF_BOUND = 4 x 1.990e-07 =
              7.961e-07 (the figure: torch's own float32 interpolate + softmax + max against float64 on these cases,
              tools/exp_segment_render_bounds.py; the kernel's own largest deviation, measured on an MI355X: 1.430e-07 at
              2x19x7x9 -> 112x144 fp32); the exact cases (equal logits: float32(1) / float32(K); one logit at +200: 1.0)
              need no bound
  threshold   labels == where(conf < min_conf, ignore, argmax) with the kernel's OWN confidence: exact
  colour      bit-equal to the restatement, with and without grey, alpha256 in {0, 1, 128, 255, 256}
  every subset of the outputs (an output not asked for is never written), repeatability, and every refusal of the entry and of the
  wrapper with the outputs unchanged."""
import numpy as np
import pytest
import torch

from tests import argmax_labels_reference as ar
from tests import segment_render_cases as sc
from tests import segment_render_reference as sr

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0xA5
LAYOUTS = ("dense", "slice")
CASE_IDS = [sc.case_id(*c) for c in sc.ALL_SHAPES]


def _place(x, dtype, layout):
    """logical [B, K, h, w] device tensor of `x`: dense NCHW, or channels 8 ... 8 + K of a NaN-filled NHWC buffer of K + 24 channels"""
    x = x.to(torch.bfloat16 if dtype == "bf16" else torch.float32)
    if layout == "dense":
        return x.to(DEV)
    B, K, h, w = x.shape
    big = torch.full((B, h, w, K + 24), float('nan'), dtype=x.dtype, device=DEV)
    big[..., 8:8 + K] = x.to(DEV).permute(0, 2, 3, 1)
    return big[..., 8:8 + K].permute(0, 3, 1, 2)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("shape,size,align", sc.ALL_SHAPES, ids=CASE_IDS)
def test_kernel_equals_the_restatement(shape, size, align, dtype, layout):
    from openess_amd import hip
    B, K = shape[:2]
    H, W = sc.out_size(shape, size)
    x = sc.logits(shape, dtype)
    xv = _place(x, dtype, layout)
    pal, grey = sc.palette(K), sc.grey(B, H, W)
    want = sr.render(x.numpy(), size, align, pal.numpy(), grey.numpy(), alpha256=128)
    got = hip.segment_render(xv, size=size, align_corners=align, palette=pal.to(DEV), background=grey.to(DEV), alpha=0.5)
    assert set(got) == {'labels', 'conf', 'rgb'}
    labels, conf, rgb = got['labels'], got['conf'], got['rgb']
    assert labels.shape == (B, H, W) and labels.dtype == torch.uint8 and labels.is_contiguous()
    assert conf.shape == (B, H, W) and conf.dtype == torch.float32 and rgb.shape == (B, H, W, 3) and rgb.dtype == torch.uint8
    assert np.array_equal(labels.cpu().numpy(), want['labels'])
    assert torch.equal(labels.long(), hip.argmax_labels(xv, size=size, align_corners=align))          # the sibling
    d = float(np.abs(conf.cpu().numpy().astype(np.float64) - want['conf']).max())
    print(f"{sc.case_id(shape, size, align)}-{dtype}-{layout}: |conf - float64| {d:.3e} (bound {sc.CONF_BOUND:.3e})")
    assert sc.finite_pixels(want['values']).all() and d <= sc.CONF_BOUND
    assert np.array_equal(rgb.cpu().numpy(), want['rgb'])
    again = hip.segment_render(xv, size=size, align_corners=align, palette=pal.to(DEV), background=grey.to(DEV), alpha=0.5)
    assert all(torch.equal(got[k], again[k]) for k in got)               # two calls, the same bits (every confidence is finite)


@pytest.mark.parametrize("want", sc.OUTPUT_SUBSETS, ids=["+".join(w) for w in sc.OUTPUT_SUBSETS])
def test_every_subset_of_the_outputs_and_nothing_else_is_written(want):
    """through the C entry with canary buffers for the outputs that are not asked for"""
    from openess_amd import _lib, hip
    shape, size, align = sc.ALL_SHAPES[4]                                  # 2x19x7x9 -> 112x144
    B, K, h, w = shape
    H, W = size
    x = sc.logits(shape, "fp32")
    xn = x.to(DEV).permute(0, 2, 3, 1).contiguous()
    pal, grey = sc.palette(K).to(DEV), sc.grey(B, H, W).to(DEV)
    ref = sr.render(x.numpy(), size, align, pal.cpu().numpy(), grey.cpu().numpy(), alpha256=77)
    bufs = {'labels': torch.full((B, H, W), POISON, dtype=torch.uint8, device=DEV),
            'conf': torch.full((B, H, W), -3.0, dtype=torch.float32, device=DEV),
            'rgb': torch.full((B, H, W, 3), POISON, dtype=torch.uint8, device=DEV)}
    ptr = {k: (bufs[k].data_ptr() if k in want else None) for k in bufs}
    rc = _lib.load().oess_segment_render(xn.data_ptr(), 0, K, B, K, h, w, H, W, 0, pal.data_ptr(), grey.data_ptr(), 77, 0.0, 255,
                                         ptr['labels'], ptr['conf'], ptr['rgb'], hip._stream())
    assert rc == 0
    torch.cuda.synchronize()
    if 'labels' in want:
        assert np.array_equal(bufs['labels'].cpu().numpy(), ref['labels'])
    else:
        assert bool((bufs['labels'] == POISON).all())
    if 'conf' in want:
        assert float(np.abs(bufs['conf'].cpu().numpy() - ref['conf']).max()) <= sc.CONF_BOUND
    else:
        assert bool((bufs['conf'] == -3.0).all())
    if 'rgb' in want:
        assert np.array_equal(bufs['rgb'].cpu().numpy(), ref['rgb'])
    else:
        assert bool((bufs['rgb'] == POISON).all())
    got = hip.segment_render(xn.permute(0, 3, 1, 2), size=size, palette=pal, background=grey, alpha=77 / 256, want=want)
    assert set(got) == set(want) and all(torch.equal(got[k], bufs[k]) for k in want)


def test_outputs_end_exactly_at_their_last_byte():
    """odd widths: rows start at every byte phase, the dword stores of one row must not reach into the next buffer's bytes"""
    from openess_amd import _lib, hip
    B, K, h, w, H, W = 2, 5, 3, 4, 7, 261                                  # 261: two chunks, the second of five pixels
    x = sc.logits((B, K, h, w), "fp32")
    xn = x.to(DEV).permute(0, 2, 3, 1).contiguous()
    pal = sc.palette(K).to(DEV)
    n = B * H * W
    for lead in (0, 1, 2, 3):
        lab = torch.full((lead + n + 8,), POISON, dtype=torch.uint8, device=DEV)
        rgb = torch.full((lead + 3 * n + 8,), POISON, dtype=torch.uint8, device=DEV)
        rc = _lib.load().oess_segment_render(xn.data_ptr(), 0, K, B, K, h, w, H, W, 0, pal.data_ptr(), None, 256, 0.0, 255,
                                             lab.data_ptr() + lead, None, rgb.data_ptr() + lead, hip._stream())
        assert rc == 0
        torch.cuda.synchronize()
        ref = sr.render(x.numpy(), (H, W), False, pal.cpu().numpy())
        assert np.array_equal(lab[lead:lead + n].cpu().numpy(), ref['labels'].ravel())
        assert np.array_equal(rgb[lead:lead + 3 * n].cpu().numpy(), ref['rgb'].ravel())
        assert bool((lab[:lead] == POISON).all()) and bool((lab[lead + n:] == POISON).all())
        assert bool((rgb[:lead] == POISON).all()) and bool((rgb[lead + 3 * n:] == POISON).all())


# ------------------------------------------------------------------------------------------------------ labels: special values
@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_input_size_compares_the_raw_values(dtype):
    """+-inf, NaN and ties at the input size: no blend, so no 0 * inf; torch.argmax's rule"""
    from openess_amd import hip
    x, planted = ar.special_logits()
    xv = _place(x, dtype, "slice")
    want = ar.argmax_labels(xv.float().cpu().numpy())
    for size in (None, (4, 6)):
        y = hip.segment_render(xv, size=size, want=('labels',))['labels']
        assert np.array_equal(y.cpu().numpy(), want) and torch.equal(y.long(), xv.argmax(1))
        assert all(int(y[p]) == k for p, k in planted.items())


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("shape,scale", ar.EXACT_CASES, ids=[f"{'x'.join(map(str, s))}-x{k}" for s, k in ar.EXACT_CASES])
def test_exact_tie_family(shape, scale, dtype):
    """integer logits at power-of-two upsampling: the float64 labels everywhere, 7 % of the pixels being exact ties"""
    from openess_amd import hip
    x = ar.exact_logits(shape)
    size = (shape[2] * scale, shape[3] * scale)
    v64 = ar.float64_upsampled(x.numpy(), size, False)
    got = hip.segment_render(_place(x, dtype, "dense"), size=size, want=('labels', 'conf'))
    assert np.array_equal(got['labels'].cpu().numpy(), np.argmax(v64, axis=1))
    want = torch.from_numpy(v64).softmax(1).max(1).values.numpy()
    assert float(np.abs(got['conf'].cpu().numpy() - want).max()) <= sc.CONF_BOUND       # exact values: float64 softmax itself


def test_non_finite_taps_blend_as_the_composed_path_blends_them():
    from openess_amd import hip
    x = sc.special_upsampled_logits()
    want = sr.render(x.numpy(), (12, 16))
    got = hip.segment_render(x.to(DEV), size=(12, 16), want=('labels', 'conf'))
    assert np.array_equal(got['labels'].cpu().numpy(), want['labels'])
    assert torch.equal(got['labels'].long(), hip.bilinear_resize(x.to(DEV), size=(12, 16)).argmax(1))
    fin = sc.finite_pixels(want['values'])
    assert 0 < fin.sum() < fin.size
    assert float(np.abs(got['conf'].cpu().numpy()[fin] - want['conf'][fin]).max()) <= sc.CONF_BOUND


# ------------------------------------------------------------------------------------------------------ confidence: exact cases
@pytest.mark.parametrize("K", sc.EQUAL_K)
def test_equal_logits_give_exactly_one_over_k(K):
    from openess_amd import hip
    want = np.float32(1) / np.float32(K)
    for value in (0.0, -3.5, 17.25):
        x = torch.full((2, K, 5, 7), value, device=DEV)
        for size in (None, (20, 21)):
            got = hip.segment_render(x, size=size, want=('labels', 'conf'))
            assert not got['labels'].any() and bool((got['conf'] == float(want)).all()), (K, value, size)


def test_one_dominant_logit_gives_exactly_one():
    from openess_amd import hip
    for k in (0, 5, 10):                                                  # first, middle, last: both branches of the running sum
        x = torch.zeros(2, 11, 4, 6, device=DEV)
        x[:, k] = 200.0
        for size in (None, (9, 13)):
            got = hip.segment_render(x, size=size, want=('labels', 'conf'))
            assert bool((got['labels'] == k).all()) and bool((got['conf'] == 1.0).all())


# ------------------------------------------------------------------------------------------------------------------- threshold
@pytest.mark.parametrize("ignore", [255, 19, 200])
@pytest.mark.parametrize("min_conf", sc.MIN_CONFS)
def test_threshold_uses_the_kernels_own_confidence(min_conf, ignore):
    from openess_amd import hip
    shape, size = (2, 19, 7, 9), (112, 144)
    x = (ar.randn_logits(shape, seed=7) * 3).to(DEV)
    pal = sc.palette(19).to(DEV)
    got = hip.segment_render(x, size=size, palette=pal, min_conf=min_conf, ignore_label=ignore)
    idx = hip.argmax_labels(x, size=size)
    below = got['conf'] < min_conf
    assert 0 < int(below.sum()) < below.numel()
    assert torch.equal(got['labels'].long(), torch.where(below, torch.full_like(idx, ignore), idx))
    assert torch.equal(got['conf'], hip.segment_render(x, size=size, want=('conf',))['conf'])          # min_conf does not touch conf
    assert np.array_equal(got['rgb'].cpu().numpy(), sr.colour(got['labels'].cpu().numpy(), pal.cpu().numpy(), ignore=ignore))
    assert bool((got['rgb'][below] == 0).all())                                                        # ignored pixels are black


def test_a_nan_confidence_keeps_its_label():
    from openess_amd import hip
    x = torch.zeros(1, 4, 2, 2, device=DEV)
    x[0, 2, 0, 0] = float('nan')
    got = hip.segment_render(x, min_conf=0.9, want=('labels', 'conf'))
    assert torch.isnan(got['conf'][0, 0, 0]) and int(got['labels'][0, 0, 0]) == 2
    assert bool((got['labels'].flatten()[1:] == 255).all())                # conf 0.25 < 0.9 everywhere else


# ---------------------------------------------------------------------------------------------------------------------- colour
@pytest.mark.parametrize("with_grey", [False, True], ids=["plain", "grey"])
@pytest.mark.parametrize("alpha256", sc.ALPHAS256)
def test_colour_bytes_equal_the_restatement(alpha256, with_grey):
    from openess_amd import hip
    shape, size = (2, 11, 5, 6), (13, 17)
    x = ar.randn_logits(shape, seed=11) * 3
    pal, grey = sc.palette(11, seed=1), sc.grey(2, 13, 17, seed=1)
    got = hip.segment_render(x.to(DEV), size=size, palette=pal.to(DEV), background=grey.to(DEV) if with_grey else None,
                             alpha=alpha256 / 256, min_conf=0.5)
    labels = got['labels'].cpu().numpy()
    assert (labels == 255).any() and (labels != 255).any()
    want = sr.colour(labels, pal.numpy(), grey.numpy() if with_grey else None, alpha256)
    assert np.array_equal(got['rgb'].cpu().numpy(), want)
    if with_grey and alpha256 < 256:                                       # ignored pixels blend towards black
        ign = labels == 255
        assert np.array_equal(got['rgb'].cpu().numpy()[ign][:, 0], (((256 - alpha256) * grey.numpy()[ign].astype(np.int64) + 128) >> 8))


# ------------------------------------------------------------------------------------------------------------------- refusals
def _entry_args(B=2, K=5, h=3, w=4, H=6, W=8):
    from openess_amd import hip
    x = torch.randn(B, h, w, K + 3, device=DEV)
    outs = (torch.full((B, H, W), POISON, dtype=torch.uint8, device=DEV), torch.full((B, H, W), -3.0, device=DEV),
            torch.full((B, H, W, 3), POISON, dtype=torch.uint8, device=DEV))
    pal, grey = sc.palette(K).to(DEV), sc.grey(B, H, W).to(DEV)
    a = dict(logits=x.data_ptr(), is_bf16=0, ps=K + 3, B=B, K=K, h=h, w=w, H=H, W=W, ac=0, palette=pal.data_ptr(), grey=grey.data_ptr(),
             alpha256=128, min_conf=0.0, ignore=255, labels=outs[0].data_ptr(), conf=outs[1].data_ptr(), rgb=outs[2].data_ptr(),
             stream=hip._stream())
    return x, outs, (pal, grey), a


def _call(a):
    from openess_amd import _lib
    return _lib.load().oess_segment_render(a['logits'], a['is_bf16'], a['ps'], a['B'], a['K'], a['h'], a['w'], a['H'], a['W'], a['ac'],
                                           a['palette'], a['grey'], a['alpha256'], a['min_conf'], a['ignore'], a['labels'], a['conf'],
                                           a['rgb'], a['stream'])


ENTRY_REFUSALS = {
    "null_logits": dict(logits=None),
    "no_output": dict(labels=None, conf=None, rgb=None),
    "rgb_without_palette": dict(palette=None),
    "k_zero": dict(K=0),
    "k_negative": dict(K=-1),
    "k_256": dict(K=256, ps=300),
    "ignore_is_a_class": dict(ignore=4),
    "ignore_negative": dict(ignore=-1),
    "ignore_256": dict(ignore=256),
    "alpha_negative": dict(alpha256=-1),
    "alpha_257": dict(alpha256=257),
    "min_conf_nan": dict(min_conf=float('nan')),
    "min_conf_negative": dict(min_conf=-0.25),
    "b_zero": dict(B=0),
    "h_in_negative": dict(h=-1),
    "w_in_zero": dict(w=0),
    "h_out_zero": dict(H=0),
    "w_out_negative": dict(W=-3),
    "stride_below_k": dict(ps=4),
    "stride_zero": dict(ps=0),
    "output_rows_overflow": dict(B=1 << 16, H=1 << 16),                # B * H = 2^32 workgroups
    "input_rows_overflow": dict(B=1 << 16, h=1 << 16, H=1),
    "input_extent_overflows": dict(ps=1 << 62),                        # B * h * w * stride beyond int64
    "output_extent_overflows": dict(B=1, H=(1 << 31) - 1, W=(1 << 31) - 1),     # 2^62 pixels of 4 bytes
}


@pytest.mark.parametrize("name", sorted(ENTRY_REFUSALS))
def test_entry_refuses_before_any_launch(name):
    x, outs, keep, a = _entry_args()
    assert _call(a) == 0                                              # the unmodified call is valid
    torch.cuda.synchronize()
    want = sr.render(x[..., :5].permute(0, 3, 1, 2).cpu().numpy(), (6, 8), False, keep[0].cpu().numpy(), keep[1].cpu().numpy(), 128)
    assert np.array_equal(outs[0].cpu().numpy(), want['labels']) and np.array_equal(outs[2].cpu().numpy(), want['rgb'])
    outs[0].fill_(POISON), outs[1].fill_(-3.0), outs[2].fill_(POISON)
    assert _call(dict(a, **ENTRY_REFUSALS[name])) == -22
    torch.cuda.synchronize()
    assert bool((outs[0] == POISON).all()) and bool((outs[1] == -3.0).all()) and bool((outs[2] == POISON).all())


def test_wrapper_refuses_before_any_launch():
    from openess_amd import hip
    x = torch.randn(2, 5, 3, 4, device=DEV)
    pal, grey = sc.palette(5).to(DEV), sc.grey(2, 6, 8).to(DEV)
    ok = dict(size=(6, 8), palette=pal, background=grey)
    assert set(hip.segment_render(x, **ok)) == {'labels', 'conf', 'rgb'}
    with pytest.raises(ValueError, match="no CPU fallback"):
        hip.segment_render(x.cpu(), **ok)
    with pytest.raises(ValueError, match="float32 / bfloat16"):
        hip.segment_render(x.half(), **ok)
    with pytest.raises(ValueError, match="4-D"):
        hip.segment_render(x[0], **ok)
    with pytest.raises(ValueError, match="K <= 255"):
        hip.segment_render(torch.zeros(1, 256, 2, 2, device=DEV), want=('labels',))
    with pytest.raises(ValueError, match="K <= 255"):
        hip.segment_render(torch.zeros(1, 0, 2, 2, device=DEV), want=('labels',))
    with pytest.raises(ValueError, match="non-empty"):
        hip.segment_render(torch.zeros(0, 3, 2, 2, device=DEV), want=('labels',))
    with pytest.raises(ValueError, match="size must be positive"):
        hip.segment_render(x, size=(0, 8), want=('labels',))
    for bad in ((), ('labels', 'labels'), ('depth',), 'colour'):
        with pytest.raises(ValueError, match="want must name"):
            hip.segment_render(x, want=bad, **ok)
    for bad in (4, -1, 256):
        with pytest.raises(ValueError, match="ignore_label"):
            hip.segment_render(x, ignore_label=bad, **ok)
    for bad in (float('nan'), -0.1):
        with pytest.raises(ValueError, match="min_conf"):
            hip.segment_render(x, min_conf=bad, **ok)
    for bad in (-0.01, 1.01, float('nan')):
        with pytest.raises(ValueError, match="alpha"):
            hip.segment_render(x, alpha=bad, **ok)
    for bad in (None, pal.cpu(), pal.int(), pal[:4], pal.t().contiguous().t(), torch.zeros(5, 4, dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError, match="palette must be"):
            hip.segment_render(x, size=(6, 8), palette=bad, background=grey)
    for bad in (grey.cpu(), grey.float(), grey[:1], grey[:, :, :7], grey.transpose(1, 2), grey[None]):
        with pytest.raises(ValueError, match="background must be"):
            hip.segment_render(x, size=(6, 8), palette=pal, background=bad)
    with pytest.raises(ValueError, match="background must be"):
        hip.segment_render(x, palette=pal, background=grey)               # size=None is the input size, 3 x 4
    # without 'rgb' neither palette nor background is looked at
    assert set(hip.segment_render(x, size=(6, 8), want=('labels', 'conf'))) == {'labels', 'conf'}
    got = hip.segment_render(x.requires_grad_(True), **ok)
    assert not any(t.requires_grad for t in got.values())
