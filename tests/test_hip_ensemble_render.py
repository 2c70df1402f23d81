"""GPU tests of K39's kernel: oess_segment_render_ensemble (hip.ensemble_render) against the restatement of
tests/ensemble_render_reference.py on the cases of tests/ensemble_render_cases.py, in fp32 and bf16, dense, as a channel slice of a
wider NaN-filled buffer and channels-last, through the wrapper and through the raw C entry.

  labels      where the float64 top-two gap of the mean probability exceeds 2 x ENSEMBLE_CONF_BOUND: the restatement's label;
              anywhere else a class within 2 x the bound of the maximum (at most 0.5 % of a case's pixels, asserted on the CPU)
  confidence  against the float64 restatement within ENSEMBLE_CONF_BOUND = 4 x 7.747e-08 = 3.099e-07 (the figure: torch's own
              float32 softmax -> mean -> max against float64, tools/exp_ensemble_render_bounds.py; the kernel's own largest
              deviation, measured on an MI355X: 7.04e-08 at 2x3, two raw views, fp32); the hand-computed cases need no bound
  colour      bit-equal to the restatement's colour of the kernel's OWN labels
  exact cases, one view == hip.segment_render, flip placement, every subset of the outputs, guard bytes at odd widths, non-finite
  pixels, threshold and blend, repeatability, and every refusal of the entry and of the wrapper with the outputs unchanged."""
import ctypes

import numpy as np
import pytest
import torch

from tests import argmax_labels_reference as ar
from tests import ensemble_render_cases as ec
from tests import ensemble_render_reference as er
from tests import segment_render_cases as sc
from tests import segment_render_reference as sr

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0xA5
LAYOUTS = ("dense", "slice", "channels_last")


def _place(x, dtype, layout):
    """logical [B, K, h, w] device tensor of `x`: dense NCHW, channels 8 ... 8 + K of a NaN-filled NHWC buffer, or channels-last"""
    x = x.to(torch.bfloat16 if dtype == "bf16" else torch.float32)
    if layout == "dense":
        return x.to(DEV)
    if layout == "channels_last":
        return x.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    B, K, h, w = x.shape
    big = torch.full((B, h, w, K + 24), float('nan'), dtype=x.dtype, device=DEV)
    big[..., 8:8 + K] = x.to(DEV).permute(0, 2, 3, 1)
    return big[..., 8:8 + K].permute(0, 3, 1, 2)


def _arr(ctype, values):
    return None if values is None else (ctype * len(values))(*values)


def _entry(a):
    """oess_segment_render_ensemble from a dict of plain values (lists for the five host arrays, None: a null array)"""
    from openess_amd import _lib
    return _lib.load().oess_segment_render_ensemble(
        _arr(ctypes.c_void_p, a['ptrs']), _arr(ctypes.c_longlong, a['ps']), _arr(ctypes.c_int, a['hs']), _arr(ctypes.c_int, a['ws']),
        _arr(ctypes.c_int, a['flips']), a['V'], a['is_bf16'], a['B'], a['K'], a['H'], a['W'], a['ac'], a['palette'], a['grey'],
        a['alpha256'], a['min_conf'], a['ignore'], a['labels'], a['conf'], a['rgb'], a['stream'])


def _entry_args(xs_nhwc, flips, K, H, W, align=False, pal=None, grey=None, alpha256=128, min_conf=0.0, ignore=255,
                labels=None, conf=None, rgb=None):
    from openess_amd import hip
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())          # noqa: E731
    return dict(ptrs=[x.data_ptr() for x in xs_nhwc], ps=[x.stride(2) if x.shape[2] > 1 else x.shape[3] for x in xs_nhwc],
                hs=[x.shape[1] for x in xs_nhwc], ws=[x.shape[2] for x in xs_nhwc], flips=[int(f) for f in flips], V=len(xs_nhwc),
                is_bf16=int(xs_nhwc[0].dtype == torch.bfloat16), B=xs_nhwc[0].shape[0], K=K, H=H, W=W, ac=int(align), palette=p(pal),
                grey=p(grey), alpha256=alpha256, min_conf=min_conf, ignore=ignore, labels=p(labels), conf=p(conf), rgb=p(rgb),
                stream=hip._stream())


def _check(got, ref, pal, grey, alpha256, what):
    """labels by the rule, confidence within the bound, colours of the kernel's own labels"""
    labels, conf = got['labels'].cpu().numpy(), got['conf'].cpu().numpy()
    share = er.check_labels(labels, ref['p'], ec.ENSEMBLE_CONF_BOUND)
    want_conf = np.take_along_axis(ref['p'], labels.astype(np.int64)[:, None], axis=1)[:, 0]
    d = float(np.abs(conf.astype(np.float64) - want_conf).max())
    print(f"{what}: |conf - float64| {d:.3e} (bound {ec.ENSEMBLE_CONF_BOUND:.3e}), weakly checked share {share:.5f}")
    assert share <= ec.WEAK_SHARE_CAP
    assert d <= ec.ENSEMBLE_CONF_BOUND
    assert np.array_equal(got['rgb'].cpu().numpy(), sr.colour(labels, pal.numpy(), grey.numpy(), alpha256))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", ec.DTYPES)
@pytest.mark.parametrize("bk,views,size,align", ec.CASES, ids=ec.CASE_IDS)
def test_kernel_equals_the_restatement(bk, views, size, align, dtype, layout):
    from openess_amd import hip
    B, K = bk
    H, W = ec.out_size(views, size)
    xs, flips = ec.logits(bk, views, dtype), ec.flips_of(views)
    xv = [_place(x, dtype, layout) for x in xs]
    pal, grey = ec.palette(K), ec.grey(B, H, W)
    ref = er.render([x.numpy() for x in xs], flips, (H, W), align)
    kw = dict(flips=flips, size=size, align_corners=align, palette=pal.to(DEV), background=grey.to(DEV), alpha=0.5)
    got = hip.ensemble_render(xv, **kw)
    assert set(got) == {'labels', 'conf', 'rgb'}
    assert got['labels'].shape == (B, H, W) and got['labels'].dtype == torch.uint8 and got['labels'].is_contiguous()
    assert got['conf'].shape == (B, H, W) and got['conf'].dtype == torch.float32
    assert got['rgb'].shape == (B, H, W, 3) and got['rgb'].dtype == torch.uint8
    _check(got, ref, pal, grey, 128, f"{ec.case_id(bk, views, size, align)}-{dtype}-{layout}")
    again = hip.ensemble_render(xv, **kw)
    assert all(torch.equal(got[k], again[k]) for k in got)               # two calls, the same bits (every confidence is finite)


@pytest.mark.parametrize("dtype", ec.DTYPES)
@pytest.mark.parametrize("bk,views,size,align", ec.CASES, ids=ec.CASE_IDS)
def test_raw_entry_equals_the_restatement(bk, views, size, align, dtype):
    """the C entry on strided NHWC views (a channel slice: pixel stride K + 24), bit-equal to the wrapper on dense views"""
    from openess_amd import hip
    B, K = bk
    H, W = ec.out_size(views, size)
    xs, flips = ec.logits(bk, views, dtype), ec.flips_of(views)
    pal, grey = ec.palette(K), ec.grey(B, H, W)
    xn = [_place(x, dtype, "slice").permute(0, 2, 3, 1) for x in xs]
    out = {'labels': torch.full((B, H, W), POISON, dtype=torch.uint8, device=DEV), 'conf': torch.full((B, H, W), -3.0, device=DEV),
           'rgb': torch.full((B, H, W, 3), POISON, dtype=torch.uint8, device=DEV)}
    pd, gd = pal.to(DEV), grey.to(DEV)
    a = _entry_args(xn, flips, K, H, W, align, pd, gd, 128, **out)
    a['ps'] = [K + 24] * len(xn)                                           # (a 1-pixel-wide view has no stride to read off)
    assert _entry(a) == 0
    torch.cuda.synchronize()
    if len(xs) == 1:                                                       # V = 1 through the entry (the wrapper goes to K35)
        want = sr.render(xs[0].numpy(), (H, W), align, pal.numpy(), grey.numpy(), 128)
        assert np.array_equal(out['labels'].cpu().numpy(), want['labels'])
    ref = er.render([x.numpy() for x in xs], flips, (H, W), align)
    _check(out, ref, pal, grey, 128, f"entry {ec.case_id(bk, views, size, align)}-{dtype}")
    if len(xs) > 1:
        got = hip.ensemble_render([_place(x, dtype, "dense") for x in xs], flips=flips, size=size, align_corners=align, palette=pd,
                                  background=gd, alpha=0.5)
        assert all(torch.equal(got[k], out[k]) for k in got)


# ----------------------------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("dtype", ec.DTYPES)
@pytest.mark.parametrize("shape,scale", ar.EXACT_CASES, ids=[f"{'x'.join(map(str, s))}-x{k}" for s, k in ar.EXACT_CASES])
def test_copies_of_one_view_give_its_labels(shape, scale, dtype):
    """integer logits at power-of-two upsampling: copies and mirrored copies of a view carry that view's labels, ties included"""
    from openess_amd import hip
    x = _place(ar.exact_logits(shape), dtype, "dense")
    xf = x.flip(-1)
    size = (shape[2] * scale, shape[3] * scale)
    want = hip.argmax_labels(x, size=size)
    assert np.array_equal(want.cpu().numpy(), ar.argmax_labels(x.float().cpu().numpy(), size))
    for views, flips in (([x, x], [0, 0]), ([x, xf], [0, 1]), ([x] * 4, [0] * 4), ([x, xf] * 4, [0, 1] * 4)):
        got = hip.ensemble_render(views, flips=flips, size=size, want=('labels',))['labels']
        assert torch.equal(got.long(), want), (len(views), flips)


# ---------------------------------------------------------------------------------------------------- hand-computed confidences
def test_two_views_give_exactly_three_quarters():
    from openess_amd import hip
    a, b = torch.zeros(2, 2, 3, 5, device=DEV), torch.zeros(2, 2, 3, 5, device=DEV)
    b[:, 0] = 200.0
    for size in (None, (6, 11)):
        for flips in ([0, 0], [1, 0], [0, 1]):
            got = hip.ensemble_render([a, b], flips=flips, size=size, want=('labels', 'conf'))
            assert not got['labels'].any() and bool((got['conf'] == 0.75).all()), (size, flips)


@pytest.mark.parametrize("V", ec.EQUAL_V)
@pytest.mark.parametrize("K", ec.EQUAL_K)
def test_equal_logits_give_exactly_one_over_k(K, V):
    from openess_amd import hip
    want = float(np.float32(1) / np.float32(K))
    for value in (0.0, -3.5, 17.25):
        views = [torch.full((2, K, 5, 7), value, device=DEV) for _ in range(V)]
        views[-1] = torch.full((2, K, 20, 21), value, device=DEV)              # a raw view among the resized ones
        flips = [v % 2 for v in range(V)]
        if V == 1:
            flips = [1]                                                        # one FLIPPED view runs the ensemble kernel
        got = hip.ensemble_render(views, flips=flips, size=(20, 21), want=('labels', 'conf'))
        assert not got['labels'].any() and bool((got['conf'] == want).all()), (K, V, value)


# ------------------------------------------------------------------------------------------------------- single view, flip
@pytest.mark.parametrize("dtype", ec.DTYPES)
def test_one_unflipped_view_is_segment_render(dtype):
    from openess_amd import hip
    x = _place(ar.randn_logits((2, 11, 5, 6), seed=3) * 3, dtype, "slice")
    pal, grey = ec.palette(11).to(DEV), ec.grey(2, 13, 17).to(DEV)
    for size, bg in (((13, 17), grey), (None, None)):
        kw = dict(size=size, palette=pal, background=bg, alpha=0.25, min_conf=0.4)
        got, want = hip.ensemble_render([x], **kw), hip.segment_render(x, **kw)
        assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
        assert all(torch.equal(hip.ensemble_render([x], flips=[False], **kw)[k], want[k]) for k in want)


def test_one_flipped_view_is_the_mirrored_render():
    """labels of a single flipped view are segment_render's, mirrored: the argmax of one view's probabilities is its argmax"""
    from openess_amd import hip
    x = (ar.randn_logits((2, 7, 4, 5), seed=4) * 3).to(DEV)
    for size in (None, (9, 14)):
        got = hip.ensemble_render([x], flips=[True], size=size, want=('labels', 'conf'))
        want = hip.segment_render(x, size=size, want=('labels', 'conf'))
        assert torch.equal(got['labels'], want['labels'].flip(-1))
        # two kernels, each within its own bound of the same float64 probability
        assert float((got['conf'] - want['conf'].flip(-1)).abs().max()) <= ec.ENSEMBLE_CONF_BOUND + sc.CONF_BOUND


def test_a_flipped_view_acts_at_the_mirrored_column():
    from openess_amd import hip
    B, K, H, W, col = 1, 3, 2, 7, 1
    views = [torch.zeros(B, K, H, W, device=DEV) for _ in range(3)]
    views[1][0, 2, 0, col] = 5.0
    base = hip.ensemble_render(views, flips=[0, 0, 0], want=('labels',))['labels']
    want = torch.zeros(B, H, W, dtype=torch.uint8, device=DEV)
    want[0, 0, col] = 2
    assert torch.equal(base, want)
    got = hip.ensemble_render(views, flips=[0, 1, 0], want=('labels',))['labels']
    want = torch.zeros(B, H, W, dtype=torch.uint8, device=DEV)
    want[0, 0, W - 1 - col] = 2
    assert torch.equal(got, want)
    # a resized flipped view: the mirror image of what it gives unflipped
    low = [torch.zeros(B, K, 2, 4, device=DEV) for _ in range(2)]
    low[1][0, 1, 1, 0] = 5.0
    plain = hip.ensemble_render(low, flips=[0, 0], size=(4, 8), want=('labels',))['labels']
    mirrored = hip.ensemble_render(low, flips=[0, 1], size=(4, 8), want=('labels',))['labels']
    assert plain.any() and torch.equal(mirrored, plain.flip(-1))


# --------------------------------------------------------------------------------------------------------- subsets and guards
@pytest.mark.parametrize("want", ec.OUTPUT_SUBSETS, ids=["+".join(w) for w in ec.OUTPUT_SUBSETS])
def test_every_subset_of_the_outputs_and_nothing_else_is_written(want):
    """through the C entry with canary buffers for the outputs that are not asked for"""
    from openess_amd import hip
    bk, views, size, align = ec.CASES[3]                                   # 1x11, three views -> 7x9
    B, K = bk
    H, W = size
    xs, flips = ec.logits(bk, views, "fp32"), ec.flips_of(views)
    xd = [x.to(DEV) for x in xs]
    xn = [x.permute(0, 2, 3, 1).contiguous() for x in xd]
    pal, grey = ec.palette(K).to(DEV), ec.grey(B, H, W).to(DEV)
    full = hip.ensemble_render(xd, flips=flips, size=size, palette=pal, background=grey, alpha=77 / 256)
    bufs = {'labels': torch.full((B, H, W), POISON, dtype=torch.uint8, device=DEV),
            'conf': torch.full((B, H, W), -3.0, dtype=torch.float32, device=DEV),
            'rgb': torch.full((B, H, W, 3), POISON, dtype=torch.uint8, device=DEV)}
    a = _entry_args(xn, flips, K, H, W, align, pal, grey, 77, **{k: bufs[k] for k in want})
    assert _entry(a) == 0
    torch.cuda.synchronize()
    canary = {'labels': POISON, 'conf': -3.0, 'rgb': POISON}
    for k in bufs:
        assert torch.equal(bufs[k], full[k]) if k in want else bool((bufs[k] == canary[k]).all()), k
    got = hip.ensemble_render(xd, flips=flips, size=size, palette=pal, background=grey, alpha=77 / 256, want=want)
    assert set(got) == set(want) and all(torch.equal(got[k], full[k]) for k in want)


@pytest.mark.parametrize("W", ec.GUARD_WIDTHS)
def test_outputs_end_exactly_at_their_last_byte(W):
    """odd widths: rows start at every byte phase, the dword stores of one row must not reach into the next buffer's bytes"""
    from openess_amd import hip
    B, K, H = 2, 3, 3
    xs = [ar.randn_logits((B, K, 2, max(1, W // 2)), seed=W), ar.randn_logits((B, K, H, W), seed=W + 1)]
    flips = [0, 1]
    xn = [x.to(DEV).permute(0, 2, 3, 1).contiguous() for x in xs]
    pal = ec.palette(K).to(DEV)
    ref = hip.ensemble_render([x.to(DEV) for x in xs], flips=flips, size=(H, W), palette=pal)
    er.check_labels(ref['labels'].cpu().numpy(), er.render([x.numpy() for x in xs], flips, (H, W))['p'], ec.ENSEMBLE_CONF_BOUND)
    n = B * H * W
    for lead in (0, 1, 2, 3):
        lab = torch.full((lead + n + 8,), POISON, dtype=torch.uint8, device=DEV)
        rgb = torch.full((lead + 3 * n + 8,), POISON, dtype=torch.uint8, device=DEV)
        a = _entry_args(xn, flips, K, H, W, pal=pal, alpha256=256, labels=lab.data_ptr() + lead, rgb=rgb.data_ptr() + lead)
        assert _entry(a) == 0
        torch.cuda.synchronize()
        assert torch.equal(lab[lead:lead + n], ref['labels'].flatten()) and torch.equal(rgb[lead:lead + 3 * n], ref['rgb'].flatten())
        assert bool((lab[:lead] == POISON).all()) and bool((lab[lead + n:] == POISON).all())
        assert bool((rgb[:lead] == POISON).all()) and bool((rgb[lead + 3 * n:] == POISON).all())


# ----------------------------------------------------------------------------------------------------------- non-finite pixels
@pytest.mark.parametrize("dtype", ec.DTYPES)
@pytest.mark.parametrize("kind", ["nan", "plus_inf_first", "plus_inf_later", "all_minus_inf"])
def test_a_non_finite_view_makes_its_pixel_nan_and_no_other(kind, dtype):
    from openess_amd import hip
    B, K, H, W = 2, 5, 6, 8
    low = _place(ar.randn_logits((B, K, 3, 4), seed=8), dtype, "dense")
    raw = _place(ar.randn_logits((B, K, H, W), seed=9), dtype, "dense")
    clean = hip.ensemble_render([low, raw], flips=[0, 1], size=(H, W), want=('labels', 'conf'), min_conf=0.3)
    bad = raw.clone()
    b, y, x = 1, 2, 1
    if kind == "nan":
        bad[b, 3, y, x] = float('nan')
    elif kind == "plus_inf_first":
        bad[b, 0, y, x] = float('inf')
    elif kind == "plus_inf_later":
        bad[b, 4, y, x] = float('inf')
    else:
        bad[b, :, y, x] = float('-inf')
    got = hip.ensemble_render([low, bad], flips=[0, 1], size=(H, W), want=('labels', 'conf'), min_conf=0.3)
    ox = W - 1 - x                                                         # the raw view is flipped
    assert torch.isnan(got['conf'][b, y, ox]) and int(got['labels'][b, y, ox]) == 0          # a NaN confidence keeps its label
    keep = torch.ones(B, H, W, dtype=torch.bool, device=DEV)
    keep[b, y, ox] = False
    assert torch.equal(got['conf'][keep], clean['conf'][keep]) and torch.equal(got['labels'][keep], clean['labels'][keep])
    assert not torch.isnan(clean['conf']).any()


# --------------------------------------------------------------------------------------------------------- threshold and blend
def _tta_views(seed=7):
    """three views that agree, as the views of one image do (independent views average every confidence below 0.9): logits, their
    mirror image under the flip flag, and a perturbed resized copy; 13 % / 56 % / 95 % of the confidences lie below 0.3 / 0.5 / 0.9"""
    base = ar.randn_logits((2, 19, 7, 9), seed=seed) * 4
    third = torch.nn.functional.interpolate(base, (9, 12), mode='bilinear') + ar.randn_logits((2, 19, 9, 12), seed=seed + 1) * 0.5
    return [base.to(DEV), base.flip(-1).to(DEV), third.to(DEV)], [0, 1, 0], (28, 36)


@pytest.mark.parametrize("ignore", [255, 19, 200])
@pytest.mark.parametrize("min_conf", ec.MIN_CONFS)
def test_threshold_uses_the_kernels_own_confidence(min_conf, ignore):
    from openess_amd import hip
    xs, flips, size = _tta_views()
    pal = ec.palette(19).to(DEV)
    got = hip.ensemble_render(xs, flips=flips, size=size, palette=pal, min_conf=min_conf, ignore_label=ignore)
    free = hip.ensemble_render(xs, flips=flips, size=size, want=('labels', 'conf'))
    below = got['conf'] < min_conf
    assert 0 < int(below.sum()) < below.numel()
    assert torch.equal(got['labels'], torch.where(below, torch.full_like(free['labels'], ignore), free['labels']))
    assert torch.equal(got['conf'], free['conf'])                                                      # min_conf does not touch conf
    assert np.array_equal(got['rgb'].cpu().numpy(), sr.colour(got['labels'].cpu().numpy(), pal.cpu().numpy(), ignore=ignore))
    assert bool((got['rgb'][below] == 0).all())                                                        # ignored pixels are black


@pytest.mark.parametrize("with_grey", [False, True], ids=["plain", "grey"])
@pytest.mark.parametrize("alpha256", ec.ALPHAS256)
def test_colour_bytes_equal_the_restatement(alpha256, with_grey):
    from openess_amd import hip
    xs, flips, size = _tta_views(seed=11)
    pal, grey = ec.palette(19, seed=1), ec.grey(2, *size, seed=1)
    got = hip.ensemble_render(xs, flips=flips, size=size, palette=pal.to(DEV), background=grey.to(DEV) if with_grey else None,
                              alpha=alpha256 / 256, min_conf=0.5)
    labels = got['labels'].cpu().numpy()
    assert (labels == 255).any() and (labels != 255).any()
    assert np.array_equal(got['rgb'].cpu().numpy(), sr.colour(labels, pal.numpy(), grey.numpy() if with_grey else None, alpha256))


# -------------------------------------------------------------------------------------------------------------------- refusals
def _refusal_setup(B=2, K=5, H=6, W=8):
    xn = [torch.randn(B, 3, 4, K + 3, device=DEV), torch.randn(B, H, W, K + 3, device=DEV)]
    outs = (torch.full((B, H, W), POISON, dtype=torch.uint8, device=DEV), torch.full((B, H, W), -3.0, device=DEV),
            torch.full((B, H, W, 3), POISON, dtype=torch.uint8, device=DEV))
    pal, grey = ec.palette(K).to(DEV), ec.grey(B, H, W).to(DEV)
    a = _entry_args(xn, [0, 1], K, H, W, False, pal, grey, 128, labels=outs[0], conf=outs[1], rgb=outs[2])
    return xn, outs, (pal, grey), a


def _views(**kw):
    """a change of one entry of the five arrays: {array name: (index, value)}"""
    return dict(_views=kw)


ENTRY_REFUSALS = {
    "null_pointer_array": dict(ptrs=None),
    "null_stride_array": dict(ps=None),
    "null_height_array": dict(hs=None),
    "null_width_array": dict(ws=None),
    "null_flip_array": dict(flips=None),
    "null_view_0": _views(ptrs=(0, None)),
    "null_view_1": _views(ptrs=(1, None)),
    "v_zero": dict(V=0),
    "v_negative": dict(V=-1),
    "v_nine": dict(V=9),
    "flip_two": _views(flips=(1, 2)),
    "flip_negative": _views(flips=(0, -1)),
    "h_in_zero": _views(hs=(0, 0)),
    "w_in_negative": _views(ws=(1, -8)),
    "stride_below_k": _views(ps=(1, 4)),
    "stride_zero": _views(ps=(0, 0)),
    "no_output": dict(labels=None, conf=None, rgb=None),
    "rgb_without_palette": dict(palette=None),
    "k_zero": dict(K=0),
    "k_256": dict(K=256),
    "ignore_is_a_class": dict(ignore=4),
    "ignore_256": dict(ignore=256),
    "alpha_negative": dict(alpha256=-1),
    "alpha_257": dict(alpha256=257),
    "min_conf_nan": dict(min_conf=float('nan')),
    "min_conf_negative": dict(min_conf=-0.25),
    "b_zero": dict(B=0),
    "h_out_zero": dict(H=0),
    "w_out_negative": dict(W=-3),
    "output_rows_overflow": dict(B=1 << 16, H=1 << 16),
    "input_rows_overflow": dict(B=1 << 16, H=1, **_views(hs=(0, 1 << 16))),
    "input_extent_overflows": _views(ps=(1, 1 << 62)),
    "output_extent_overflows": dict(B=1, H=(1 << 31) - 1, W=(1 << 31) - 1),
}


def _modified(a, change):
    b = dict(a)
    for key, value in change.items():
        if key == '_views':
            for name, (i, v) in value.items():
                b[name] = list(b[name])
                b[name][i] = v
        else:
            b[key] = value
    return b


@pytest.mark.parametrize("name", sorted(ENTRY_REFUSALS))
def test_entry_refuses_before_any_launch(name):
    from openess_amd import hip
    xn, outs, keep, a = _refusal_setup()
    assert _entry(a) == 0                                              # the unmodified call is valid
    torch.cuda.synchronize()
    want = hip.ensemble_render([x[..., :5].permute(0, 3, 1, 2) for x in xn], flips=[0, 1], size=(6, 8), palette=keep[0],
                               background=keep[1])
    assert all(torch.equal(o, want[k]) for o, k in zip(outs, ('labels', 'conf', 'rgb')))
    outs[0].fill_(POISON), outs[1].fill_(-3.0), outs[2].fill_(POISON)
    assert _entry(_modified(a, ENTRY_REFUSALS[name])) == -22
    torch.cuda.synchronize()
    assert bool((outs[0] == POISON).all()) and bool((outs[1] == -3.0).all()) and bool((outs[2] == POISON).all())


def test_wrapper_refuses_before_any_launch():
    from openess_amd import hip
    x, y = torch.randn(2, 5, 3, 4, device=DEV), torch.randn(2, 5, 6, 8, device=DEV)
    pal, grey = ec.palette(5).to(DEV), ec.grey(2, 6, 8).to(DEV)
    ok = dict(size=(6, 8), palette=pal, background=grey)
    assert set(hip.ensemble_render([x, y], flips=[0, 1], **ok)) == {'labels', 'conf', 'rgb'}
    for bad in ([], (), x, None, [x] * 9):
        with pytest.raises(ValueError, match="1 ... 8 views"):
            hip.ensemble_render(bad, **ok)
    for bad in ([0], [0, 1, 0], [0, 2], "01"):
        with pytest.raises(ValueError, match="flips must hold"):
            hip.ensemble_render([x, y], flips=bad, **ok)
    with pytest.raises(ValueError, match="no CPU fallback"):
        hip.ensemble_render([x.cpu(), y.cpu()], **ok)
    for bad in (y.cpu(), y.bfloat16(), y[:1], y[:, :4]):
        with pytest.raises(ValueError, match="share view 0's"):
            hip.ensemble_render([x, bad], **ok)
    for bad in (y.half(), y[0], "view"):
        with pytest.raises(ValueError, match="float32 / bfloat16"):
            hip.ensemble_render([x, bad], **ok)
    with pytest.raises(ValueError, match="K <= 255"):
        hip.ensemble_render([torch.zeros(1, 256, 2, 2, device=DEV)] * 2, want=('labels',))
    with pytest.raises(ValueError, match="non-empty"):
        hip.ensemble_render([x, torch.zeros(2, 5, 0, 8, device=DEV)], want=('labels',))
    with pytest.raises(ValueError, match="size must be positive"):
        hip.ensemble_render([x, y], size=(0, 8), want=('labels',))
    for bad in ((), ('labels', 'labels'), ('depth',), 'colour'):
        with pytest.raises(ValueError, match="want must name"):
            hip.ensemble_render([x, y], want=bad, **ok)
    for bad in (4, -1, 256):
        with pytest.raises(ValueError, match="ignore_label"):
            hip.ensemble_render([x, y], ignore_label=bad, **ok)
    for bad in (float('nan'), -0.1):
        with pytest.raises(ValueError, match="min_conf"):
            hip.ensemble_render([x, y], min_conf=bad, **ok)
    for bad in (-0.01, 1.01, float('nan')):
        with pytest.raises(ValueError, match="alpha"):
            hip.ensemble_render([x, y], alpha=bad, **ok)
    for bad in (None, pal.cpu(), pal.int(), pal[:4]):
        with pytest.raises(ValueError, match="palette must be"):
            hip.ensemble_render([x, y], size=(6, 8), palette=bad, background=grey)
    for bad in (grey.cpu(), grey.float(), grey[:1], grey[:, :, :7]):
        with pytest.raises(ValueError, match="background must be"):
            hip.ensemble_render([x, y], size=(6, 8), palette=pal, background=bad)
    with pytest.raises(ValueError, match="background must be"):
        hip.ensemble_render([x, y], palette=pal, background=grey)          # size=None is view 0's size, 3 x 4
    got = hip.ensemble_render([x.requires_grad_(True), y], flips=[1, 0], **ok)
    assert not any(t.requires_grad for t in got.values())
