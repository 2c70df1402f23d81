"""The restatement of oess_segment_render_ensemble's contract (tests/ensemble_render_reference.py) pinned without a GPU: (a) the
recorded confidence figure is what tools/exp_ensemble_render_bounds.py's function measures, and the bound four times it; (b) on
every case and dtype the share of pixels whose labels are checked by value (float64 top-two gap within twice the bound) stays under
the cap, so a seed that would weaken the GPU test is found here; the restatement passes its own label rule; (c) the mirror identity
upsampled(flip(x))[..., ::-1] == upsampled(x) on the exact cases, and ensembles of copies of one view giving that view's labels;
(d) the restatement against torch's float64 composed form (interpolate -> softmax -> flip -> mean -> max)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import argmax_labels_reference as ar
from tests import ensemble_render_cases as ec
from tests import ensemble_render_reference as er

EXACT_IDS = [f"{'x'.join(map(str, s))}-x{k}" for s, k in ar.EXACT_CASES]


def test_cases_module_holds_the_measured_figure():
    figure, where = ec.measure_conf_figure()
    print(f"torch float32 softmax -> mean -> max against float64: {figure!r} at {where}")
    assert figure == ec.ENSEMBLE_CONF_FIGURE and ec.ENSEMBLE_CONF_BOUND == 4.0 * ec.ENSEMBLE_CONF_FIGURE


@pytest.mark.parametrize("dtype", ec.DTYPES)
@pytest.mark.parametrize("bk,views,size,align", ec.CASES, ids=ec.CASE_IDS)
def test_weakly_checked_share_stays_under_the_cap(bk, views, size, align, dtype):
    xs = [x.numpy() for x in ec.logits(bk, views, dtype)]
    H, W = ec.out_size(views, size)
    ref = er.render(xs, ec.flips_of(views), (H, W), align)
    assert ref['p'].shape == (bk[0], bk[1], H, W) and ref['p'].dtype == np.float64 and np.isfinite(ref['p']).all()
    assert np.allclose(ref['p'].sum(1), 1.0, rtol=0, atol=1e-12)
    share = er.check_labels(ref['labels'], ref['p'], ec.ENSEMBLE_CONF_BOUND)          # the restatement passes its own rule
    print(f"{ec.case_id(bk, views, size, align)}-{dtype}: weakly checked share {share:.5f} (cap {ec.WEAK_SHARE_CAP})")
    assert share <= ec.WEAK_SHARE_CAP


@pytest.mark.parametrize("dtype", ec.DTYPES)
@pytest.mark.parametrize("bk,views,size,align", ec.CASES, ids=ec.CASE_IDS)
def test_restatement_equals_the_composed_form_in_float64(bk, views, size, align, dtype):
    """resize(x_v) -> softmax -> flip -> mean -> max in torch float64; the restatement rounds only the blend to float32"""
    xs = ec.logits(bk, views, dtype)
    H, W = ec.out_size(views, size)
    p = 0.0
    for x, (h, w, f) in zip(xs, views):
        v = x.double() if (h, w) == (H, W) else F.interpolate(x.double(), size=(H, W), mode='bilinear', align_corners=align)
        q = v.softmax(1)
        p = p + (q.flip(-1) if f else q)
    want = (p / len(xs)).max(1).values.numpy()
    got = er.render([x.numpy() for x in xs], ec.flips_of(views), (H, W), align)['conf']
    d = float(np.abs(got - want).max())
    print(f"{ec.case_id(bk, views, size, align)}-{dtype}: restatement against the float64 composed form {d:.3e}")
    # float32 blend (values of a few units, 2^-24 relative) and torch's float32 index arithmetic at 130 -> 259 (4e-6)
    assert d <= 1e-5


@pytest.mark.parametrize("shape,scale", ar.EXACT_CASES, ids=EXACT_IDS)
def test_exact_cases_mirror_identity_and_copies(shape, scale):
    x = ar.exact_logits(shape).numpy()
    size = (shape[2] * scale, shape[3] * scale)
    xf = np.ascontiguousarray(x[..., ::-1])
    assert np.array_equal(ar.upsampled(xf, size, False)[..., ::-1], ar.upsampled(x, size, False))
    want = ar.argmax_labels(x, size)
    for xs, flips in (([x, x], [0, 0]), ([x, xf], [0, 1]), ([x] * 4, [0] * 4), ([x, xf] * 4, [0, 1] * 4)):
        assert np.array_equal(er.render(xs, flips, size)['labels'], want), (len(xs), flips)


def test_non_finite_views_make_the_pixel_nan():
    x = ar.randn_logits((1, 4, 2, 3), seed=2).numpy()
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[0, 2, 1, 1] = bad
        ref = er.render([x, y], [0, 0], (2, 3))
        assert np.isnan(ref['conf'][0, 1, 1]) and ref['labels'][0, 1, 1] == 0 and np.isnan(ref['p'][0, :, 1, 1]).all()
        assert np.isfinite(np.delete(ref['conf'].ravel(), 4)).all()
    y = x.copy()
    y[0, :, 0, 2] = -np.inf
    ref = er.render([y, x], [1, 0], (2, 3))                                   # flipped: column 2 lands at column 0
    assert np.isnan(ref['conf'][0, 0, 0]) and ref['labels'][0, 0, 0] == 0 and np.isfinite(ref['conf'][0, 0, 1:]).all()


def test_hand_computed_confidences():
    a, b = np.zeros((1, 2, 1, 1), np.float32), np.zeros((1, 2, 1, 1), np.float32)
    b[0, 0] = 200.0
    ref = er.render([a, b], [0, 0], (1, 1))
    assert ref['labels'][0, 0, 0] == 0 and ref['conf'][0, 0, 0] == 0.75
    for K in ec.EQUAL_K:
        for V in ec.EQUAL_V:
            ref = er.render([np.full((1, K, 2, 2), 1.5, np.float32)] * V, [v % 2 for v in range(V)], (2, 2))
            assert not ref['labels'].any() and np.allclose(ref['conf'], 1.0 / K, rtol=0, atol=1e-16)
