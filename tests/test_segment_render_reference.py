"""The restatement of oess_segment_render's contract (tests/segment_render_reference.py) pinned without a GPU: (a) integer logits in
-4 ... 4 at power-of-two upsampling, where the float32 blend is exact: values and labels equal float64
F.interpolate(...).argmax(1); (b) its confidence against float64 softmax(...).max(1) of the float64 interpolation within the figure
tools/exp_segment_render_bounds.py prints (the restatement rounds only the blend to float32; torch's float32 path rounds the
softmax too); (c) the colour formula against a plain Python loop."""
import numpy as np
import pytest
import torch

from tests import argmax_labels_reference as ar
from tests import segment_render_cases as sc
from tests import segment_render_reference as sr


@pytest.mark.parametrize("shape,scale", ar.EXACT_CASES, ids=[f"{'x'.join(map(str, s))}-x{k}" for s, k in ar.EXACT_CASES])
def test_integer_logits_give_float64_values_and_labels(shape, scale):
    x = ar.exact_logits(shape)
    size = (shape[2] * scale, shape[3] * scale)
    out = sr.render(x.numpy(), size)
    v64 = torch.nn.functional.interpolate(x.double(), size=size, mode='bilinear', align_corners=False)
    assert np.array_equal(out['values'].astype(np.float64), v64.numpy())
    assert np.array_equal(out['argmax'], v64.argmax(1).numpy())
    assert out['labels'].dtype == np.uint8 and np.array_equal(out['labels'], v64.argmax(1).numpy())
    # exact values: the float64 confidence of the restatement IS the float64 softmax
    assert np.allclose(out['conf'], v64.softmax(1).max(1).values.numpy(), rtol=0, atol=1e-15)


def test_cases_module_holds_the_measured_figure():
    figure, where = sc.measure_conf_figure()
    print(f"torch float32 confidence against float64: {figure:.3e} at {where}")
    # torch's CPU kernels may vectorise differently on another host: the recorded figure has to be of the measured size
    assert 0.5 * sc.CONF_FIGURE <= figure <= 2.0 * sc.CONF_FIGURE and sc.CONF_BOUND == 4.0 * sc.CONF_FIGURE


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("shape,size,align", sc.ALL_SHAPES, ids=[sc.case_id(*c) for c in sc.ALL_SHAPES])
def test_confidence_equals_float64_softmax_within_the_figure(shape, size, align, dtype):
    x = sc.logits(shape, dtype)
    got = sr.render(x.numpy(), size, align)['conf']
    want = sc.torch_conf(x, size, align, torch.float64).numpy()
    d = float(np.abs(got - want).max())
    print(f"{sc.case_id(shape, size, align)}-{dtype}: restatement against float64 {d:.3e} (figure {sc.CONF_FIGURE:.3e})")
    assert got.dtype == np.float64 and d <= sc.CONF_FIGURE


def test_threshold_and_nan():
    labels = np.array([[[0, 1, 2, 3]]])
    conf = np.array([[[0.2, 0.5, np.nan, 0.49999]]])
    assert sr.threshold(labels, conf, 0.5).tolist() == [[[255, 1, 2, 255]]]
    assert sr.threshold(labels, conf, 0.0).tolist() == [[[0, 1, 2, 3]]]
    assert sr.threshold(labels, conf, 0.5, ignore=7).tolist() == [[[7, 1, 2, 7]]]


@pytest.mark.parametrize("alpha256", sc.ALPHAS256)
def test_colour_formula_against_a_plain_loop(alpha256):
    B, H, W, K = 2, 3, 4, 5
    pal = sc.palette(K).numpy()
    grey = sc.grey(B, H, W).numpy()
    labels = torch.randint(0, K, (B, H, W), generator=torch.Generator().manual_seed(3)).numpy().astype(np.uint8)
    labels[0, 0, 0], labels[1, 2, 3] = 255, 255
    plain = sr.colour(labels, pal)
    blended = sr.colour(labels, pal, grey, alpha256)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                c = [0, 0, 0] if labels[b, y, x] == 255 else [int(v) for v in pal[labels[b, y, x]]]
                assert plain[b, y, x].tolist() == c
                g = int(grey[b, y, x])
                assert blended[b, y, x].tolist() == [(alpha256 * ch + (256 - alpha256) * g + 128) >> 8 for ch in c]
    if alpha256 == 0:
        assert np.array_equal(blended, np.repeat(grey[..., None], 3, axis=3))
    if alpha256 == 256:
        assert np.array_equal(blended, plain)
