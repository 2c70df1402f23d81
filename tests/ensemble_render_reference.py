"""NumPy restatement of the contract of oess_segment_render_ensemble (include/oess.h).

  values         per view the float32 class values of tests/segment_render_reference.py (raw at the output size, otherwise the
                 blend in the kernel's association), mirrored along W where the view's flip flag is set: exact
  probabilities  q_vk = softmax over k of view v, p_k = mean over the views, in float64 FROM those float32 values: the kernel's
                 float32 arithmetic is held to this within tests/ensemble_render_cases.py ENSEMBLE_CONF_BOUND
  label          first_argmax (torch.argmax's rule) over p; confidence = p_label
  threshold, colour   tests/segment_render_reference.py: exact given a label and a confidence
Nothing here needs a GPU."""
import numpy as np

from tests import argmax_labels_reference as ar
from tests import segment_render_reference as sr

f32 = np.float32


def view_values(xs, flips, size, align=False):
    """list of float32 [B, K, H, W]: every view's class values at `size`, mirrored per flag"""
    out = []
    for x, f in zip(xs, flips):
        v = sr.values(x, size, align)
        out.append(np.ascontiguousarray(v[..., ::-1]) if f else v)
    return out


def probabilities(vals):
    """float64 [B, K, H, W]: the mean over the views of the softmax of their float32 class values (NaN where torch gives NaN)"""
    p = 0.0
    with np.errstate(invalid='ignore', over='ignore'):
        for v in vals:
            assert v.dtype == f32
            v = v.astype(np.float64)
            e = np.exp(v - v.max(axis=1, keepdims=True))
            p = p + e / e.sum(axis=1, keepdims=True)
    return p / len(vals)


def render(xs, flips, size, align=False, palette=None, grey=None, alpha256=128, min_conf=0.0, ignore=255):
    """the whole contract on a list of float32 logits: dict(values, p float64, argmax int64, conf float64, labels u8, rgb u8 | None)"""
    vals = view_values(xs, flips, size, align)
    p = probabilities(vals)
    idx = ar.first_argmax(p)
    conf = np.take_along_axis(p, idx[:, None], axis=1)[:, 0]
    labels = sr.threshold(idx, conf, min_conf, ignore)
    rgb = None if palette is None else sr.colour(labels, palette, grey, alpha256, ignore)
    return dict(values=vals, p=p, argmax=idx, conf=conf, labels=labels, rgb=rgb)


def top2_gap(p):
    """float64 [B, H, W]: the gap between the two largest of p [B, K, H, W]; inf when K == 1"""
    if p.shape[1] == 1:
        return np.full(p[:, 0].shape, np.inf)
    s = np.sort(p, axis=1)
    return s[:, -1] - s[:, -2]


def weak_pixels(p, bound):
    """bool [B, H, W]: pixels whose float64 top-two gap does not exceed 2 x bound (their label is checked by value, not by index)"""
    return ~(top2_gap(p) > 2.0 * bound)


def check_labels(labels, p, bound):
    """The label rule of the tests: where the top-two gap of the float64 p exceeds 2 x bound the label is first_argmax(p);
    anywhere else it is a class whose p is within 2 x bound of the maximum.  No pixel goes unchecked.  Returns the weak share."""
    labels = np.asarray(labels).astype(np.int64)
    assert labels.min() >= 0 and labels.max() < p.shape[1]
    weak = weak_pixels(p, bound)
    want = ar.first_argmax(p)
    assert np.array_equal(labels[~weak], want[~weak]), "a label with a clear float64 margin differs from the restatement's"
    chosen = np.take_along_axis(p, labels[:, None], axis=1)[:, 0]
    assert (chosen[weak] >= p.max(axis=1)[weak] - 2.0 * bound).all(), "a near-tie label is not among the float64 near-maxima"
    return float(weak.mean())
