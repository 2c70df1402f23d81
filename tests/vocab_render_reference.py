"""NumPy restatement of the contracts of oess_segment_render_grouped and oess_head_render (include/oess.h).

  grouped   name values: the float32 values of tests/segment_render_reference.py (raw at the input size, otherwise the blend in the
            kernel's association): exact.  Class value = the largest member, NaN when a member is NaN (torch.amax): exact.
            Label = first_argmax over the class values (torch.argmax's rule): exact.  Confidence = 1 / sum_k exp(c_k - c_max) in
            float64 FROM the float32 class values; the kernel's float32 walk is held to it within vocab_render_cases.CONF_BOUND.
  head      name values in float64: bias_p + sum_c w[p][c] * x[c] from the float32 operands (bf16 taps already widened); the
            kernel's float32 fmaf chain is held to it within VALUE_BOUND times the scale |bias_p| + sum_c |w[p][c] x[c]|.  Class
            values, labels and confidence from these in float64.
Nothing here needs a GPU."""
import numpy as np

from tests import argmax_labels_reference as ar
from tests import segment_render_reference as sr


def group_amax(v, offsets):
    """[B, K, H, W] of name values v [B, P, H, W]: per class the largest member; a NaN member makes the class value NaN"""
    with np.errstate(invalid='ignore'):
        return np.stack([np.maximum.reduce(v[:, a:b], axis=1) for a, b in zip(offsets[:-1], offsets[1:])], axis=1)


def confidence64(c):
    """float64 [B, H, W]: softmax probability of the largest of the class values c [B, K, H, W] (any float dtype), in float64"""
    c = np.asarray(c).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return 1.0 / np.exp(c - c.max(axis=1, keepdims=True)).sum(axis=1)


def grouped_render(x, offsets, size=None, align=False, palette=None, grey=None, alpha256=128, min_conf=0.0, ignore=255):
    """the grouped contract on float32 logits x [B, P, h, w]: dict(values float32 [B, P, H, W], classes float32 [B, K, H, W],
    argmax int64, conf float64, labels uint8, rgb uint8 | None)"""
    v = sr.values(x, size, align)
    c = group_amax(v, offsets)
    assert c.dtype == np.float32
    idx = ar.first_argmax(c)
    conf = confidence64(c)
    labels = sr.threshold(idx, conf, min_conf, ignore)
    rgb = None if palette is None else sr.colour(labels, palette, grey, alpha256, ignore)
    return dict(values=v, classes=c, argmax=idx, conf=conf, labels=labels, rgb=rgb)


def head_values64(x, weight, bias=None):
    """(float64 name values [B, P, H, W], float64 scale [B, P, H, W] = |bias_p| + sum_c |w[p][c] x[c]|) of float32 x [B, C, H, W],
    weight [P, C], bias [P] | None"""
    x, w = np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(weight, dtype=np.float32).astype(np.float64)
    b = np.zeros(w.shape[0]) if bias is None else np.asarray(bias, dtype=np.float32).astype(np.float64)
    v = np.einsum('pc,bchw->bphw', w, x) + b[None, :, None, None]
    scale = np.einsum('pc,bchw->bphw', np.abs(w), np.abs(x)) + np.abs(b)[None, :, None, None]
    return v, scale


def head_render(x, weight, bias, offsets):
    """the head contract in float64: dict(values, scale float64 [B, P, H, W], classes float64 [B, K, H, W], argmax int64, conf
    float64, margin float64 [B, H, W] between the two largest class values (inf when K == 1))"""
    v, scale = head_values64(x, weight, bias)
    c = group_amax(v, offsets)
    return dict(values=v, scale=scale, classes=c, argmax=ar.first_argmax(c), conf=confidence64(c), margin=ar.top2_margin(c)[0])
