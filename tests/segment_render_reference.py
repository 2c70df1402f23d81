"""NumPy restatement of the contract of oess_segment_render (include/oess.h).

  values      the float32 class values of tests/argmax_labels_reference.py (raw at the input size, otherwise the blend in the
              kernel's association, one rounding per operation): exact
  label       that module's first_argmax (torch.argmax's rule): exact
  confidence  1 / sum_k exp(v_k - v_max) in float64 FROM the float32 values: the kernel's float32 walk is held to this within
              tests/segment_render_cases.py CONF_BOUND
  threshold   label = ignore where conf < min_conf (false for NaN): exact given a confidence
  colour      palette[label], black for ignore; over grey (a * c + (256 - a) * grey + 128) >> 8 in integers: exact
Nothing here needs a GPU."""
import numpy as np

from tests import argmax_labels_reference as ar

f32 = np.float32


def values(x, size=None, align=False):
    """float32 [B, K, H, W] class values of float32 logits x [B, K, h, w]"""
    x = np.ascontiguousarray(np.asarray(x, dtype=f32))
    if size is None or tuple(size) == x.shape[2:]:
        return x
    return ar.upsampled(x, size, align)


def confidence(v):
    """float64 [B, H, W]: softmax probability of the largest of the float32 values v [B, K, H, W]"""
    v = np.asarray(v)
    assert v.dtype == f32
    v = v.astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return 1.0 / np.exp(v - v.max(axis=1, keepdims=True)).sum(axis=1)


def threshold(labels, conf, min_conf, ignore=255):
    """uint8 labels with `ignore` where conf < min_conf (a NaN confidence keeps its label)"""
    with np.errstate(invalid='ignore'):
        return np.where(np.asarray(conf) < min_conf, ignore, labels).astype(np.uint8)


def colour(labels, palette, grey=None, alpha256=128, ignore=255):
    """uint8 [B, H, W, 3] of uint8 labels [B, H, W], palette [K, 3], optional grey [B, H, W]"""
    labels = np.asarray(labels).astype(np.int64)
    pal = np.concatenate([np.asarray(palette).astype(np.int64), np.zeros((1, 3), np.int64)])
    c = pal[np.where(labels == ignore, len(pal) - 1, np.minimum(labels, len(pal) - 1))]
    if grey is not None:
        c = (alpha256 * c + (256 - alpha256) * np.asarray(grey).astype(np.int64)[..., None] + 128) >> 8
    assert c.min() >= 0 and c.max() <= 255
    return c.astype(np.uint8)


def render(x, size=None, align=False, palette=None, grey=None, alpha256=128, min_conf=0.0, ignore=255):
    """the whole contract on float32 logits x: dict(values float32, argmax int64, conf float64, labels uint8, rgb uint8 | None)"""
    v = values(x, size, align)
    idx = ar.first_argmax(v)
    conf = confidence(v)
    labels = threshold(idx, conf, min_conf, ignore)
    rgb = None if palette is None else colour(labels, palette, grey, alpha256, ignore)
    return dict(values=v, argmax=idx, conf=conf, labels=labels, rgb=rgb)
