"""NumPy float32 restatement of the contract of oess_argmax_labels (include/oess.h) and the shared cases of its
tests.  Every operation below is one float32 operation with one rounding, in the kernel's order, and the kernel is compiled
without FMA contraction: the restatement is exact, GPU results are compared with array_equal.

  index rule   ATen's area_pixel_compute_source_index in float32 (csrc/bilinear_axis.h):
                 scale = align ? (in - 1) / (out - 1) (0 when out == 1) : in / out
                 src   = align ? scale * dst : max(scale * (dst + 0.5) - 0.5, 0)
                 i0 = min((int)src, in - 1), i1 = i0 + 1 if i0 < in - 1 else i0, lam = src - i0
  taps         bf16 logits are widened to float32 first (the caller passes float32 here)
  blend        hy * (hx * p00 + wx * p01) + wy * (hx * p10 + wx * p11), hx = 1 - wx, hy = 1 - wy, in that association
  same size    (H, W) == (h, w): no blend at all, the raw values are compared
  argmax       torch.argmax's rule: first index among equal maxima; NaN above everything; the first NaN wins
Nothing here needs a GPU."""
import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32

# (B, K, h, w), (H, W) or None = same size, align_corners
SHAPES = [((1, 1, 1, 1), (1, 1), False),
          ((1, 2, 1, 1), (3, 5), False),
          ((2, 3, 2, 3), None, False),
          ((1, 11, 3, 4), (7, 9), False),
          ((2, 19, 7, 9), (112, 144), False),
          ((2, 11, 5, 6), (13, 17), True),
          ((2, 4, 9, 8), (4, 3), False),          # downsampling
          ((1, 256, 2, 2), (4, 4), False)]
# two source rows of 25 x 256 fp32 = 51 200 bytes: above the kernel's 48 KB LDS budget, the taps come from global memory
GLOBAL_PATH_SHAPE = ((1, 256, 2, 25), (3, 40), False)
# the near-tie cap: shapes and seed whose share of near-ties was checked against torch's own float32 interpolation
CAP_CASES = [((2, 11, 7, 9), (77, 99), False),
             ((2, 19, 7, 9), (112, 144), False),
             ((1, 11, 28, 40), (440, 640), False),
             ((2, 11, 5, 6), (13, 17), True)]
# integer logits, power-of-two upsampling: every product and sum of the blend is exact in float32
# (7.1 %, 7.3 % and 7.0 % of their pixels are exact ties between the two largest classes: test_argmax_labels_reference.py)
EXACT_CASES = [((2, 11, 6, 7), 2), ((2, 11, 5, 4), 4), ((2, 19, 5, 4), 8)]


def case_id(shape, size, align):
    return "x".join(map(str, shape)) + "-" + ("same" if size is None else f"{size[0]}x{size[1]}") + ("-ac" if align else "")


def randn_logits(shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def exact_logits(shape, seed=0):
    """integers in -4 ... 4"""
    return torch.randint(-4, 5, shape, generator=torch.Generator().manual_seed(seed)).float()


def special_logits():
    """[2, 5, 4, 6] randn with ties, NaN and +-inf planted, and the labels the rule gives at the planted pixels {(b, y, x): label}"""
    x = randn_logits((2, 5, 4, 6), seed=1)
    x[0, 1, 0, 0] = x[0, 3, 0, 0] = 9.0                                   # a tie: the first index wins
    x[0, 2, 1, 1] = float('nan')
    x[0, 4, 1, 1] = float('nan')                                          # two NaN: the first wins
    x[1, 0, 2, 2] = float('inf')
    x[1, 3, 2, 2] = float('nan')                                          # NaN above +inf
    x[1, :, 3, 3] = float('-inf')                                         # all equal: label 0
    x[1, 2, 0, 5] = float('inf')                                          # a blend would turn this into 0 * inf = NaN at its neighbours
    return x, {(0, 0, 0): 1, (0, 1, 1): 2, (1, 2, 2): 3, (1, 3, 3): 0, (1, 0, 5): 2}


def src_index(n_in, n_out, align):
    dst = np.arange(n_out, dtype=f32)
    if align:
        scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
        s = scale * dst
    else:
        scale = f32(n_in) / f32(n_out)
        s = np.maximum(scale * (dst + f32(0.5)) - f32(0.5), f32(0))
    i0 = np.minimum(s.astype(np.int32), n_in - 1)
    i1 = np.where(i0 < n_in - 1, i0 + 1, i0)
    lam = s - i0.astype(f32)
    assert s.dtype == f32 and lam.dtype == f32
    return i0, i1, lam


def upsampled(x, size, align):
    """float32 [B, K, H, W]: the blend of the contract on float32 x [B, K, h, w]"""
    x = np.asarray(x)
    assert x.dtype == f32 and x.ndim == 4
    y0, y1, wy = src_index(x.shape[2], size[0], align)
    x0, x1, wx = src_index(x.shape[3], size[1], align)
    hy, hx = (f32(1) - wy)[:, None], (f32(1) - wx)[None, :]
    wy, wx = wy[:, None], wx[None, :]
    top, bot = x[:, :, y0], x[:, :, y1]
    with np.errstate(invalid='ignore', over='ignore'):
        v = hy * (hx * top[..., x0] + wx * top[..., x1]) + wy * (hx * bot[..., x0] + wx * bot[..., x1])
    assert v.dtype == f32
    return v


def first_argmax(v):
    """int64 [B, H, W] of [B, K, H, W] under torch.argmax's rule, one class at a time as the kernel walks them"""
    best = v[:, 0].copy()
    idx = np.zeros(best.shape, np.int64)
    with np.errstate(invalid='ignore'):
        for k in range(1, v.shape[1]):
            take = (v[:, k] > best) | (np.isnan(v[:, k]) & ~np.isnan(best))
            best = np.where(take, v[:, k], best)
            idx[take] = k
    return idx


def argmax_labels(x, size=None, align=False):
    """the contract: labels of float32 logits x [B, K, h, w] at `size` (None or the input size: the raw values)"""
    x = np.ascontiguousarray(np.asarray(x, dtype=f32))
    if size is None or tuple(size) == x.shape[2:]:
        return first_argmax(x)
    return first_argmax(upsampled(x, size, align))


def float64_upsampled(x, size, align):
    """float64 [B, K, H, W] of torch's own bilinear interpolation in float64"""
    return F.interpolate(torch.as_tensor(np.asarray(x)).double(), size=tuple(size), mode='bilinear', align_corners=align).numpy()


def top2_margin(v):
    """(margin between the two largest of K values, max_k |value|) per pixel of [B, K, H, W]; margin = inf when K == 1"""
    if v.shape[1] == 1:
        return np.full(v[:, 0].shape, np.inf), np.abs(v).max(1)
    s = np.sort(v, axis=1)
    return s[:, -1] - s[:, -2], np.abs(v).max(1)
