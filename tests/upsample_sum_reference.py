"""NumPy float64 restatement of the contract of oess_upsample_bilinear2x_sum_nhwc_bf16 (include/oess.h):

    out[b, oy, ox, c] = bilinear2x(x + skip)[b, oy, ox, c]

with bilinear2x = F.interpolate(scale_factor=2, mode='bilinear', align_corners=False): per axis the source coordinate of
output o is max(0, (o + 0.5) / 2 - 0.5), the taps are i0 = floor(src) and i1 = min(i0 + 1, n - 1), the weight of i1 is
lambda = src - i0.  Written from that sentence, not from the kernel.  tests/test_upsample_sum_reference.py pins it to torch on the
CPU; tests/test_hip_upsample_sum.py holds the kernel to it.  Nothing here needs a GPU."""
import numpy as np


def axis_taps(n):
    """(i0, i1, lambda) of the 2 n outputs of an axis of n inputs."""
    o = np.arange(2 * n, dtype=np.float64)
    src = np.maximum(0.0, (o + 0.5) / 2.0 - 0.5)
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    return i0, i1, src - i0


def upsample2x_sum(x, skip=None):
    """x, skip: [B, H, W, C] arrays (any float type, taken to float64) -> float64 [B, 2H, 2W, C]."""
    s = np.asarray(x, dtype=np.float64)
    if skip is not None:
        s = s + np.asarray(skip, dtype=np.float64)
    _, H, W, _ = s.shape
    y0, y1, ly = axis_taps(H)
    x0, x1, lx = axis_taps(W)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    rows = (1.0 - ly) * s[:, y0] + ly * s[:, y1]
    return (1.0 - lx) * rows[:, :, x0] + lx * rows[:, :, x1]


def tap_magnitude(x, skip=None):
    """A of the kernel's bound: per output element the largest |x| + |skip| among its taps, float64 [B, 2H, 2W, C].  A tap of
    weight zero (i1 at o = 0, where lambda is 0) contributes nothing to the output and is left out, which only tightens A."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    if skip is not None:
        a = a + np.abs(np.asarray(skip, dtype=np.float64))
    _, H, W, _ = a.shape
    y0, y1, ly = axis_taps(H)
    x0, x1, lx = axis_taps(W)
    y1, x1 = np.where(ly > 0, y1, y0), np.where(lx > 0, x1, x0)
    rows = np.maximum(a[:, y0], a[:, y1])
    return np.maximum(rows[:, :, x0], rows[:, :, x1])
