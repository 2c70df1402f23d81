"""Float64 reference of hip.slic_superpixels (K24): the algorithm of the GPU kernels stated directly in numpy, with
scipy.ndimage.gaussian_filter for the blur.  It is skimage.segmentation.slic(img, n_segments, compactness, sigma, start_label=0,
enforce_connectivity=False) as far as its published steps go; bit parity with skimage itself is not pinned anywhere.

A centre is (y, x, L, a, b); centre k = i nx + j of the ny x nx lattice.  `dtype` is float64 everywhere it is used as the
reference; tools/exp_slic_bounds.py passes float32 (with its own fp32 blur) to measure what fp32 arithmetic alone costs."""
import math

import numpy as np
from scipy import ndimage


def lattice(H, W, n_segments):
    s = math.sqrt(H * W / n_segments)
    ny, nx = max(1, int(math.floor(H / s))), max(1, int(math.floor(W / s)))
    step = max(int(math.ceil(H / ny)), int(math.ceil(W / nx)))
    return ny, nx, step


def lattice_pixels(H, W, ny, nx):
    ys = [int(math.floor((i + 0.5) * H / ny)) for i in range(ny)]
    xs = [int(math.floor((j + 0.5) * W / nx)) for j in range(nx)]
    return ys, xs


def blur(frames, sigma):
    """frames [B, 3, H, W] -> float64, per channel a Gaussian of radius int(4 sigma + 0.5), border rule reflect."""
    x = np.asarray(frames, dtype=np.float64)
    return ndimage.gaussian_filter(x, sigma=(0, 0, sigma, sigma), mode='reflect', truncate=4.0)


def rgb_to_lab(rgb, dtype=np.float64):
    """rgb [B, 3, H, W] -> [B, H, W, 3], skimage's sRGB -> CIELAB (D65, 2 degrees); every constant in `dtype`."""
    t = dtype
    v = np.asarray(rgb, dtype=t)
    lin = np.where(v > t(0.04045), np.power((np.maximum(v, t(0)) + t(0.055)) / t(1.055), t(2.4)), v / t(12.92)).astype(t)
    r, g, b = lin[:, 0], lin[:, 1], lin[:, 2]
    X = (t(0.412453) * r + t(0.357580) * g + t(0.180423) * b) / t(0.95047)
    Y = t(0.212671) * r + t(0.715160) * g + t(0.072169) * b
    Z = (t(0.019334) * r + t(0.119193) * g + t(0.950227) * b) / t(1.08883)

    def f(u):
        return np.where(u > t(0.008856), np.cbrt(np.maximum(u, t(0))), t(7.787) * u + t(16.0) / t(116.0)).astype(t)
    fx, fy, fz = f(X), f(Y), f(Z)
    return np.stack([t(116.0) * fy - t(16.0), t(500.0) * (fx - fy), t(200.0) * (fy - fz)], axis=-1).astype(t)


def lab_map(frames, sigma=3.0, compactness=6.0):
    return rgb_to_lab(blur(frames, sigma)) * (1.0 / compactness)


def initial_centers(lab, ny, nx):
    B, H, W, _ = lab.shape
    ys, xs = lattice_pixels(H, W, ny, nx)
    c = np.zeros((B, ny * nx, 5), dtype=lab.dtype)
    for i, y in enumerate(ys):
        for j, x in enumerate(xs):
            c[:, i * nx + j, 0], c[:, i * nx + j, 1] = y, x
            c[:, i * nx + j, 2:] = lab[:, y, x]
    return c


def initial_labels(B, H, W, ny, nx):
    yy = (np.arange(H) * ny // H)[:, None]
    xx = (np.arange(W) * nx // W)[None, :]
    return np.broadcast_to(yy * nx + xx, (B, H, W)).astype(np.int64).copy()


def assign(lab, centers, prev, step, with_margin=False):
    """One assignment.  Returns labels, and with_margin the best and second-best distance of every pixel (inf where none)."""
    B, H, W, _ = lab.shape
    t = lab.dtype.type
    labels = prev.copy()
    best = np.full((B, H, W), np.inf, dtype=lab.dtype)
    second = np.full((B, H, W), np.inf, dtype=lab.dtype)
    yy = np.arange(H, dtype=lab.dtype)[:, None]
    xx = np.arange(W, dtype=lab.dtype)[None, :]
    inv = t(1.0) / (t(step) * t(step))
    for b in range(B):
        for k in range(centers.shape[1]):
            cy, cx = centers[b, k, 0], centers[b, k, 1]
            y0, y1 = int(max(cy - t(2 * step), t(0))), int(min(cy + t(2 * step) + t(1), t(H)))
            x0, x1 = int(max(cx - t(2 * step), t(0))), int(min(cx + t(2 * step) + t(1), t(W)))
            if y0 >= y1 or x0 >= x1:
                continue
            dy, dx = yy[y0:y1] - cy, xx[:, x0:x1] - cx
            dc = lab[b, y0:y1, x0:x1] - centers[b, k, 2:]
            d = (dy * dy + dx * dx) * inv + (dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1] + dc[..., 2] * dc[..., 2])
            bw, sw, lw = best[b, y0:y1, x0:x1], second[b, y0:y1, x0:x1], labels[b, y0:y1, x0:x1]
            win = d < bw                                     # strict: ties stay with the lowest k
            sw[...] = np.where(win, bw, np.minimum(sw, d))
            lw[win] = k
            bw[win] = d[win]
    return (labels, best, second) if with_margin else labels


def update(lab, labels, centers):
    """Means of (y, x, L, a, b) per centre, an empty centre stays; also returns the counts."""
    B, H, W, _ = lab.shape
    K = centers.shape[1]
    new = centers.copy()
    counts = np.zeros((B, K), dtype=np.int64)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    for b in range(B):
        l = labels[b].ravel()
        cnt = np.bincount(l, minlength=K)
        counts[b] = cnt
        has = cnt > 0
        comps = [yy.ravel(), xx.ravel()] + [lab[b, ..., c].ravel() for c in range(3)]
        for i, v in enumerate(comps):
            s = np.bincount(l, weights=v.astype(np.float64), minlength=K)
            new[b, has, i] = (s[has] / cnt[has]).astype(lab.dtype)
    return new, counts


def slic(frames, n_segments, compactness=6.0, sigma=3.0, iters=10, lab=None):
    """Labels int64 [B, H, W] and centres [B, K, 5] after exactly `iters` rounds.  lab: a map to start from (any float dtype)."""
    B, _, H, W = frames.shape
    ny, nx, step = lattice(H, W, n_segments)
    if lab is None:
        lab = lab_map(frames, sigma, compactness)
    centers = initial_centers(lab, ny, nx)
    labels = initial_labels(B, H, W, ny, nx)
    for _ in range(iters):
        labels = assign(lab, centers, labels, step)
        centers, _ = update(lab, labels, centers)
    return labels, centers
