"""Inputs of the SLIC tests (K24): seeded uint8 images scaled by 1 / 255, B = 2, on the smallest shapes that reach every branch of
the kernels, and their float64 references (computed once per process and shared; callers must not modify them)."""
import functools

import numpy as np
from scipy import ndimage

from tests import slic_reference as ref

B = 2
SIGMA, COMPACTNESS = 3.0, 6.0
# (H, W, n_segments): K = 8 | odd extents, K = 4 | K = 256: the LDS and index bounds, step 4 | K = 96, several workgroups per sample
SHAPES = [(40, 56, 12), (37, 53, 6), (64, 64, 256), (110, 160, 100)]
EXPECTED_K = {(40, 56, 12): 8, (37, 53, 6): 4, (64, 64, 256): 256, (110, 160, 100): 96}
KINDS = ['blobs', 'noise', 'checker']
CASES = [(kind, *shape) for shape in SHAPES for kind in KINDS]
ITERS = (1, 2, 10)


def case_id(case):
    return "{}-{}x{}-n{}".format(*case)


def _stretch(x):
    lo, hi = x.min(), x.max()
    return np.round((x - lo) / (hi - lo) * 255.0)


def frames_u8(kind, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == 'noise':
        img = rng.integers(0, 256, (B, 3, H, W))
    elif kind == 'blobs':
        img = np.stack([[_stretch(ndimage.gaussian_filter(rng.standard_normal((H, W)), 4.0)) for _ in range(3)] for _ in range(B)])
    elif kind == 'checker':
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        board = ((yy // 12 + xx // 16) % 2) * 120.0
        img = np.stack([np.stack([board + 100.0 * yy / H + 10 * b, 255.0 - board - 90.0 * xx / W, board * 0.5 + 60.0 * (yy + xx) / (H + W)])
                        for b in range(B)])
        img = np.clip(np.round(img + rng.integers(0, 4, img.shape)), 0, 255)
    else:
        raise ValueError(kind)
    return img.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def frames(kind, H, W, n):
    """float32 [B, 3, H, W] in [0, 1]."""
    seed = 1205 + 1000 * KINDS.index(kind) + H * 7 + W
    x = frames_u8(kind, H, W, seed).astype(np.float32) * np.float32(1.0 / 255.0)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(kind, H, W, n):
    """The float64 run: {'lab', 'lattice', 'labels': {iters: labels}, 'centers': {iters: centres}} with iters 0 = the start."""
    x = frames(kind, H, W, n)
    ny, nx, step = ref.lattice(H, W, n)
    lab = ref.lab_map(x, SIGMA, COMPACTNESS)
    centers = ref.initial_centers(lab, ny, nx)
    labels = ref.initial_labels(B, H, W, ny, nx)
    out = {'lab': lab, 'lattice': (ny, nx, step), 'labels': {0: labels}, 'centers': {0: centers}}
    for it in range(1, max(ITERS) + 1):
        labels = ref.assign(lab, centers, labels, step)
        centers, _ = ref.update(lab, labels, centers)
        out['labels'][it], out['centers'][it] = labels, centers
    return out
