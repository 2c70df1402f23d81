"""Inputs of the SLIC connectivity tests (K24): int64 label maps [2, H, W], two DIFFERENT maps per case so that a leak between
samples shows, with their thresholds and, where one can be written down by hand, the expected result.

(a) the float64 SLIC labels of tests/slic_cases.py after 1 and after 10 rounds (12 cases x 2 = 24 cases, 48 maps), thresholds
    from the sizes rule;
(b) hand-made maps on 37 x 53 (odd extents, edge tiles) and 64 x 64, `max_size` above the whole map;
(c) one 64 x 64 case with components of `max_size` pixels and more (K = 16), to be compared with the loop run WITHOUT the cut.

References are computed once per process and shared; callers must not modify them."""
import collections
import functools

import numpy as np

from tests import slic_cases as sc
from tests import slic_connectivity_reference as cref

Case = collections.namedtuple("Case", "name maps min_size max_size bound expected")
A_ITERS = (1, 10)


def sizes(H, W, K):
    """skimage's thresholds, restated: (min_size, max_size, bound) -- what hip.slic_connectivity_sizes must return."""
    segment = H * W / K
    min_size = int(0.5 * segment)
    return min_size, int(3 * segment), H * W // max(min_size, 1)


def _ro(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    a.setflags(write=False)
    return a


def _hand(name, maps, min_size, expected=None):
    maps = _ro(maps)
    _, H, W = maps.shape
    return Case(name, maps, min_size, H * W + 1, H * W // max(min_size, 1), None if expected is None else _ro(expected))


def _serpentine(n):
    """Label 1 on a one-pixel-wide path through label 0: the odd rows, joined alternately at the right and the left end."""
    m = np.zeros((n, n), np.int64)
    for i, y in enumerate(range(1, n - 1, 2)):
        m[y, 1:n - 1] = 1
        if y + 2 < n - 1:
            m[y + 1, n - 2 if i % 2 == 0 else 1] = 1
    return m


@functools.lru_cache(maxsize=None)
def hand_made():
    H, W = 37, 53
    N = H * W
    rng = np.random.default_rng(2405)
    out = []
    # many small components that chain into each other
    for h, w in ((H, W), (64, 64)):
        out.append(_hand(f"random4-{h}x{w}", rng.integers(0, 4, (2, h, w)), 40))
    out.append(_hand("one-label", np.stack([np.full((H, W), 7), np.full((H, W), -3)]), 40, np.zeros((2, H, W))))
    different = np.stack([np.arange(N)[::-1].reshape(H, W), rng.permutation(N).reshape(H, W)])
    raster = np.broadcast_to(np.arange(N).reshape(H, W), (2, H, W))
    out.append(_hand("all-different-min1", different, 1, raster))                    # a pure renumbering
    out.append(_hand("all-different-min5", different, 5, np.zeros((2, H, W))))        # everything small: all 0
    # long union chains across tiles; sample 1's path starts at pixel (0, 0), so the path is component 0 there
    s = _serpentine(64)
    s1 = s.copy()
    s1[0, 0] = s1[0, 1] = 1
    for m in (s, s1):                                                                 # two components: the path and the rest
        assert sorted(cref.components(m)[1].values()) == sorted([int((m == 0).sum()), int((m == 1).sum())])
    out.append(_hand("serpentine-64x64", np.stack([s, s1]), 40, np.stack([s, 1 - s1])))
    rows = np.arange(H)[:, None] * np.ones((1, W), np.int64)
    out.append(_hand("stripes", np.stack([rows % 2, rows % 3 + 5]), W, np.stack([rows, rows])))     # a row has exactly min_size pixels
    # a small component at pixel (0, 0): no donor -> 0, although both its neighbours end up labelled otherwise
    m0 = np.full((H, W), 10)
    m0[2:] = 11
    m0[0, 0] = m0[1, 0] = 2
    e0 = (m0 == 11).astype(np.int64)
    m1 = np.full((H, W), 10)
    m1[10:] = 11
    m1[2:, 0] = 11
    m1[0, 0] = m1[0, 1] = m1[1, 0] = 2
    out.append(_hand("corner-no-donor", np.stack([m0, m1]), 5, np.stack([e0, (m1 == 11).astype(np.int64)])))
    # first- and last-visited earlier neighbours differ: A (rank 0) above B | C (ranks 1, 2) above D (rank 3); the small component
    # lies in D's top row under the B | C seam.  Two pixels: D, D, B, then D, D, C -> C.  One pixel: D, D, D, B -> B.
    base = np.full((H, W), 10)
    base[10:20, :26] = 11
    base[10:20, 26:] = 12
    base[20:] = 13
    eb = base - 10
    m0, m1 = base.copy(), base.copy()
    m0[20, 25] = m0[20, 26] = 99
    m1[20, 25] = 99
    e0, e1 = eb.copy(), eb.copy()
    e0[20, 25] = e0[20, 26] = 2
    e1[20, 25] = 1
    out.append(_hand("last-seen", np.stack([m0, m1]), 5, np.stack([e0, e1])))
    # a small component whose only earlier neighbour is itself small: A rows 0-4 (rank 0), B rows 5-9 (rank 1), C rows 10+ (rank
    # 2); s1 = {(9, x), (9, x + 1), (10, x)} takes B, s2 = (10, x + 1) touches s1 above and left of it.  x = 0: C's root comes after
    # s2, so s1 is s2's only earlier neighbour; x = 30: C is earlier too and seen first, s1 is seen last.
    base = np.full((H, W), 10)
    base[5:10] = 11
    base[10:] = 12
    maps, exps = [], []
    for x in (0, 30):
        m, e = base.copy(), base - 10
        m[9, x] = m[9, x + 1] = m[10, x] = 50
        m[10, x + 1] = 51
        e[9, x] = e[9, x + 1] = e[10, x] = e[10, x + 1] = 1
        maps.append(m)
        exps.append(e)
    out.append(_hand("chain-of-two", np.stack(maps), 5, np.stack(exps)))
    # equality-only comparison: labels beyond 32 bits, and two labels that agree in their low 32 bits
    big = np.stack([rng.integers(0, 4, (H, W)) + (1 << 40), rng.integers(0, 2, (H, W)) * (1 << 32) + 5])
    out.append(_hand("labels-2^40", big, 40))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def slic_label_cases():
    """(a): Case per (kind, H, W, n, rounds), maps = the float64 reference labels of tests/slic_cases.py."""
    out = []
    for case in sc.CASES:
        _, H, W, n = case
        ny, nx, _ = sc.reference(*case)['lattice']
        min_size, max_size, bound = sizes(H, W, ny * nx)
        for it in A_ITERS:
            out.append(Case(f"{sc.case_id(case)}-it{it}", _ro(sc.reference(*case)['labels'][it]), min_size, max_size, bound, None))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oversize_case():
    """(c): 64 x 64 at K = 16 (min_size 128, max_size 768): quadrants of 1024 pixels and halves of 2048 with speckles in them."""
    min_size, max_size, bound = sizes(64, 64, 16)
    rng = np.random.default_rng(77)
    yy, xx = np.meshgrid(np.arange(64), np.arange(64), indexing='ij')
    quad = (yy // 32) * 2 + xx // 32
    half = xx // 32 + 4
    maps = np.stack([quad, half])
    speck = rng.random(maps.shape) < 0.03
    maps = np.where(speck, 9, maps)
    return Case("oversize-64x64", _ro(maps), min_size, max_size, bound, None)


A_NAMES = [f"{sc.case_id(c)}-it{it}" for c in sc.CASES for it in A_ITERS]
B_NAMES = ["random4-37x53", "random4-64x64", "one-label", "all-different-min1", "all-different-min5", "serpentine-64x64", "stripes",
           "corner-no-donor", "last-seen", "chain-of-two", "labels-2^40"]
C_NAME = "oversize-64x64"
ALL_NAMES = A_NAMES + B_NAMES + [C_NAME]


def get(name):
    if name == C_NAME:
        return oversize_case()
    for c in (hand_made() if name in B_NAMES else slic_label_cases()):
        if c.name == name:
            return c
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(labels int64 [2, H, W], counts [2]) of the sequential loop WITHOUT the cut: what the GPU pass must give.  Read-only."""
    c = get(name)
    res = [cref.enforce_sequential(m, c.min_size, None) for m in c.maps]
    return _ro(np.stack([r[0] for r in res])), tuple(r[1] for r in res)
