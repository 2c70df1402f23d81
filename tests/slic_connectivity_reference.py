"""numpy / pure-Python statements of SLIC's connectivity pass (K24; skimage's _enforce_label_connectivity_cython restated, so
that nothing here needs skimage): the sequential loop with the optional `max_size` cut, the order-free form the GPU builds, and
the size of a map's largest component.  One 2-D map of any integers at a time; labels are compared for equality only."""
import numpy as np


def _neighbours(c, W, H):
    """The in-bounds 4-neighbours of flat index c in the loop's order: right, left, down, up."""
    cy, cx = divmod(c, W)
    out = []
    if cx + 1 < W:
        out.append(c + 1)
    if cx > 0:
        out.append(c - 1)
    if cy + 1 < H:
        out.append(c + W)
    if cy > 0:
        out.append(c - W)
    return out


def enforce_sequential(seg, min_size, max_size=None):
    """The sequential loop.  max_size None: no cut (a component of any size stays whole).  Returns (labels int64 [H, W],
    the number of kept components = the label count)."""
    seg = np.asarray(seg)
    H, W = seg.shape
    s = seg.ravel().tolist()
    out = [-1] * (H * W)
    cur = 0
    for p in range(H * W):
        if out[p] >= 0:
            continue
        adjacent, lab = 0, s[p]
        out[p] = cur
        queue = [p]
        v = 0
        while v < len(queue) and (max_size is None or len(queue) < max_size):
            for n in _neighbours(queue[v], W, H):
                if s[n] == lab and out[n] == -1:
                    out[n] = cur
                    queue.append(n)
                    if max_size is not None and len(queue) >= max_size:
                        break
                elif out[n] >= 0 and out[n] != cur:
                    adjacent = out[n]
            v += 1
        if len(queue) < min_size:
            for q in queue:
                out[q] = adjacent                         # absorbed: cur is not advanced
        else:
            cur += 1
    return np.array(out, dtype=np.int64).reshape(H, W), cur


def components(seg):
    """(root [H W] list: the lowest raster index of every pixel's 4-connected equal-label component, {root: size} in raster
    order of the roots)."""
    seg = np.asarray(seg)
    H, W = seg.shape
    s = seg.ravel().tolist()
    root = [-1] * (H * W)
    sizes = {}
    for p in range(H * W):
        if root[p] >= 0:
            continue
        root[p] = p
        stack, n = [p], 0
        while stack:
            c = stack.pop()
            n += 1
            for m in _neighbours(c, W, H):
                if root[m] < 0 and s[m] == s[p]:
                    root[m] = p
                    stack.append(m)
        sizes[p] = n
    return root, sizes


def largest_component(seg):
    return max(components(seg)[1].values())


def enforce_order_free(seg, min_size):
    """The order-free form: kept components (size >= min_size) are ranked by root; a small component takes the final label of
    its donor, the last pixel its queue-order walk sees that lies in a component with a smaller root, or 0 without one."""
    seg = np.asarray(seg)
    H, W = seg.shape
    root, sizes = components(seg)
    final, rank = {}, 0
    for r, size in sizes.items():                         # increasing root: a donor's component is resolved before it is needed
        if size >= min_size:
            final[r] = rank
            rank += 1
            continue
        donor, seen, queue, v = None, {r}, [r], 0
        while v < len(queue):
            for m in _neighbours(queue[v], W, H):
                if root[m] == r:
                    if m not in seen:
                        seen.add(m)
                        queue.append(m)
                elif root[m] < r:
                    donor = root[m]
            v += 1
        final[r] = 0 if donor is None else final[donor]
    return np.array([final[r] for r in root], dtype=np.int64).reshape(H, W), rank
