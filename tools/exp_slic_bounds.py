"""CPU-only experiment behind the bounds of tests/test_hip_slic.py: the SLIC algorithm in numpy fp32 (separable
fp32 blur with fp32 taps, fp32 Lab, fp32 distances and means) against the float64 reference of tests/slic_reference.py on the
cases of tests/slic_cases.py and on 200 x 346 with n = 25.  Prints, per case: max|lab32 - lab64|, the colour error of one update
from the reference's labels, the share of pixels one assignment leaves out of the margin test, the share on which an fp32
assignment from the reference's centres disagrees inside the margin, and the label disagreement after 1, 2 and 10 rounds.
The tests' two float bounds are four times the largest of the first two columns."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import slic_cases as sc            # noqa: E402
from tests import slic_reference as ref       # noqa: E402

MARGIN = 1e-3


def blur32(frames, sigma):
    f = np.float32
    R = int(4.0 * sigma + 0.5)
    k = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-0.5 * k * k / (sigma * sigma))
    w = (w / w.sum()).astype(f)
    x = np.asarray(frames, dtype=f)
    for axis in (2, 3):
        pad = [(0, 0)] * 4
        pad[axis] = (R, R)
        p = np.pad(x, pad, mode='symmetric')
        acc = np.zeros_like(x)
        n = x.shape[axis]
        for i in range(2 * R + 1):
            sl = [slice(None)] * 4
            sl[axis] = slice(i, i + n)
            acc = (acc + w[i] * p[tuple(sl)]).astype(f)
        x = acc
    return x


def lab32(frames, sigma, compactness):
    return (ref.rgb_to_lab(blur32(frames, sigma), np.float32) * np.float32(1.0 / compactness)).astype(np.float32)


def update32(lab, labels, centers):
    """fp32 means as sequential fp32 sums would give them at best: float64 sums of fp32 values, one rounding."""
    new, _ = ref.update(lab.astype(np.float32), labels, centers.astype(np.float32))
    return new.astype(np.float32)


def main():
    cases = list(sc.CASES) + [(k, 200, 346, 25) for k in sc.KINDS]
    worst_lab = worst_col = 0.0
    print(f"{'case':28s} {'lab':>9s} {'colour':>9s} {'left out':>9s} {'assign':>9s} " + " ".join(f"{'it' + str(i):>8s}" for i in sc.ITERS))
    for case in cases:
        kind, H, W, n = case
        x = sc.frames(*case)
        ny, nx, step = ref.lattice(H, W, n)
        l64 = ref.lab_map(x, sc.SIGMA, sc.COMPACTNESS)
        l32 = lab32(x, sc.SIGMA, sc.COMPACTNESS)
        e_lab = float(np.abs(l32.astype(np.float64) - l64).max())
        c0 = ref.initial_centers(l64, ny, nx)
        p0 = ref.initial_labels(sc.B, H, W, ny, nx)
        a64, best, second = ref.assign(l64, c0, p0, step, with_margin=True)
        c1, _ = ref.update(l64, a64, c0)
        e_col = float(np.abs(update32(l64, a64, c0).astype(np.float64)[..., 2:] - c1[..., 2:]).max())
        keep = (second - best) > MARGIN * best
        a32 = ref.assign(l64.astype(np.float32), c0.astype(np.float32), p0, step)
        left = 1.0 - keep.mean()
        bad = float(((a32 != a64) & keep).mean())
        shares = []
        for it in sc.ITERS:
            g64, _ = ref.slic(x, n, sc.COMPACTNESS, sc.SIGMA, it, lab=l64)
            g32, _ = ref.slic(x, n, sc.COMPACTNESS, sc.SIGMA, it, lab=l32)
            shares.append(float((g64 != g32).mean()))
        worst_lab, worst_col = max(worst_lab, e_lab), max(worst_col, e_col)
        print(f"{sc.case_id(case):28s} {e_lab:9.2e} {e_col:9.2e} {left:9.2e} {bad:9.2e} " + " ".join(f"{s:8.2e}" for s in shares))
    print(f"max|lab32 - lab64| = {worst_lab:.3e}  -> bound {4 * worst_lab:.3e}")
    print(f"max colour error   = {worst_col:.3e}  -> bound {4 * worst_col:.3e}")


if __name__ == "__main__":
    main()
