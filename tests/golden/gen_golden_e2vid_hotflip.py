#!/usr/bin/env python3
"""Golden vectors for EventPreprocessor's hot-pixel removal and flip, produced by RUNNING the reference's own
`EventPreprocessor.__init__` / `__call__` (e2vid/utils/inference_utils.py:56-87, imported from the reference tree with the path
and the stubs of gen_golden_e2vid_pre.py).  `np.int = int` is set before the import: the reference calls `np.int` (:61), which NumPy >= 1.24
no longer has.  Stored: the inputs (copies taken BEFORE the call: the reference zeroes its argument in place), the hot-pixel
rows as written to the file, and the outputs, for B = 2, 5 bins at 12 x 20 and 13 x 19 (H x W) and the combinations
hot only / flip only / both / both + no_normalize.  The rows include (0, 0), (W-1, H-1) and a duplicate.
Run:  python tests/golden/gen_golden_e2vid_hotflip.py"""
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden_e2vid_pre import _NoTimer, install_stubs  # noqa: E402

SIZES = [(12, 20), (13, 19)]                                  # (H, W)
COMBOS = {"hot": (True, False, False), "flip": (False, True, False), "both": (True, True, False),
          "both_nonorm": (True, True, True)}                  # (hot list, flip, no_normalize)


def hot_rows(H, W):
    """`x,y` rows: the two opposite corners, a duplicate, and interior / border pixels."""
    return np.array([[0, 0], [W - 1, H - 1], [3, 5], [3, 5], [W - 1, 0], [7, H - 2], [1, 1]], np.int64)


def main():
    np.int = int
    install_stubs()
    import e2vid.utils.inference_utils as iu
    iu.CudaTimer = _NoTimer
    torch.set_num_threads(4)
    rng = np.random.default_rng(3207)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for (H, W) in SIZES:
            tag = f"{H}x{W}"
            x = (rng.normal(0.2, 1.3, (2, 5, H, W)) * (rng.uniform(0, 1, (2, 5, H, W)) > 0.6)).astype(np.float32)
            rows = hot_rows(H, W)
            path = os.path.join(tmp, f"hot_{tag}.txt")
            np.savetxt(path, rows, fmt="%d", delimiter=",")
            out[f"in_{tag}"], out[f"rows_{tag}"] = x, rows
            for name, (hot, flip, nonorm) in COMBOS.items():
                pre = iu.EventPreprocessor(SimpleNamespace(no_normalize=nonorm, hot_pixels_file=path if hot else None, flip=flip))
                out[f"out_{tag}_{name}"] = pre(torch.from_numpy(x.copy())).numpy().copy()
    np.savez_compressed(os.path.join(HERE, "e2vid_hotflip.npz"), **out)
    print("wrote e2vid_hotflip.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
