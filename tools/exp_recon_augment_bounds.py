#!/usr/bin/env python3
"""Where the bounds of the K27 tests come from (CPU only, no GPU, seconds):

  contrast_fp32_vs_f64    max |torch fp32 on the CPU - float64 restatement| of the contrast and combined rows of
                          tests/recon_augment_cases.py, per shape (the reference's own ops: _io.adjust_brightness / adjust_contrast /
                          torch.flip on the fp32 image).  tests/test_hip_recon_augment.py allows the kernel four times the largest.
  normal_fp32_vs_f64      max |Box-Muller in NumPy fp32 - in float64| on the Philox integers of the noise row, per shape; the
                          noise parity bound is four times it, times 0.05.
  oracle_fp32_vs_f64_share  share of grey levels that differ between the CPU oracle's E2VID + PostProcessor in torch fp32 and in
                          float64 on the batches of tests/online_recon_cases.py (and the largest difference, in grey levels).
                          tests/test_hip_online_recon.py allows the fp32 GPU path four times it.

    python tools/exp_recon_augment_bounds.py        -> one JSON line; the values are recorded in DESIGN.md K27
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from openess_amd.datasets import _io                      # noqa: E402
from tests import online_recon_cases as oc                # noqa: E402
from tests import recon_augment_cases as cases            # noqa: E402
from tests import recon_augment_reference as ref          # noqa: E402


def torch_fp32(u8, c):
    """sequence_ov.py:204-221 on the fp32 image, noise excluded: fp32 [B, 3, H, W]."""
    out = []
    for b in range(u8.shape[0]):
        x = torch.from_numpy((u8[b] / 255).astype(np.float32))[None].repeat(3, 1, 1)
        if c['flip'][b]:
            x = torch.flip(x, [2])
        if c['brightness'][b] != 1.0:
            x = _io.adjust_brightness(x, float(np.float32(c['brightness'][b])))
        if c['contrast'][b] != 1.0:
            x = _io.adjust_contrast(x, float(np.float32(c['contrast'][b])))
        out.append(x.numpy())
    return np.stack(out)


def main():
    res = {'contrast_fp32_vs_f64': {}, 'normal_fp32_vs_f64': {}, 'oracle_fp32_vs_f64_share': {}, 'oracle_fp32_vs_f64_max_levels': {}}
    for shape in cases.SHAPES:
        u8 = cases.grey(shape)
        worst = 0.0
        for name, c in cases.CONTRAST_CASES.items():
            want = ref.augment(u8, c['flip'], c['brightness'], c['contrast'], c['noise_seed'])
            worst = max(worst, float(np.abs(torch_fp32(u8, c).astype(np.float64) - want).max()))
        res['contrast_fp32_vs_f64']['%dx%d' % shape] = worst
        n = 3 * shape[0] * shape[1]
        d = 0.0
        for seed in cases.NOISE_CASE['noise_seed']:
            words = ref.noise_words(seed, n)
            d = max(d, float(np.abs(ref.normals_from_words(words, np.float32).astype(np.float64) - ref.normals_from_words(words)).max()))
        res['normal_fp32_vs_f64']['%dx%d' % shape] = d
    model = oc.oracle_model(oc.filled_state_dict())
    for hw in oc.SIZES:
        batch, ds = oc.host_batch(hw)
        vox = oc.oracle_voxels(batch[2], ds)
        a = oc.post_cpu(oc.oracle_image(vox, model, hw, torch.float32)).numpy().astype(np.int64)
        b = oc.post_cpu(oc.oracle_image(vox, model, hw, torch.float64)).numpy().astype(np.int64)
        res['oracle_fp32_vs_f64_share']['%dx%d' % hw] = float((a != b).mean())
        res['oracle_fp32_vs_f64_max_levels']['%dx%d' % hw] = int(np.abs(a - b).max())
    print(json.dumps(res))


if __name__ == '__main__':
    main()
