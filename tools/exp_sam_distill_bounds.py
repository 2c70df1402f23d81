"""Where the bounds of tests/test_hip_sam_distill.py come from (CPU only): torch's float32 against float64 on the kernel test cases
of tests/sam_distill_reference.py, i.e. what one correct fp32 implementation of the five reference lines loses.  The test bounds
are four times the worst figure of each column, the project's convention:

    python tools/exp_sam_distill_bounds.py

loss: |loss32 - loss64|;  grad: max|g32 - g64| / max|g64|.  The bf16 rows run both precisions on the bf16-rounded student map."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import sam_distill_reference as sr  # noqa: E402


def main():
    torch.set_num_threads(1)                    # one summation order
    for bf16 in (False, True):
        worst, rows = sr.fp32_figures(bf16)
        for i, align, el, eg in rows:
            print(f"{'bf16' if bf16 else 'fp32'} map  case {i} {sr.CASES[i]} align={int(align)}: loss {el:.3e}  grad {eg:.3e}  "
                  f"(min norm {sr.case(i, bf16, align)['min_norm']:.3e})")
        print(f"{'bf16' if bf16 else 'fp32'} map  worst: loss {worst[0]:.3e}  grad {worst[1]:.3e}   -> bounds x4: "
              f"loss {4 * worst[0]:.3e}  grad {4 * worst[1]:.3e}")


if __name__ == '__main__':
    main()
