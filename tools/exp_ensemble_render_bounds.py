#!/usr/bin/env python3
"""CPU measurement behind the confidence bound of oess_segment_render_ensemble's tests (tests/test_hip_ensemble_render.py,
DESIGN.md K39): torch's own float32 softmax over the classes -> mean over the views -> max, against the same three operations in
float64, both started from the restatement's float32 class values (tests/ensemble_render_reference.py), on exactly the cases,
dtypes and inputs the GPU test runs (tests/ensemble_render_cases.py: CASES x DTYPES, logits()).  The figure is the largest
absolute difference of the two confidences; the test's bound is four times it.  Also prints, per case, the share of pixels whose
float64 top-two gap lies within twice that bound (their labels are checked by value).  The kernel's own outputs never enter.  No GPU.
    python tools/exp_ensemble_render_bounds.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ensemble_render_cases as ec  # noqa: E402
from tests import ensemble_render_reference as er  # noqa: E402


def main():
    figure, where = ec.measure_conf_figure(lambda case, d: print(f"conf {d:.3e} {case}", flush=True))
    bound = 4.0 * figure
    worst_share = 0.0
    for bk, views, size, align in ec.CASES:
        for dtype in ec.DTYPES:
            ref = er.render([x.numpy() for x in ec.logits(bk, views, dtype)], ec.flips_of(views), ec.out_size(views, size), align)
            share = float(er.weak_pixels(ref['p'], bound).mean())
            worst_share = max(worst_share, share)
            print(f"weak {share:.5f} {ec.case_id(bk, views, size, align)}-{dtype}", flush=True)
    print(json.dumps({"figure": {"conf": repr(figure)}, "at": {"conf": where}, "bound": {"conf": bound},
                      "weak_share": {"worst": worst_share, "cap": ec.WEAK_SHARE_CAP},
                      "in_cases_module": {"ENSEMBLE_CONF_FIGURE": ec.ENSEMBLE_CONF_FIGURE,
                                          "ENSEMBLE_CONF_BOUND": ec.ENSEMBLE_CONF_BOUND}}))


if __name__ == "__main__":
    main()
