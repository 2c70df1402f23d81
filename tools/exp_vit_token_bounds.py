#!/usr/bin/env python3
"""CPU measurement behind the bounds of the ViT token kernels' tests (tests/test_hip_vit_tokens.py): the fp32 models of the
kernels' rounding points (tests/vit_token_cases.py: attention_model, layer_norm_model) against the float64 references, in the
error measures of that module, on exactly the cases the GPU tests run:

  attention:  every family of ATT_BOUNDED_FAMILIES at every L of ATT_BOUNDED_L,
              err = |o - ref64| / (sum_j p_j |v_j| + |ref64|);
  layernorm:  every case of LN_CASES x LN_ROWS x LN_FAMILIES on the route it takes, and the two grid-stride cases,
              err = |y - ref64| / (2^-9 |ref64| + 2^-18 kappa_r |gamma_c| + 2^-20 |ref64 - beta_c|).

The bound of a quantity is four times its largest figure (the rule of K16 - K22).  The kernels' own outputs never enter.  No GPU.
    python tools/exp_vit_token_bounds.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import vit_token_cases as vc  # noqa: E402


def attention_figures():
    fig = {}
    for family in vc.ATT_BOUNDED_FAMILIES:
        worst = 0.0
        for L in vc.ATT_BOUNDED_L:
            c = vc.bounded_case(family, L)
            e = vc.attention_err(vc.attention_model(c["qkv"], c["B"], c["L"], c["heads"]), c["qkv"], c["B"], c["L"], c["heads"])
            print(f"attention {family} B={c['B']} L={c['L']} heads={c['heads']}: err {e:.3e}", flush=True)
            worst = max(worst, e)
        fig[family] = worst
    return fig


def layernorm_figures():
    fig = {f: 0.0 for f in vc.LN_FAMILIES}
    for (C, layout, route) in vc.LN_CASES:
        for rows in vc.LN_ROWS:
            for family in vc.LN_FAMILIES:
                x, g, b = vc.layernorm_inputs(C, rows, family)
                e = vc.layernorm_err(vc.layer_norm_model(x, g, b, vc.LN_EPS, route), x, g, b)
                fig[family] = max(fig[family], e)
        print(f"layernorm C={C} {layout} ({route}): " + " ".join(f"{k} {v:.3f}" for k, v in fig.items()) + " (running largest)",
              flush=True)
    for (C, layout, route) in vc.LN_GRID_CASES:
        x, g, b = vc.layernorm_inputs(C, vc.LN_GRID_ROWS, "randn")
        e = vc.layernorm_err(vc.layer_norm_model(x, g, b, vc.LN_EPS, route), x, g, b)
        print(f"layernorm C={C} rows={vc.LN_GRID_ROWS} ({route}): randn {e:.3f}", flush=True)
        fig["randn"] = max(fig["randn"], e)
    return fig


def main():
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    fig = {"attention": attention_figures(), "layernorm": layernorm_figures()}
    largest = {k: max(v.values()) for k, v in fig.items()}
    print(json.dumps({"largest": fig, "figure": largest, "bound": {k: 4.0 * v for k, v in largest.items()},
                      "in_cases_module": {"attention": vc.ATT_BOUND, "layernorm": vc.LN_BOUND}}))


if __name__ == "__main__":
    main()
