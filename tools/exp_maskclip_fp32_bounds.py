"""CPU measurement behind the bounds of the fp32 MaskCLIP tests (tests/vit_f32_cases.py): fp32 on the CPU against
float64 on every test case.  The test bounds are four times these figures.  No GPU, no kernel of this project runs here.

    python tools/exp_maskclip_fp32_bounds.py [--skip-tower]

  attention : the fp32 model of the kernel's rounding points, per family and L
  LayerNorm : torch fp32 F.layer_norm, per family (largest over the cases and row counts); the model of the kernels' summation
              order and its one-pass mutation next to it
  GELU GEMM : the k-ordered fp32 chain and torch's fp32 matmul, largest over the shapes
  tower     : torch fp32 of oracle/maskclip.py against its float64 copy: logits and v_map as max|d| / max|ref|, the argmax
              agreement and the pixels the margin leaves out"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import vit_f32_cases as fc  # noqa: E402


def attention():
    out = {}
    for family in fc.ATT_BOUNDED_FAMILIES:
        worst = 0.0
        for L in fc.ATT_BOUNDED_L:
            c = fc.bounded_case(family, L)
            e = fc.attention_err(fc.attention_model_f32(c["qkv"], c["B"], L, c["heads"]), c["qkv"], c["B"], L, c["heads"])
            print(f"attention {family:11s} L={L:5d}: FIGURE (model) {e:.3e} (module {fc.ATT_FIGURES[family, L]:.3e})")
            worst = max(worst, e)
        out[family] = worst
        print(f"attention {family:11s} largest {worst:.3e}")
    return out


def layernorm():
    out = {}
    for family in fc.LN_FAMILIES:
        worst = {"torch": 0.0, "model": 0.0, "one_pass": 0.0}
        for C, layout, route in fc.LN_CASES:
            for rows in fc.LN_ROWS:
                x, g, b = fc.layernorm_inputs(C, rows, family)
                worst["torch"] = max(worst["torch"], fc.layernorm_err(fc.layernorm_torch_f32(x, g, b), x, g, b))
                worst["model"] = max(worst["model"], fc.layernorm_err(fc.layer_norm_model_f32(x, g, b, route=route), x, g, b))
                worst["one_pass"] = max(worst["one_pass"],
                                        fc.layernorm_err(fc.layer_norm_model_f32(x, g, b, route=route, one_pass=True), x, g, b))
        out[family] = worst["torch"]
        print(f"layernorm {family:18s} FIGURE (torch fp32) {worst['torch']:.3e} (module {fc.LN_FIGURES[family]:.3e}); "
              f"kernel model {worst['model']:.3e}; one-pass model {worst['one_pass']:.3e}")
    return out


def gelu():
    chain = mm = 0.0
    for rows, Cin, Cout in fc.linear_shapes():
        c = fc.linear_gelu_case(rows, Cin, Cout)
        for with_br in (False, True):
            chain = max(chain, fc.linear_gelu_err(fc.linear_chain_f32(c, with_br), c, with_br))
            v = c["x"] @ c["w"].T
            if with_br:
                v = v + c["b"] + c["r"]
            mm = max(mm, fc.linear_gelu_err(torch.nn.functional.gelu(v), c, with_br))
    print(f"gelu gemm FIGURE (k-ordered fp32 chain) {chain:.3e} (module {fc.GELU_FIGURE:.3e}); torch fp32 matmul {mm:.3e}")
    return chain


def tower():
    for i, (img_size, hw, B) in enumerate(fc.TOWER_CASES):
        o, img, ref, v64 = fc.tower_reference(i)
        with torch.no_grad():
            out = o(img)
            _, v = o.encoder(img)
        bad, left = fc.argmax_check(out, ref)
        print(f"tower case {i + 1} img_size={img_size} image={hw} B={B}: logits FIGURE {fc.rel_max(out, ref):.3e} "
              f"(module {fc.TOWER_LOGIT_FIGURES[i]:.3e}); v_map FIGURE {fc.rel_max(v, v64):.3e} (module {fc.TOWER_VMAP_FIGURES[i]:.3e}); "
              f"argmax disagreements at the margin {bad}; left out {100 * left:.2f} %; "
              f"agreement on every pixel {100 * float((out.argmax(1) == ref.argmax(1)).double().mean()):.2f} %")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--skip-tower", action="store_true")
    ap.add_argument("--only", choices=("attention", "layernorm", "gelu", "tower"))
    a = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for name, fn in (("attention", attention), ("layernorm", layernorm), ("gelu", gelu), ("tower", tower)):
        if a.only and a.only != name:
            continue
        if name == "tower" and a.skip_tower:
            continue
        fn()


if __name__ == "__main__":
    main()
