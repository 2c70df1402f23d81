"""CPU measurement behind the bounds of tests/test_hip_clip_text.py (K29): torch fp32 against the float64 restatement
(tests/clip_text_reference.py) on exactly the committed cases, as the largest absolute error over the largest output magnitude,
per kernel and for the tower.  A GPU bound is four times the figure printed here; the figures are the *_FIGURES constants of
tests/clip_text_reference.py.  No GPU, no kernel: nothing the code under test produced goes into a bound.

    python tools/exp_clip_text_bounds.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import clip_text_reference as cr  # noqa: E402


def main():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    print("causal attention (B, L, heads): figure")
    for B, L, heads in cr.CAUSAL_BOUNDED:
        qkv = cr.causal_bounded_case(B, L, heads)
        print(f"  {(B, L, heads)}: {cr.rel_max(cr.causal_attention32(qkv, B, L, heads), cr.causal_attention64(qkv, B, L, heads)):.3e}")
    print("QuickGELU linear (rows, Cin, Cout): figure")
    for shape in cr.QGELU_SHAPES:
        c = cr.qgelu_case(*shape)
        print(f"  {shape}: {cr.rel_max(cr.qgelu32(c), cr.qgelu64(c)):.3e}")
    print("prompt mean D: figure")
    for D in cr.PROMPT_D:
        c = cr.prompt_case(D)
        print(f"  {D}: {cr.rel_max(cr.prompt_mean32(c['e'], c['offsets']), cr.prompt_mean64(c['e'], c['offsets'])):.3e}")
    print("tower: figure")
    for name, (geo, _, _) in cr.TOWER_CASES.items():
        got = cr.text_encode32(cr.tower_state(name), cr.tower_ids(name), geo["heads"])
        print(f"  {name}: {cr.rel_max(got, cr.tower_reference(name)):.3e}")


if __name__ == "__main__":
    main()
