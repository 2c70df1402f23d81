#!/usr/bin/env python3
"""How far the bf16 MaskCLIP tower's pseudo-labels sit from the fp32 tower's (K25): both forwards of the same weights on the same
images, one JSON line: the argmax agreement (the fraction of pixels whose dense-CLIP label is the same), the relative RMS of the
bf16 logits against the fp32 ones, and the milliseconds of each.  Without --checkpoint the weights are the seeded random fill of
the tests (tests/vit_f32_cases.py tower_pair's); with the three files of a MaskCLIP checkpoint they are the real tower's.  --refine adds the share of labels MaskCLIP's refinement (K26, forward(img, refine=True)) changes in each
precision, the agreement of the two refined label maps and the milliseconds of the refined forwards.

    python tools/eval_maskclip_precision.py [--batch 8] [--height 440] [--width 640] [--classes 11] [--seed 0]
        [--checkpoint CKPT --text-embeddings PT --visual-projs PT] [--refine [--pd-thresh 0.5] [--ks-thresh 1.0]]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openess_amd.models.maskclip_model import maskClipFeatureExtractor  # noqa: E402


def seeded_fill(m, K, seed):
    """the fill of tests/test_hip_maskclip.py::_pair, applied to the mirror itself"""
    torch.manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('cls_token') or n.endswith('pos_embed'):
                p.normal_(0, 0.3)
            elif 'ln' in n and n.endswith('weight'):
                p.uniform_(0.7, 1.3)
            elif n.endswith('bias'):
                p.normal_(0, 0.1)
        m.decoder.text_embeddings.copy_(torch.nn.functional.normalize(torch.randn(K, 512), dim=1))


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=440)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--classes", type=int, default=11)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--checkpoint")
    ap.add_argument("--text-embeddings")
    ap.add_argument("--visual-projs")
    ap.add_argument("--refine", action="store_true", help="also the share of labels MaskCLIP's refinement changes (K26)")
    ap.add_argument("--pd-thresh", type=float, default=0.5)
    ap.add_argument("--ks-thresh", type=float, default=1.0)
    a = ap.parse_args()
    m = maskClipFeatureExtractor(text_embeddings_path=a.text_embeddings, visual_projs_path=a.visual_projs,
                                 text_categories=a.classes, maskclip_checkpoint=a.checkpoint)
    if not a.checkpoint:
        seeded_fill(m, a.classes, a.seed)
    m.cuda().eval()
    torch.manual_seed(a.seed + 1)
    img = torch.rand(a.batch, 3, a.height, a.width, device="cuda")
    lo, hi = m(img), m.forward_fp32(img)
    agree = float((lo.argmax(1) == hi.argmax(1)).double().mean())
    rel_rms = float(((lo.double() - hi.double()).pow(2).mean() / hi.double().pow(2).mean()).sqrt())
    res = {"metric": "maskclip_bf16_vs_fp32", "size": f"{a.batch}x3x{a.height}x{a.width}", "classes": a.classes,
           "weights": "checkpoint" if a.checkpoint else f"seeded fill {a.seed}", "argmax_agreement": round(agree, 6),
           "logits_rel_rms": float(f"{rel_rms:.4e}"), "bf16_ms": round(timed(lambda: m(img), a.iters, a.warmup), 3),
           "fp32_ms": round(timed(lambda: m.forward_fp32(img), a.iters, a.warmup), 3)}
    if a.refine:
        # K26: MaskCLIP's refinement (prompt denoising + key smoothing) at the decoder's thresholds: the share of the labels it
        # changes in each precision, and how far the two refined label maps agree
        m.decoder.pd_thresh, m.decoder.ks_thresh = a.pd_thresh, a.ks_thresh
        rlo, rhi = m(img, refine=True), m.forward_fp32(img, refine=True)
        res.update({"pd_thresh": a.pd_thresh, "ks_thresh": a.ks_thresh,
                    "refine_changed_bf16": round(float((rlo.argmax(1) != lo.argmax(1)).double().mean()), 6),
                    "refine_changed_fp32": round(float((rhi.argmax(1) != hi.argmax(1)).double().mean()), 6),
                    "refined_argmax_agreement": round(float((rlo.argmax(1) == rhi.argmax(1)).double().mean()), 6),
                    "bf16_refine_ms": round(timed(lambda: m(img, refine=True), a.iters, a.warmup), 3),
                    "fp32_refine_ms": round(timed(lambda: m.forward_fp32(img, refine=True), a.iters, a.warmup), 3)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
