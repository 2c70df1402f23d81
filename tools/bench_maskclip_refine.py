#!/usr/bin/env python3
"""MaskCLIP refinement (K26: prompt denoising + key smoothing, hip.maskclip_refine) on the GPU, seeded random operands:

  * the refinement alone at 8 x 11 x 28 x 40 logits and C = 768 keys (the tower's shapes at 8 x 3 x 440 x 640), with fp32 and with
    bf16 keys read in place from a [B (L + 1), C] token matrix: microseconds of each of the five kernels (HIP events between the
    launches, medians), GB/s of the two passes over k counted over the bytes of k alone, and the whole call;
  * next to it torch fp32 on the GPU doing what the reference does (the explicit form of tests/maskclip_refine_reference.py:
    softmax, normalisation over the token axis, (k^ k^T) @ P with its L x L matrix, the selection);
  * the last layer's key path (LayerNorm + two token GEMMs) in both precisions;
  * the tower's forward with and without refine=True, bf16 and fp32, interleaved in one run, medians.

Prints one line per row and one JSON line.

    python tools/bench_maskclip_refine.py [--iters 20] [--warmup 3] [--batch 8] [--height 440] [--width 640] [--no-tower]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openess_amd import hip  # noqa: E402
from tests import maskclip_refine_reference as refine_reference  # noqa: E402
from openess_amd.models.maskclip_model import maskClipFeatureExtractor  # noqa: E402
from tools.eval_maskclip_precision import seeded_fill, timed  # noqa: E402

PHASES = ("conf", "prob", "gram", "hm", "apply")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=440)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--classes", type=int, default=11)
    ap.add_argument("--no-tower", action="store_true")
    a = ap.parse_args()
    B, K, C = a.batch, a.classes, 768
    hp, wp = (a.height + 15) // 16, (a.width + 15) // 16
    L = hp * wp
    g = torch.Generator().manual_seed(0)
    logits = (0.2 + 0.03 * torch.randn(B, hp, wp, K, generator=g)).cuda().permute(0, 3, 1, 2)       # the tower's NHWC memory
    tok = torch.randn(B * (L + 1), C, generator=g).cuda()
    res = {"metric": "maskclip_refine", "size": f"{B}x{K}x{hp}x{wp}", "C": C, "iters": a.iters, "warmup": a.warmup}
    with torch.no_grad():
        for name, t in (("k_fp32", tok), ("k_bf16", tok.bfloat16())):
            k = t.view(B, L + 1, C)[:, 1:]
            kbytes = B * L * C * t.element_size()
            for _ in range(a.warmup):
                hip.maskclip_refine(logits, k)
            runs = [hip.maskclip_refine_phase_ms(logits, k) for _ in range(a.iters)]
            us = {p: round(1e3 * statistics.median(r[p] for r in runs), 2) for p in PHASES}
            row = {"kernel_us": us, "kernel_sum_us": round(sum(us.values()), 2), "k_MB": round(kbytes / 1e6, 2),
                   "gram_GBps": round(kbytes / us["gram"] / 1e3, 1), "apply_GBps": round(kbytes / us["apply"] / 1e3, 1),
                   "call_us": round(1e3 * statistics.median(timed(lambda: hip.maskclip_refine(logits, k), a.iters, a.warmup)
                                                            for _ in range(3)), 2)}
            res[name] = row
            print(f"{name}: " + "  ".join(f"{p} {us[p]:.2f} us" for p in PHASES) + f"  | sum {row['kernel_sum_us']:.2f} us, call "
                  f"{row['call_us']:.2f} us; k {row['k_MB']} MB: gram {row['gram_GBps']} GB/s, apply {row['apply_GBps']} GB/s")
        kf = tok.view(B, L + 1, C)[:, 1:]
        explicit = lambda: refine_reference.refine(logits, kf, 0.5, 1.0, form="explicit", dtype=torch.float32)
        res["torch_explicit_us"] = round(1e3 * statistics.median(timed(explicit, a.iters, a.warmup) for _ in range(3)), 2)
        print(f"torch explicit (k^ k^T) @ P on the GPU: {res['torch_explicit_us']:.2f} us")
        if not a.no_tower:
            m = maskClipFeatureExtractor(text_categories=K)
            seeded_fill(m, K, 0)
            m.cuda().eval()
            torch.manual_seed(a.height)
            img = torch.rand(B, 3, a.height, a.width, device="cuda")
            last = m.encoder.layers[-1]
            x32 = torch.randn(B * (L + 1), C, device="cuda")
            x16 = x32.bfloat16()
            paths = {"key_path_bf16": lambda: last.forward_key_path(x16), "key_path_fp32": lambda: last.forward_key_path_fp32(x32),
                     "bf16": lambda: m(img), "bf16_refine": lambda: m(img, refine=True),
                     "fp32": lambda: m.forward_fp32(img), "fp32_refine": lambda: m.forward_fp32(img, refine=True)}
            acc = {p: [] for p in paths}
            for _ in range(3):                                      # interleaved
                for p, fn in paths.items():
                    acc[p].append(timed(fn, max(a.iters // 4, 3), 1))
            for p in paths:
                res[p + "_ms"] = round(statistics.median(acc[p]), 3)
                print(f"{p:14s} {res[p + '_ms']:9.3f} ms  (runs {', '.join(f'{t:.3f}' for t in acc[p])})")
            for p in ("bf16", "fp32"):
                res[p + "_refine_overhead"] = round(res[p + "_refine_ms"] / res[p + "_ms"] - 1.0, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
