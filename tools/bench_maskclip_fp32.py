#!/usr/bin/env python3
"""fp32 MaskCLIP ViT-B/16 tower (K25): milliseconds per forward at 8 x 3 x 440 x 640 (1121 tokens per image), seeded random
weights, for three paths on the same weights, interleaved in one run, medians:
  bf16   maskClipFeatureExtractor.forward (bf16 storage, bf16 MFMA),
  fp32   maskClipFeatureExtractor.forward_fp32 (f32-input MFMA token GEMMs and attention, fp32 LayerNorm),
  torch  the restatement oracle/maskclip.py moved to the GPU (torch fp32).
Then a per-kernel breakdown of the fp32 forward from a replay of every token-kernel call of one forward on its own: the token
GEMMs per layer class (patch, qkv, v, out, fc1, fc2, proj, text) in TFLOP/s with the fraction of the 157.3 TFLOP/s f32 matrix
peak, the attention launch in microseconds (30.9 GFLOP per layer at B = 8), LayerNorm in GB/s.  HIP events around --iters
back-to-back calls after --warmup.  Prints one line per row and one JSON line.

    python tools/bench_maskclip_fp32.py [--iters 5] [--warmup 1] [--batch 8] [--height 440] [--width 640] [--no-torch]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openess_amd import hip  # noqa: E402
from openess_amd.models.maskclip_model import maskClipFeatureExtractor  # noqa: E402
from tools.eval_maskclip_precision import seeded_fill, timed  # noqa: E402

PEAK_F32_TF = 157.3
GEMM_CLASS = {(768, 768, None): "patch", (768, 2304, None): "qkv", (768, 768, 'res'): "out", (768, 3072, 'gelu'): "fc1",
              (3072, 768, 'res'): "fc2", (768, 512, None): "proj"}


def record(m, img):
    """one forward_fp32 with the three wrappers wrapped: [(class, replay closure, FLOPs, bytes)]"""
    calls = []
    real = hip.linear_tokens_f32, hip.attention_d64_f32, hip.layer_norm_tokens_f32

    def lin(x, packed, bias, Cout, act=None, residual=None, out=None):
        y = real[0](x, packed, bias, Cout, act=act, residual=residual, out=out)
        rows, Cin = x.shape
        key = (Cin, Cout, 'gelu' if act else 'res' if residual is not None else None)
        cls = GEMM_CLASS.get(key, "text" if Cin == 512 else "v" if (Cin, Cout) == (768, 768) else f"{Cin}x{Cout}")
        if cls == "patch" and rows != img.shape[0] * ((img.shape[2] + 15) // 16) * ((img.shape[3] + 15) // 16):
            cls = "v"                                              # 768 -> 768 without residual: the patch GEMM or the value slice
        xs, rs, ys = x.clone(), None if residual is None else residual.clone(), torch.empty_like(y)
        calls.append((cls, lambda: real[0](xs, packed, bias, Cout, act=act, residual=rs, out=ys), 2.0 * rows * Cin * Cout, 0))
        return y

    def att(qkv, B, L, heads, out=None):
        y = real[1](qkv, B, L, heads, out=out)
        qs, ys = qkv.clone(), torch.empty_like(y)
        calls.append(("attention", lambda: real[1](qs, B, L, heads, out=ys), 4.0 * B * heads * L * L * 64, 0))
        return y

    def ln(x, gamma, beta, eps=1e-6, out=None):
        y = real[2](x, gamma, beta, eps, out=out)
        xs, ys = x.clone(), torch.empty_like(y)
        calls.append(("layernorm", lambda: real[2](xs, gamma, beta, eps, out=ys), 0.0, 8.0 * x.numel()))
        return y

    hip.linear_tokens_f32, hip.attention_d64_f32, hip.layer_norm_tokens_f32 = lin, att, ln
    try:
        m.forward_fp32(img)
    finally:
        hip.linear_tokens_f32, hip.attention_d64_f32, hip.layer_norm_tokens_f32 = real
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=440)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    K = 11
    m = maskClipFeatureExtractor(text_categories=K)
    seeded_fill(m, K, 0)
    m.cuda().eval()
    torch.manual_seed(a.height)
    img = torch.rand(a.batch, 3, a.height, a.width, device="cuda")
    res = {"metric": "maskclip_forward_ms", "size": f"{a.batch}x3x{a.height}x{a.width}", "iters": a.iters, "warmup": a.warmup}
    paths = {"bf16": lambda: m(img), "fp32": lambda: m.forward_fp32(img)}
    if not a.no_torch:
        from oracle.maskclip import maskClipFeatureExtractor as Oracle
        ref = Oracle(K)
        ref.load_state_dict(m.state_dict())
        ref.cuda().eval()
        paths["torch"] = lambda: ref(img)
    with torch.no_grad():
        acc = {p: [] for p in paths}
        for _ in range(3):                                          # interleaved: bf16, fp32, torch, bf16, ...
            for p, fn in paths.items():
                acc[p].append(timed(fn, a.iters, a.warmup))
        for p in paths:
            res[p + "_ms"] = round(statistics.median(acc[p]), 3)
            print(f"{p:6s} forward {res[p + '_ms']:9.3f} ms  (runs {', '.join(f'{t:.3f}' for t in acc[p])})")
        calls = record(m, img)
        by = {}
        for cls, fn, flops, nbytes in calls:
            t = statistics.median(timed(fn, a.iters, a.warmup) for _ in range(3))
            e = by.setdefault(cls, [0, 0.0, 0.0, 0.0])
            e[0] += 1; e[1] += t; e[2] += flops; e[3] += nbytes
    rows = {}
    for cls, (n, ms, flops, nbytes) in by.items():
        row = {"calls": n, "ms": round(ms, 3)}
        if cls == "layernorm":
            row["GBps"] = round(nbytes / ms / 1e6, 1)
            print(f"{cls:10s} {n:3d} calls {ms:8.3f} ms  {row['GBps']:8.1f} GB/s")
        else:
            row["TFLOPs"] = round(flops / ms / 1e9, 2)
            row["of_f32_peak"] = round(flops / ms / 1e9 / PEAK_F32_TF, 3)
            if cls == "attention":
                row["us_per_launch"] = round(1e3 * ms / n, 1)
            print(f"{cls:10s} {n:3d} calls {ms:8.3f} ms  {row['TFLOPs']:7.2f} TFLOP/s  {100 * row['of_f32_peak']:5.1f} % of the f32 matrix peak"
                  + (f"  {row['us_per_launch']:.1f} us per launch" if cls == "attention" else ""))
        rows[cls] = row
    res["kernels"] = rows
    res["kernel_sum_ms"] = round(sum(r["ms"] for r in rows.values()), 3)
    res["gflop"] = round(sum(v[2] for v in by.values()) / 1e9, 1)
    res["floor_ms_at_f32_peak"] = round(sum(v[2] for v in by.values()) / 1e9 / PEAK_F32_TF, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
