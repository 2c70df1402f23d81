#!/usr/bin/env python3
"""fp32 image teacher (K17): milliseconds per forward at the pretraining geometry (8 x 3 x 440 x 640, a 110 x 160 map from
layer1 on), seeded random weights, BatchNorm in train mode as the reference leaves it, for three paths on the same weights,
interleaved in one run:
  bf16   DilationFeatureExtractor.forward (the training path's bf16-storage kernels, no_grad),
  fp32   DilationFeatureExtractor.forward_fp32 (f32-input MFMA convolutions, the train-mode BatchNorm kernel),
  torch  the oracle's DilationFeatureExtractor moved to the GPU (torch / MIOpen fp32, channels_last).
Then the train-mode BatchNorm launches on their own: every distinct (shape, residual, ReLU) call of one forward_fp32 is
replayed on fresh tensors of that shape; per geometry the time of the three launches together and the GB/s of the traffic the
kernel cannot avoid (the input read twice, the output written once, the residual read once: 12 or 16 bytes per element).
HIP events around --iters back-to-back calls after --warmup.  Prints one line per row and one JSON line.

    python tools/bench_teacher_fp32.py [--iters 5] [--warmup 2] [--batch 8]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openess_amd import hip  # noqa: E402
from openess_amd.models.image_model import DilationFeatureExtractor  # noqa: E402
from oracle import nets as on  # noqa: E402
from tests.synth import fill_by_name  # noqa: E402


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


def record_batch_norms(net, img):
    """One forward_fp32 with the BatchNorm wrapper wrapped: {(shape, has residual, relu): number of calls}."""
    seen = {}
    real = hip.batch_norm_train_f32

    def bn(x, m, relu=False, residual=None, out=None, return_stats=False):
        key = (tuple(x.shape), residual is not None, bool(relu))
        seen[key] = seen.get(key, 0) + 1
        return real(x, m, relu=relu, residual=residual, out=out, return_stats=return_stats)

    hip.batch_norm_train_f32 = bn
    try:
        net.forward_fp32(img)
    finally:
        hip.batch_norm_train_f32 = real
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=440)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--only-fp32", action="store_true", help="run the fp32 forward only (for a kernel trace)")
    a = ap.parse_args()
    net = DilationFeatureExtractor(None)
    fill_by_name(net.encoder, 13)
    fill_by_name(net.decoder[0], 14)
    net.cuda().train()
    torch.manual_seed(a.height)
    img = torch.rand(a.batch, 3, a.height, a.width, device="cuda")
    res = {"metric": "teacher_forward_ms", "size": f"{a.batch}x3x{a.height}x{a.width}", "iters": a.iters, "warmup": a.warmup}
    with torch.no_grad():
        if a.only_fp32:
            res["fp32_ms"] = round(timed(lambda: net.forward_fp32(img), a.iters, a.warmup), 3)
            print(json.dumps(res))
            return
        ref = on.DilationFeatureExtractor()
        fill_by_name(ref.encoder, 13, sorted(net.encoder.state_dict().keys()))
        fill_by_name(ref.decoder[0], 14)
        ref.cuda().train().to(memory_format=torch.channels_last)
        img_cl = img.contiguous(memory_format=torch.channels_last)
        paths = {"bf16": lambda: net(img), "fp32": lambda: net.forward_fp32(img), "torch": lambda: ref(img_cl)}
        acc = {p: [] for p in paths}
        for _ in range(3):                                      # interleaved: bf16, fp32, torch, bf16, ...
            for p, fn in paths.items():
                acc[p].append(timed(fn, a.iters, a.warmup))
        for p, v in acc.items():
            res[p + "_ms"] = round(sorted(v)[len(v) // 2], 3)
        res["fp32_speedup_vs_torch"] = round(res["torch_ms"] / res["fp32_ms"], 2)
        res["fp32_over_bf16"] = round(res["fp32_ms"] / res["bf16_ms"], 2)
        print({k: res[k] for k in ("size", "bf16_ms", "fp32_ms", "torch_ms", "fp32_speedup_vs_torch", "fp32_over_bf16")}, flush=True)
        res["batch_norm"] = []
        total_ms = total_bytes = 0.0
        for (shape, has_res, relu), calls in sorted(record_batch_norms(net, img).items()):
            B, C, H, W = shape
            x = torch.randn(B, H, W, C, device="cuda").permute(0, 3, 1, 2)
            r = torch.randn(B, H, W, C, device="cuda").permute(0, 3, 1, 2) if has_res else None
            y = torch.empty_like(x)
            bn = torch.nn.BatchNorm2d(C).cuda()
            ms = min(timed(lambda: hip.batch_norm_train_f32(x, bn, relu=relu, residual=r, out=y), a.iters, a.warmup) for _ in range(2))
            nbytes = x.numel() * 4.0 * (4 if has_res else 3)
            row = {"shape": f"{B}x{C}x{H}x{W}", "residual": has_res, "relu": relu, "calls": calls, "ms": round(ms, 3),
                   "gbytes": round(nbytes / 1e9, 3), "gb_per_s": round(nbytes / 1e6 / ms, 1)}
            print(row, flush=True)
            res["batch_norm"].append(row)
            total_ms += ms * calls
            total_bytes += nbytes * calls
            del x, r, y
        res["batch_norm_ms"] = round(total_ms, 3)
        res["batch_norm_gb_per_s"] = round(total_bytes / 1e6 / total_ms, 1)
        res["batch_norm_share_of_fp32"] = round(total_ms / res["fp32_ms"], 3)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
