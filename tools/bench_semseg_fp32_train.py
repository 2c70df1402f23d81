#!/usr/bin/env python3
"""fp32 SemSegE2VID training layers (K18): milliseconds per forward + backward of the task decoder alone at 1 x 240 x 320 and
8 x 480 x 640 (latents of 32 / 64 / 128 / 256 channels at 1, 1/2, 1/4, 1/8 of the size, no gradient asked for them), seeded random
weights, loss = (logits * fixed cotangent).sum(), for three paths on the same weights, interleaved in one run, median of three:
  bf16   SemSegE2VID.forward (the training path's bf16-storage kernels),
  fp32   SemSegE2VID.forward_fp32_train (f32-input MFMA convolutions, wgrad and dgrad; fp32 InstanceNorm / upsample-concat),
  torch  the oracle's SemSegE2VID moved to the GPU (torch / MIOpen fp32 autograd).
Also oess_conv2d_wgrad_f32 alone per decoder layer shape at 8 x 480 x 640: TFLOP/s (2 B H W R^2 Cin Cout) against the 157.3 TF
f32 MFMA peak, and the number of pixel ranges.  HIP events around --iters back-to-back steps after --warmup.  Prints one line per
case and one JSON line.

    python tools/bench_semseg_fp32_train.py [--iters 5] [--warmup 2]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openess_amd import hip  # noqa: E402
from openess_amd.models.style_networks import SemSegE2VID  # noqa: E402
from oracle import nets as on  # noqa: E402
from tests.synth import fill_by_name  # noqa: E402

F32_MFMA_TF = 157.3
SIZES = ((1, 240, 320), (8, 480, 640))
# (scale of the map, Cin, Cout, R): the decoder's distinct convolutions
LAYERS = ((8, 256, 256, 3), (8, 256, 128, 3), (4, 256, 128, 3), (4, 128, 64, 3), (2, 128, 64, 3), (2, 64, 64, 3), (1, 64, 32, 3),
          (1, 32, 11, 1))


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


def wgrad_alone(B, H, W, iters, warmup):
    out = []
    for s, Cin, Cout, R in LAYERS:
        h, w = H // s, W // s
        x = torch.randn(B, h, w, Cin, device="cuda").permute(0, 3, 1, 2)
        dy = torch.randn(B, h, w, Cout, device="cuda").permute(0, 3, 1, 2)
        ms = timed(lambda: hip.conv2d_wgrad_f32(x, dy, R), iters, warmup)
        tf = 2.0 * B * h * w * R * R * Cin * Cout / (ms * 1e-3) / 1e12
        row = {"layer": f"{B}x{h}x{w} {Cin}->{Cout} {R}x{R}", "ranges": hip.conv2d_wgrad_f32_splits(B, h, w, Cin, Cout, R),
               "us": round(ms * 1e3, 1), "tflops": round(tf, 2), "frac_of_peak": round(tf / F32_MFMA_TF, 3)}
        print("wgrad_f32", row, flush=True)
        out.append(row)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args(argv)
    net = SemSegE2VID(256, 11, skip_connect=True, skip_type='concat', text_embeddings_path='', materialize_ch256=False)
    fill_by_name(net, 12)
    net.cuda().train()
    ref = on.SemSegE2VID(256, 11)
    fill_by_name(ref, 12, sorted(net.state_dict().keys()))
    ref.cuda().train()
    res = {"metric": "semseg_decoder_fwd_bwd_ms", "iters": a.iters, "warmup": a.warmup, "cases": []}
    for B, H, W in SIZES:
        torch.manual_seed(H)
        lat32 = {s: torch.randn(B, H // s, W // s, 32 * s, device="cuda").permute(0, 3, 1, 2) for s in (1, 2, 4, 8)}
        lat16 = {s: v.to(torch.bfloat16) for s, v in lat32.items()}
        cot = torch.randn(B, H, W, 11, device="cuda").permute(0, 3, 1, 2)

        def step(module, fwd):
            for p in module.parameters():
                p.grad = None
            (fwd()[0][1] * cot).sum().backward()

        paths = {"bf16": lambda: step(net, lambda: net(lat16)), "fp32": lambda: step(net, lambda: net.forward_fp32_train(lat32)),
                 "torch": lambda: step(ref, lambda: ref(lat32))}
        acc = {p: [] for p in paths}
        for _ in range(3):                                      # interleaved: bf16, fp32, torch, bf16, ...
            for p, fn in paths.items():
                acc[p].append(timed(fn, a.iters, a.warmup))
        row = {"size": f"{B}x{H}x{W}"}
        for p, v in acc.items():
            row[p + "_ms"] = round(sorted(v)[len(v) // 2], 3)
        row["fp32_speedup_vs_torch"] = round(row["torch_ms"] / row["fp32_ms"], 2)
        row["fp32_over_bf16"] = round(row["fp32_ms"] / row["bf16_ms"], 2)
        print(row, flush=True)
        res["cases"].append(row)
    res["wgrad_f32"] = wgrad_alone(*SIZES[-1], max(a.iters, 5), max(a.warmup, 2))
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
