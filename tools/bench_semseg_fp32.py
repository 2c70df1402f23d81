#!/usr/bin/env python3
"""fp32 SemSegE2VID inference (K15): milliseconds per forward of the task decoder alone at 1 x 240 x 320, 1 x 440 x 640 and
8 x 480 x 640 (latents of 32 / 64 / 128 / 256 channels at 1, 1/2, 1/4, 1/8 of the size), seeded random weights, for three paths
on the same weights, interleaved in one run:
  bf16   SemSegE2VID.forward (the training path's bf16-storage kernels, no_grad),
  fp32   SemSegE2VID.forward_fp32 (f32-input MFMA convolutions + the fp32 InstanceNorm / upsample-concat kernels),
  torch  the oracle's SemSegE2VID moved to the GPU (torch / MIOpen fp32).
Also the fp32 InstanceNorm kernel alone: GB/s on the 8 x 480 x 640 x 32 map (algorithmic bytes: 4 read for the statistics,
4 read + 4 written for the apply, per element) against the 8 TB/s HBM figure, and its time on the launch-bound 4 x 6 x 256 map.
HIP events around --iters back-to-back forwards after --warmup.  Prints one line per case and one JSON line.

    python tools/bench_semseg_fp32.py [--iters 20] [--warmup 3]
Kernel trace of one fp32 batch: rocprofv3 --kernel-trace --stats -- python tools/bench_semseg_fp32.py --only-fp32 --iters 1 --warmup 1"""
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

HBM_TBS = 8.0
SIZES = ((1, 240, 320), (1, 440, 640), (8, 480, 640))


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


def norm_alone(iters, warmup):
    out = []
    for B, C, H, W in ((8, 32, 480, 640), (1, 256, 4, 6)):
        x = torch.randn(B, H, W, C, device="cuda").permute(0, 3, 1, 2)
        y = torch.empty_like(x)
        ms = timed(lambda: hip.instance_norm_f32(x, relu=True, out=y), iters, warmup)
        gbs = 12.0 * x.numel() / (ms * 1e-3) / 1e9
        out.append({"map": f"{B}x{H}x{W}x{C}", "us": round(ms * 1e3, 1), "gb_per_s": round(gbs, 1), "frac_of_hbm": round(gbs / (HBM_TBS * 1e3), 3)})
        print(f"instance_norm_f32 {B}x{H}x{W}x{C}: {ms * 1e3:.1f} us, {gbs:.0f} GB/s = {gbs / (HBM_TBS * 1e3):.3f} of {HBM_TBS} TB/s", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only-fp32", action="store_true", help="run the fp32 path only, largest size (for a kernel trace)")
    a = ap.parse_args()
    net = SemSegE2VID(256, 11, skip_connect=True, skip_type='concat', text_embeddings_path='', materialize_ch256=False)
    fill_by_name(net, 12)
    net.cuda().eval()
    ref = None
    if not a.only_fp32:
        ref = on.SemSegE2VID(256, 11)
        fill_by_name(ref, 12, sorted(net.state_dict().keys()))
        ref.cuda().eval()
    res = {"metric": "semseg_decoder_ms", "iters": a.iters, "warmup": a.warmup, "cases": []}
    for B, H, W in (SIZES[-1:] if a.only_fp32 else SIZES):
        torch.manual_seed(H)
        lat32 = {s: torch.randn(B, H // s, W // s, 32 * s, device="cuda").permute(0, 3, 1, 2) for s in (1, 2, 4, 8)}
        lat16 = {s: v.to(torch.bfloat16) for s, v in lat32.items()}
        row = {"size": f"{B}x{H}x{W}"}
        paths = {"fp32": lambda: net.forward_fp32(lat32)}
        if not a.only_fp32:
            paths = {"bf16": lambda: net(lat16), "fp32": paths["fp32"], "torch": lambda: ref(lat32)}
        with torch.no_grad():
            acc = {p: [] for p in paths}
            for _ in range(1 if a.only_fp32 else 3):            # interleaved: bf16, fp32, torch, bf16, ...
                for p, fn in paths.items():
                    acc[p].append(timed(fn, a.iters, a.warmup))
        for p, v in acc.items():
            row[p + "_ms"] = round(sorted(v)[len(v) // 2], 3)
        if "torch_ms" in row:
            row["fp32_speedup_vs_torch"] = round(row["torch_ms"] / row["fp32_ms"], 2)
            row["fp32_over_bf16"] = round(row["fp32_ms"] / row["bf16_ms"], 2)
        print(row, flush=True)
        res["cases"].append(row)
    if not a.only_fp32:
        res["instance_norm_f32"] = norm_alone(max(a.iters, 20), max(a.warmup, 3))
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
