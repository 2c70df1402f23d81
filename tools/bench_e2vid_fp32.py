#!/usr/bin/env python3
"""fp32 E2VID inference (K14): frames per second of reconstruct()'s per-frame work (fp32 voxel grid -> EventPreprocessor -> pad ->
recurrent UNet -> image) at 240 x 180, 346 x 260 and 640 x 480, B = 1, E2VID_lightweight (3 encoders) with seeded random weights,
for three paths on the same weights:
  bf16   ImageReconstructor default (the training path's bf16-storage kernels),
  fp32   ImageReconstructor(precision='fp32') (f32-input MFMA kernels),
  torch  the oracle's fp32 E2VIDRecurrent(full=True) moved to the GPU (torch / MIOpen fp32).
Also the fp32 gates conv (3 x 3, cat(x, h) 128 -> 256 at level 0) and the fp32 encoder-0 conv (5 x 5 stride 2, 32 -> 64) alone,
as TFLOP/s from the geometry and as a fraction of the 157.3 TF f32 matrix peak.  HIP events around --iters back-to-back frames
after --warmup frames.  Prints one line per case and one JSON line.

    python tools/bench_e2vid_fp32.py [--iters 50] [--warmup 5]
Kernel trace of fp32 frames: rocprofv3 --kernel-trace --stats -- python tools/bench_e2vid_fp32.py --only-fp32 --iters 1 --warmup 1"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openess_amd import hip  # noqa: E402
from openess_amd.e2vid.image_reconstructor import ImageReconstructor  # noqa: E402
from openess_amd.e2vid.model.model import E2VID_LIGHTWEIGHT_CONFIG, E2VIDRecurrent  # noqa: E402
from oracle import nets as on  # noqa: E402
from tests.synth import fill_by_name  # noqa: E402

PEAK_F32_TF = 157.3
SIZES = ((240, 180), (346, 260), (640, 480))


def time_frames(fn, grid, iters, warmup):
    for _ in range(warmup):
        fn(grid)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn(grid)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters          # ms per frame


def layer_tflops(iters, warmup):
    """The two fp32 layers at 640 x 480 alone (same kernels and epilogues as in the network)."""
    torch.manual_seed(0)
    out = []
    for name, (Cin, H, W, Cout, k, st, act) in (("gates_3x3_128to256_320x240", (128, 240, 320, 256, 3, 1, None)),
                                                ("enc0_5x5s2_32to64_640x480", (32, 480, 640, 64, 5, 2, 'relu'))):
        x = torch.randn(1, Cin, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
        w = hip.pack_conv_weight_f32(torch.randn(Cout, Cin, k, k, device="cuda") * 0.05)
        b = torch.randn(Cout, device="cuda")
        pad = k // 2
        Ho, Wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
        y = torch.empty((1, Ho, Wo, Cout), device="cuda").permute(0, 3, 1, 2)
        ms = time_frames(lambda t: hip.conv2d_f32(t, w, b, Cout, k, k, st, pad, act=act, out=y), x, iters, warmup)
        flop = 2.0 * Ho * Wo * Cout * Cin * k * k
        tf = flop / (ms * 1e-3) / 1e12
        out.append({"layer": name, "us": round(ms * 1e3, 1), "gflop": round(flop / 1e9, 2), "tflops": round(tf, 1),
                    "frac_of_peak": round(tf / PEAK_F32_TF, 3)})
        print(f"{name}: {ms * 1e3:.1f} us, {flop / 1e9:.2f} GFLOP, {tf:.1f} TF/s = {tf / PEAK_F32_TF:.3f} of {PEAK_F32_TF} TF", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only-fp32", action="store_true", help="time the fp32 path only (for a kernel trace)")
    a = ap.parse_args()
    dev = torch.device("cuda")
    m = E2VIDRecurrent(E2VID_LIGHTWEIGHT_CONFIG).eval()
    fill_by_name(m, 11)
    m.cuda()
    ref = None
    if not a.only_fp32:
        ref = on.E2VIDRecurrent(E2VID_LIGHTWEIGHT_CONFIG, full=True).eval()
        fill_by_name(ref, 11, sorted(m.state_dict().keys()))
        ref.cuda()
    res = {"metric": "e2vid_reconstruct_fps", "iters": a.iters, "warmup": a.warmup, "cases": []}
    for W, H in SIZES:
        torch.manual_seed(W)
        grid = (torch.randn(1, 5, H, W) * (torch.rand(1, 5, H, W) > 0.8)).to(dev)
        row = {"size": f"{W}x{H}"}
        paths = (("fp32",),) if a.only_fp32 else (("bf16",), ("fp32",), ("torch",))
        for (p,) in paths:
            with torch.no_grad():
                if p == "torch":
                    crop = ImageReconstructor(m, H, W, 5, dev).crop
                    # the oracle makes its zero initial state on the CPU: start the sequence from the same zeros on the GPU
                    z = [torch.zeros(1, 64 << i, crop.height_crop_size >> (i + 1), crop.width_crop_size >> (i + 1), device=dev)
                         for i in range(3)]
                    state = {"st": [(t, t) for t in z]}

                    def fn(g, crop=crop, state=state):
                        img, state["st"], _ = ref(crop.pad(on.event_preprocess(g)), state["st"])
                        return img
                else:
                    rec = ImageReconstructor(m, H, W, 5, dev, SimpleNamespace(precision=p))

                    def fn(g, rec=rec):
                        return rec.update_reconstruction(g, reconstruct=True)[0]
                ms = time_frames(fn, grid, a.iters, a.warmup)
            row[p + "_ms"] = round(ms, 3)
            row[p + "_fps"] = round(1e3 / ms, 1)
        if "torch_ms" in row:
            row["fp32_speedup_vs_torch"] = round(row["torch_ms"] / row["fp32_ms"], 2)
        print(row, flush=True)
        res["cases"].append(row)
    res["layers_fp32"] = layer_tflops(max(a.iters, 10), max(a.warmup, 2))
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
