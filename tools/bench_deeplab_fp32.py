#!/usr/bin/env python3
"""fp32 DeepLabv3-R50 inference (K16): milliseconds per forward at the frame2recon_full geometry (8 x 3 x 440 x 640, output
stride 16 as the shipped YAMLs set it unless --output-stride says otherwise), seeded random weights, for three paths on the same
weights, interleaved in one run:
  bf16   deeplabv3_resnet50.forward (the training path's bf16-storage kernels, eval mode, no_grad),
  fp32   deeplabv3_resnet50.forward_fp32 (f32-input MFMA convolutions, fp32 pools),
  torch  the oracle's DeepLabV3 moved to the GPU (torch / MIOpen fp32, channels_last).
Then a per-layer-class breakdown of the fp32 forward -- stem (7 x 7 stride 2), 1 x 1, 3 x 3, dilated 3 x 3, pool (max pool +
global average pool) -- from a replay of every layer call of one forward on its own: the HIP kernel and torch's fp32 op of the
same layer (conv + bias [+ residual] [+ ReLU] on channels_last tensors), interleaved; per class the summed time of both, the
FLOPs from the geometry and the achieved fraction of the 157.3 TF f32 matrix peak.  HIP events around --iters back-to-back calls
after --warmup.  Prints one line per row and one JSON line.

    python tools/bench_deeplab_fp32.py [--iters 10] [--warmup 2] [--batch 8] [--output-stride 16]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openess_amd import hip  # noqa: E402
from openess_amd.models.deeplabv3 import deeplabv3_resnet50  # noqa: E402
from oracle import nets as on  # noqa: E402
from tests.synth import fill_by_name  # noqa: E402

PEAK_F32_TF = 157.3
CLASSES = ("stem", "1x1", "3x3", "dilated 3x3", "pool")


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


def record_layers(net, img):
    """One forward_fp32 with the three layer wrappers wrapped: [(class, replay closure for HIP, closure for torch, FLOPs)]."""
    calls = []
    real = hip.conv2d_f32, hip.max_pool_3x3s2_f32, hip.global_avg_pool_f32

    def unpack(packed, Cout, Cin, R, S):
        return packed[:R * S * Cin, :Cout].reshape(R, S, Cin, Cout).permute(3, 2, 0, 1).contiguous(memory_format=torch.channels_last)

    def conv(x, packed, bias, Cout, R, S, stride=1, pad=0, act=None, x2=None, upsample2x=False, residual=None, out=None, dilation=1):
        y = real[0](x, packed, bias, Cout, R, S, stride=stride, pad=pad, act=act, residual=residual, out=out, dilation=dilation)
        cls = "stem" if R == 7 else "1x1" if R == 1 else "3x3" if dilation == 1 else "dilated 3x3"
        xs, rs, w = x.clone(), None if residual is None else residual.clone(), unpack(packed, Cout, x.shape[1], R, S)
        ys = torch.empty_like(y)

        def run_hip():
            real[0](xs, packed, bias, Cout, R, S, stride=stride, pad=pad, act=act, residual=rs, out=ys, dilation=dilation)

        def run_torch():
            t = F.conv2d(xs, w, bias, stride, pad, dilation)
            if rs is not None:
                t = t + rs
            return F.relu(t) if act == 'relu' else t
        calls.append((cls, run_hip, run_torch, 2.0 * y.shape[0] * y.shape[2] * y.shape[3] * Cout * R * S * x.shape[1]))
        return y

    def maxpool(x, out=None):
        y = real[1](x, out=out)
        xs = x.clone()
        calls.append(("pool", lambda: real[1](xs), lambda: F.max_pool2d(xs, 3, 2, 1), 0.0))
        return y

    def avgpool(x):
        y = real[2](x)
        xs = x.clone()
        calls.append(("pool", lambda: real[2](xs), lambda: xs.mean(dim=(2, 3), keepdim=True), 0.0))
        return y

    hip.conv2d_f32, hip.max_pool_3x3s2_f32, hip.global_avg_pool_f32 = conv, maxpool, avgpool
    try:
        net.forward_fp32(img)
    finally:
        hip.conv2d_f32, hip.max_pool_3x3s2_f32, hip.global_avg_pool_f32 = real
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=440)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--output-stride", type=int, default=16)
    ap.add_argument("--only-fp32", action="store_true", help="run the fp32 forward only (for a kernel trace)")
    a = ap.parse_args()
    net = deeplabv3_resnet50(num_classes=11, text_embeddings_path=None, output_stride=a.output_stride, pretrained_backbone='')
    fill_by_name(net, 15)
    net.cuda().eval()
    torch.manual_seed(a.height)
    img = torch.rand(a.batch, 3, a.height, a.width, device="cuda")
    res = {"metric": "deeplab_forward_ms", "size": f"{a.batch}x3x{a.height}x{a.width}", "output_stride": a.output_stride,
           "iters": a.iters, "warmup": a.warmup}
    with torch.no_grad():
        if a.only_fp32:
            res["fp32_ms"] = round(timed(lambda: net.forward_fp32(img), a.iters, a.warmup), 3)
            print(json.dumps(res))
            return
        ref = on.DeepLabV3(11, a.output_stride)
        fill_by_name(ref, 15, sorted(net.state_dict().keys()))
        ref.cuda().eval().to(memory_format=torch.channels_last)
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
        rows = {c: {"layers": 0, "hip_ms": 0.0, "torch_ms": 0.0, "gflop": 0.0} for c in CLASSES}
        for cls, run_hip, run_torch, flop in record_layers(net, img):
            t = {"hip": [], "torch": []}
            for _ in range(2):                                  # interleaved per layer
                t["hip"].append(timed(run_hip, a.iters, a.warmup))
                t["torch"].append(timed(run_torch, a.iters, a.warmup))
            r = rows[cls]
            r["layers"] += 1
            r["hip_ms"] += min(t["hip"])
            r["torch_ms"] += min(t["torch"])
            r["gflop"] += flop / 1e9
        res["classes"] = []
        for cls in CLASSES:
            r = rows[cls]
            tf = r["gflop"] / r["hip_ms"] if r["hip_ms"] > 0 else 0.0          # GFLOP / ms = TFLOP / s
            row = {"class": cls, "layers": r["layers"], "hip_ms": round(r["hip_ms"], 3), "torch_ms": round(r["torch_ms"], 3),
                   "hip_over_torch": round(r["hip_ms"] / r["torch_ms"], 2) if r["torch_ms"] > 0 else None,
                   "gflop": round(r["gflop"], 1), "tflops": round(tf, 1), "frac_of_f32_peak": round(tf / PEAK_F32_TF, 3)}
            print(row, flush=True)
            res["classes"].append(row)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
