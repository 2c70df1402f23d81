#!/usr/bin/env python3
"""fp32 training of the dilated ResNet-50 backbone (K21): milliseconds per forward + backward of the backbone alone at
8 x 3 x 440 x 640, output stride 16 (replace_stride_with_dilation = [False, False, True]), seeded random weights, every BatchNorm in
train mode, loss = (features * fixed cotangent).sum(), for three paths on the same weights, interleaved in one run, median of three:
  bf16   ResNet.features (the training path's bf16-storage kernels),
  fp32   ResNet.features_fp32_autograd (f32-input MFMA convolutions, wgrad and dgrad; fp32 BatchNorm and max pool each way),
  torch  oracle.nets.ResNet50 moved to the GPU (torch / MIOpen fp32 autograd).
Per kernel family, alone: oess_conv2d_dilated_wgrad_f32 per layer class of the backbone at that size, TFLOP/s
(2 B Ho Wo R^2 Cin Cout) against the 157.3 TF f32 MFMA peak and the number of pixel ranges; oess_batch_norm_bwd_f32 in GB/s of the
bytes it has to move (x and dy read twice, the output read twice with a ReLU, dx and the residual's gradient written once).
HIP events around --iters back-to-back steps after --warmup.  Prints one line per case and one JSON line.

    python tools/bench_resnet_fp32_train.py [--iters 5] [--warmup 2]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openess_amd import _lib, hip  # noqa: E402
from openess_amd.models._resnet import resnet50  # noqa: E402
from oracle import nets as on  # noqa: E402
from tests.synth import damp_residual, fill_by_name  # noqa: E402

F32_MFMA_TF = 157.3
SIZE = (8, 3, 440, 640)
DILATE = [False, False, True]
# (class, Cin, Cout, H, W of the input map, R, stride, pad, dilation) at 8 x 440 x 640
WGRAD_LAYERS = (("stem 7x7 s2", 3, 64, 440, 640, 7, 2, 3, 1), ("layer1 3x3", 64, 64, 110, 160, 3, 1, 1, 1),
                ("layer1 1x1 64->256", 64, 256, 110, 160, 1, 1, 0, 1), ("layer1 1x1 256->64", 256, 64, 110, 160, 1, 1, 0, 1),
                ("layer2 3x3 s2", 128, 128, 110, 160, 3, 2, 1, 1), ("layer2 1x1 s2 downsample", 256, 512, 110, 160, 1, 2, 0, 1),
                ("layer2 3x3", 128, 128, 55, 80, 3, 1, 1, 1), ("layer3 3x3", 256, 256, 28, 40, 3, 1, 1, 1),
                ("layer3 1x1 256->1024", 256, 1024, 28, 40, 1, 1, 0, 1), ("layer4 3x3 d2", 512, 512, 28, 40, 3, 1, 2, 2),
                ("layer4 1x1 512->2048", 512, 2048, 28, 40, 1, 1, 0, 1))
# (class, C, H, W, relu, residual)
BN_LAYERS = (("stem bn1 + relu", 64, 220, 320, True, False), ("layer1 bn3 + residual + relu", 256, 110, 160, True, True),
             ("layer1 downsample bn", 256, 110, 160, False, False), ("layer4 bn3 + residual + relu", 2048, 28, 40, True, True))


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


def wgrad_alone(B, iters, warmup):
    lib, out = _lib.load(), []
    for name, Cin, Cout, H, W, R, stride, pad, dil in WGRAD_LAYERS:
        Ho, Wo = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1, (W + 2 * pad - dil * (R - 1) - 1) // stride + 1
        x = torch.randn(B, H, W, Cin, device="cuda").permute(0, 3, 1, 2)
        if Cin == 3:
            x = x.contiguous()                                  # the image arrives NCHW
        dy = torch.randn(B, Ho, Wo, Cout, device="cuda").permute(0, 3, 1, 2)
        ms = timed(lambda: hip.conv2d_dilated_wgrad_f32(x, dy, R, stride, pad, dil, want_db=False), iters, warmup)
        tf = 2.0 * B * Ho * Wo * R * R * Cin * Cout / (ms * 1e-3) / 1e12
        need = lib.oess_conv2d_dilated_wgrad_f32_workspace_bytes(B, H, W, Cin, Cout, R, R, stride, pad, dil)
        row = {"layer": f"{name}: {B}x{H}x{W} {Cin}->{Cout}", "ranges": need // (4 * (R * R * Cin * Cout + Cout)),
               "us": round(ms * 1e3, 1), "tflops": round(tf, 2), "frac_of_peak": round(tf / F32_MFMA_TF, 3)}
        print("wgrad_f32", row, flush=True)
        out.append(row)
    return out


def bn_bwd_alone(B, iters, warmup):
    out = []
    for name, C, H, W, relu, residual in BN_LAYERS:
        bn = torch.nn.BatchNorm2d(C).cuda().train()
        x = torch.randn(B, H, W, C, device="cuda").permute(0, 3, 1, 2).requires_grad_(True)
        res = torch.randn(B, H, W, C, device="cuda").permute(0, 3, 1, 2).requires_grad_(True) if residual else None
        dy = torch.randn(B, H, W, C, device="cuda").permute(0, 3, 1, 2)
        y = hip.batch_norm_f32_train(x, bn, relu=relu, residual=res)
        leaves = [x, bn.weight, bn.bias] + ([res] if residual else [])
        ms = timed(lambda: torch.autograd.grad(y, leaves, dy, retain_graph=True), iters, warmup)
        elems = B * H * W * C
        nbytes = 4 * elems * (2 + 2 + (2 if relu else 0) + 1 + (1 if residual and relu else 0))
        row = {"layer": f"{name}: {B}x{C}x{H}x{W}", "us": round(ms * 1e3, 1), "gb_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1)}
        print("bn_bwd_f32", row, flush=True)
        out.append(row)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args(argv)
    net = resnet50(replace_stride_with_dilation=DILATE)
    fill_by_name(net, 21)
    damp_residual(net)
    net.cuda().train()
    ref = on.ResNet50(tuple(DILATE))
    fill_by_name(ref, 21, sorted(net.state_dict().keys()))
    damp_residual(ref)
    ref.cuda().train()
    torch.manual_seed(21)
    x = torch.rand(SIZE, device="cuda")
    with torch.no_grad():
        shape = net.features_fp32(x).shape
    cot = torch.randn(shape[0], shape[2], shape[3], shape[1], device="cuda").permute(0, 3, 1, 2)

    def step(module, fwd):
        for p in module.parameters():
            p.grad = None
        (fwd().float() * cot).sum().backward()

    paths = {"bf16": lambda: step(net, lambda: net.features(x)), "fp32": lambda: step(net, lambda: net.features_fp32_autograd(x)),
             "torch": lambda: step(ref, lambda: ref(x))}
    acc = {p: [] for p in paths}
    for _ in range(3):                                          # interleaved: bf16, fp32, torch, bf16, ...
        for p, fn in paths.items():
            acc[p].append(timed(fn, a.iters, a.warmup))
    row = {"size": "x".join(str(v) for v in SIZE), "output_stride": 16}
    for p, v in acc.items():
        row[p + "_ms"] = round(sorted(v)[len(v) // 2], 3)
    row["fp32_speedup_vs_torch"] = round(row["torch_ms"] / row["fp32_ms"], 2)
    row["fp32_over_bf16"] = round(row["fp32_ms"] / row["bf16_ms"], 2)
    print(row, flush=True)
    res = {"metric": "resnet50_backbone_fwd_bwd_ms", "iters": a.iters, "warmup": a.warmup, "backbone": row,
           "wgrad_f32": wgrad_alone(SIZE[0], max(a.iters, 5), max(a.warmup, 2)),
           "bn_bwd_f32": bn_bwd_alone(SIZE[0], max(a.iters, 5), max(a.warmup, 2)), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
