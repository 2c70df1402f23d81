#!/usr/bin/env python3
"""fp32 training of the whole DeepLabv3-R50 (K22): milliseconds per forward + backward at 8 x 3 x 440 x 640, output stride 16,
seeded random weights, every BatchNorm in train mode, Dropout(0.1) on, loss = (full-size logits * fixed cotangent).sum(), for
three paths on the same weights, interleaved in one run, median of three:
  bf16   deeplabv3_resnet50.forward (the training path's bf16-storage kernels),
  fp32   deeplabv3_resnet50.forward_fp32_train (the K18 / K21 / K22 fp32 layer set; the full-size feature map is not formed),
  torch  oracle.nets.DeepLabV3 moved to the GPU (torch / MIOpen fp32 autograd; logits only, its full-size feature map is left out
         as well).
--backbone-too: the backbone alone through ResNet.features_fp32_autograd on the same input, to split the step.
HIP events around --iters back-to-back steps after --warmup.  Prints one JSON line.

    python tools/bench_deeplab_fp32_train.py [--iters 5] [--warmup 2] [--backbone-too]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openess_amd.models.deeplabv3 import deeplabv3_resnet50  # noqa: E402
from oracle import nets as on  # noqa: E402
from tests.synth import damp_residual, fill_by_name  # noqa: E402

SIZE, K = (8, 3, 440, 640), 11


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--backbone-too", action="store_true")
    a = ap.parse_args(argv)
    net = deeplabv3_resnet50(K, '', 16, '')
    fill_by_name(net, 22)
    damp_residual(net)
    net.cuda().train()
    ref = on.DeepLabV3(K, output_stride=16)
    fill_by_name(ref, 22, sorted(net.state_dict().keys()))
    damp_residual(ref)
    ref.cuda().train()
    torch.manual_seed(22)
    x = torch.rand(SIZE, device="cuda")
    cot = torch.randn(SIZE[0], SIZE[2], SIZE[3], K, device="cuda").permute(0, 3, 1, 2)

    def step(module, fwd):
        for p in module.parameters():
            p.grad = None
        (fwd().float() * cot).sum().backward()

    def torch_logits():
        logits, _ = ref.classifier(ref.backbone(x))
        return F.interpolate(logits, size=SIZE[2:], mode='bilinear', align_corners=False)

    paths = {"bf16": lambda: step(net, lambda: net(x)[0]), "fp32": lambda: step(net, lambda: net.forward_fp32_train(x)[0]),
             "torch": lambda: step(ref, torch_logits)}
    if a.backbone_too:
        body = net.backbone

        def backbone_step():
            for p in body.parameters():
                p.grad = None
            y = body.forward_fp32_autograd(x)['out']
            y.backward(torch.ones_like(y))
        paths["fp32_backbone"] = backbone_step
    acc = {p: [] for p in paths}
    for _ in range(3):                                          # interleaved: bf16, fp32, torch, bf16, ...
        for p, fn in paths.items():
            acc[p].append(timed(fn, a.iters, a.warmup))
    row = {"size": "x".join(str(v) for v in SIZE), "output_stride": 16}
    for p, v in acc.items():
        row[p + "_ms"] = round(sorted(v)[len(v) // 2], 3)
    row["fp32_speedup_vs_torch"] = round(row["torch_ms"] / row["fp32_ms"], 2)
    row["fp32_over_bf16"] = round(row["fp32_ms"] / row["bf16_ms"], 2)
    res = {"metric": "deeplabv3_r50_fwd_bwd_ms", "iters": a.iters, "warmup": a.warmup, "model": row,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
