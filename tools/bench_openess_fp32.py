#!/usr/bin/env python3
"""The fused upsampled-L1 node (K23, hip.upsampled_l1_mean) against what it replaces, hip.l1_mean on the same two fp32
hip.UpsampledFeature, at the joint stage's size: 8 x 256 x 28 x 40 -> 440 x 640.  For each: forward + backward time (device
events, interleaved rounds, the median) and torch.cuda.max_memory_allocated over forward + backward, above what the operands hold.
Algorithmic bytes: the fused node reads the two 9.2 MB maps (forward: once per chunk of output rows from L2; backward: nine taps
each) and writes two 9.2 MB gradients; the chain writes and reads the 2.3 GB difference and its 2.3 GB gradient.
    python tools/bench_openess_fp32.py [--iters 10] [--rounds 3] [--shape 8 256 28 40 440 640]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=6, default=[8, 256, 28, 40, 440, 640], metavar=("B", "C", "h", "w", "Ho", "Wo"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_openess_fp32 needs the GPU")
    from openess_amd import hip
    B, C, h, w, Ho, Wo = args.shape
    g = torch.Generator().manual_seed(23)
    a = torch.randn(B, C, h, w, generator=g).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    b = torch.randn(B, C, h, w, generator=g).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    routes = {"fused": hip.upsampled_l1_mean, "materialised": hip.l1_mean}

    def step(fn):
        a.grad = b.grad = None
        loss = fn(hip.UpsampledFeature(a, (Ho, Wo), False), hip.UpsampledFeature(b, (Ho, Wo), False))
        loss.backward()
        return loss.detach()

    out = {"shape": args.shape, "full_resolution_bytes": B * C * Ho * Wo * 4, "iters": args.iters, "rounds": args.rounds}
    loss, times = {}, {k: [] for k in routes}
    for name, fn in routes.items():                       # warm-up, then the peak of one forward + backward
        step(fn)
        a.grad = b.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss[name] = float(step(fn))
        torch.cuda.synchronize()
        out[name] = {"peak_bytes": torch.cuda.max_memory_allocated() - base, "loss": loss[name]}
    for _ in range(args.rounds):
        for name, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.iters):
                step(fn)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.iters)
    for name, v in times.items():
        out[name]["fwd_bwd_ms"] = round(sorted(v)[len(v) // 2], 3)
        out[name]["rounds_ms"] = [round(t, 3) for t in v]
    out["fused_over_materialised_ms"] = round(out["fused"]["fwd_bwd_ms"] / out["materialised"]["fwd_bwd_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
