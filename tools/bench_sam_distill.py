#!/usr/bin/env python3
"""The fused SAM distillation node (K34, hip.sam_distill_loss on a hip.UpsampledFeature) against the composed path it replaces
(hip.bilinear_resize of the student map, the resize and crop of the SAM map, hip.cosine_mean_loss), at the pre-training step's
size: a bf16 8 x 256 x 28 x 40 map -> 440 x 640 against an fp32 8 x 256 x 64 x 64 SAM map.  For each: forward + backward time
(device events, interleaved rounds, the median) and torch.cuda.max_memory_allocated over forward + backward above what is live
before the call.  Then the frame2recon pre-training step (contrastive + dense-CLIP) with the key on and off, the same way.
    python tools/bench_sam_distill.py [--iters 10] [--rounds 3] [--shape 8 256 28 40 440 640] [--sam 64 64] [--step-iters 3]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(routes, iters, rounds):
    """{name: [ms per call, one per round]}: the routes take turns inside every round"""
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for name, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / iters)
    return times


def _measure(routes, iters, rounds):
    out = {}
    for name, fn in routes.items():                       # warm-up, then the peak of one call
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        value = fn()
        torch.cuda.synchronize()
        out[name] = {"peak_bytes": torch.cuda.max_memory_allocated() - base, "loss": float(value)}
    for name, v in _timed(routes, iters, rounds).items():
        out[name]["fwd_bwd_ms"] = round(sorted(v)[len(v) // 2], 3)
        out[name]["rounds_ms"] = [round(t, 3) for t in v]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=6, default=[8, 256, 28, 40, 440, 640], metavar=("B", "C", "h", "w", "Ho", "Wo"))
    ap.add_argument("--sam", type=int, nargs=2, default=[64, 64], metavar=("hs", "ws"))
    ap.add_argument("--step-iters", type=int, default=3, help="0: skip the pre-training step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sam_distill needs the GPU")
    from openess_amd import hip
    B, C, h, w, Ho, Wo = args.shape
    g = torch.Generator().manual_seed(34)
    a = torch.randn(B, C, h, w, generator=g).cuda().bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    sam = (1 + 0.5 * torch.randn(B, C, *args.sam, generator=g)).cuda()

    def node(feat):
        def run():
            a.grad = None
            loss = hip.sam_distill_loss(sam, feat())
            loss.backward()
            return loss.detach()
        return run
    routes = {"fused": node(lambda: hip.UpsampledFeature(a, (Ho, Wo), False)),
              "composed": node(lambda: hip.bilinear_resize(a, size=(Ho, Wo), align_corners=False))}
    out = {"shape": args.shape, "sam": args.sam, "full_resolution_bf16_bytes": B * C * Ho * Wo * 2, "iters": args.iters, "rounds": args.rounds}
    out.update(_measure(routes, args.iters, args.rounds))
    out["fused_over_composed_ms"] = round(out["fused"]["fwd_bwd_ms"] / out["composed"]["fwd_bwd_ms"], 3)
    print(json.dumps(out), flush=True)
    if args.step_iters <= 0:
        return
    del a, routes
    torch.cuda.empty_cache()
    from openess_amd.training.pretrain_step import PretrainStep
    K, sps = 11, 100
    frame = torch.rand(B, 3, Ho, Wo, generator=g).cuda()
    pl = torch.randint(0, K, (B, Ho, Wo), generator=g).cuda()
    gy, gx = torch.arange(Ho) * 10 // Ho, torch.arange(Wo) * 10 // Wo
    sp = (gy[:, None] * 10 + gx[None, :]).expand(B, Ho, Wo).contiguous().cuda()
    batch = (frame, None, frame, pl, sp, (B - 1) * sps + 100)
    steps = {}
    for name, on in (("sam_on", True), ("sam_off", False)):
        st = PretrainStep(config_option="frame2recon", img_size=(Ho, Wo), if_spatial_contrastive=True, superpixel_size=sps,
                          sam_distillation=on)

        def run(st=st, on=on):
            return st.train_step(batch, sam_feat=sam if on else None)[2]
        steps[name] = run
    res = {"step": "frame2recon, contrastive + dense-CLIP", "batch": B, "iters": args.step_iters, "rounds": args.rounds}
    res.update(_measure(steps, args.step_iters, args.rounds))
    res["sam_on_minus_off_ms"] = round(res["sam_on"]["fwd_bwd_ms"] - res["sam_off"]["fwd_bwd_ms"], 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
