#!/usr/bin/env python3
"""fp32 pre-training of frame2voxel against the bf16 step, and the fused fp32 head-pool node against the materialised fp32 chain
(DESIGN.md K20).  Needs the GPU.

  step:  PretrainStep(frame2voxel, contrastive loss on) with precision 'bf16' and 'fp32' on the same batch, one step of each in
         turn (interleaved, so clock and thermal drift hit both alike), HIP events around train_step; medians.
  node:  k = pool(normalize(upsample_x4(x))) forward + backward on an fp32 [B, 256, H/4, W/4] map: the fused node
         (hip.UpsampledNormalizedFeature.pool) and the chain it replaces (bilinear_resize -> l2_normalize -> superpixel_pool, what
         pooled_teacher_features=False runs), interleaved, HIP events; GB/s against byte counts DERIVED FROM THE SHAPES
         (not measured): with full = B C Ho Wo 4 bytes, x = full / 16, tmp = full / 4 (the x-pass intermediate), ids = B Ho Wo 8,
             materialised = 4 full (resize write, normalise read + write, pool read)
                          + 5 full + 2 tmp + x (pool adjoint write, L2 adjoint 2 reads + 1 write, x pass read + tmp write, y pass)
             fused        = 2 x (forward, backward) + 2 ids + 2 tmp + x (grad_x)

    python tools/bench_pretrain_fp32.py [--steps N] [--warmup W] [--batch B] [--height H --width W] [--nwin N] [--parts node,step]
The defaults are the BASELINE size (8 x 440 x 640, 20 sub-windows).  The last line is one JSON object."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPS, BINS, K = 100, 5, 11


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _interleaved(fns, steps, warmup):
    """{name: median ms} of the callables run in turn, `warmup` untimed rounds first"""
    ms = {n: [] for n in fns}
    for it in range(warmup + steps):
        for n, fn in fns.items():
            t = _timed(fn)
            if it >= warmup:
                ms[n].append(t)
    return {n: statistics.median(v) for n, v in ms.items()}


def _superpixels(B, H, W, g):
    """blocky maps (8 x 8 blocks of one id, ids < SPS), as bench.py's stage rooflines use"""
    return torch.randint(0, SPS, (B, H // 8, W // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)


def bench_step(args, dev):
    from openess_amd.training.pretrain_step import PretrainStep
    B, H, W, nwin = args.batch, args.height, args.width, args.nwin
    g = torch.Generator().manual_seed(7)
    ev = (torch.randn(B, nwin * BINS, H, W, generator=g) * (torch.rand(B, nwin * BINS, H, W, generator=g) > 0.7)).to(dev)
    frame = torch.rand(B, 3, H, W, generator=g).to(dev)
    pl = torch.randint(0, K, (B, H, W), generator=g).to(dev)
    sp = _superpixels(B, H, W, g)
    S = int((sp + torch.arange(B)[:, None, None] * SPS).max()) + 1
    batch = (ev, None, frame, pl, sp.to(dev), S)
    steps = {p: PretrainStep(config_option='frame2voxel', img_size=(H, W), nr_events_data=nwin, nr_temporal_bins=BINS,
                             if_spatial_contrastive=True, superpixel_size=SPS, device=dev, precision=p) for p in ('bf16', 'fp32')}
    losses = {}

    def run(p):
        losses[p] = float(steps[p].train_step(batch)[2])
    ms = _interleaved({p: (lambda p=p: run(p)) for p in steps}, args.steps, args.warmup)
    return {'bf16_ms': ms['bf16'], 'fp32_ms': ms['fp32'], 'fp32_over_bf16': ms['fp32'] / ms['bf16'], 'last_loss': losses}


def bench_node(args, dev):
    from openess_amd import hip
    B, C, H, W = args.batch, 256, args.height // 4, args.width // 4
    Ho, Wo = 4 * H, 4 * W
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, C, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    sp = _superpixels(B, Ho, Wo, g).to(dev)
    S = B * SPS
    gk = torch.randn(S, C, generator=g).to(dev)

    def fused():
        x.grad = None
        hip.UpsampledNormalizedFeature(x, 4).pool(sp, SPS, S).backward(gk)

    def materialised():
        x.grad = None
        hip.superpixel_pool(hip.UpsampledNormalizedFeature(x, 4).materialize(), sp, SPS, S).backward(gk)
    ms = _interleaved({'fused': fused, 'materialised': materialised}, args.steps, args.warmup)
    full = B * C * Ho * Wo * 4
    xb, tmp, ids = full // 16, full // 4, B * Ho * Wo * 8
    nbytes = {'materialised': 9 * full + 2 * tmp + xb, 'fused': 3 * xb + 2 * ids + 2 * tmp}
    return {'fused_ms': ms['fused'], 'materialised_ms': ms['materialised'], 'speedup': ms['materialised'] / ms['fused'],
            'derived_bytes': nbytes, 'derived_byte_ratio': nbytes['materialised'] / nbytes['fused'],
            'fused_gbps_of_derived': nbytes['fused'] / ms['fused'] / 1e6, 'materialised_gbps_of_derived': nbytes['materialised'] / ms['materialised'] / 1e6}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=440)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--nwin", type=int, default=20)
    ap.add_argument("--parts", default="node,step", help="comma list of node, step")
    args = ap.parse_args(argv)
    if args.height % 8 or args.width % 8 or args.steps < 1 or args.warmup < 0:
        ap.error("height and width must be multiples of 8, steps >= 1, warmup >= 0")
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_pretrain_fp32.py needs the GPU")
    dev = torch.device('cuda', torch.cuda.current_device())
    parts = args.parts.split(',')
    if not parts or set(parts) - {'node', 'step'}:
        ap.error("--parts takes node and / or step")
    out = {'size': [args.batch, args.height, args.width], 'nwin': args.nwin, 'steps': args.steps, 'warmup': args.warmup}
    if 'node' in parts:
        out['node'] = bench_node(args, dev)
    if 'step' in parts:
        out['step'] = bench_step(args, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
