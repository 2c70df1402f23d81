#!/usr/bin/env python3
"""E2VID post-processing: the fused HIP pass (oess_e2vid_postprocess_*: one launch with fixed bounds, two with auto-HDR)
against the reference's torch composition (conv2d unsharp mask + intensity rescaling; auto-HDR adds two .item() host syncs), per call,
at 1 x 1 x 440 x 640 and 8 x 1 x 480 x 640, fixed bounds and auto-HDR, uint8 output (the PNG bytes; the torch path also makes its
fp32 byte / 255, as the reference does).  HIP events around --iters back-to-back calls after --warmup calls.  Prints one JSON line.

    python tools/bench_postprocess.py [--iters 200] [--warmup 20]
Launch counts: rocprofv3 --kernel-trace --stats -- python tools/bench_postprocess.py --iters 10 --warmup 0 --only-hip"""
import argparse
import json
import os
import sys
from collections import deque

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openess_amd.e2vid.image_reconstructor import PostProcessor  # noqa: E402
from openess_amd.e2vid.utils.inference_utils import gkern  # noqa: E402


class TorchPost:
    """UnsharpMaskFilter + IntensityRescaler of the reference (e2vid/utils/inference_utils.py:90-129, 234-252) as torch ops."""

    def __init__(self, auto):
        self.kernel = gkern(5, 1.0)[None, None].cuda()
        self.auto, self.bounds, self.Imin, self.Imax = auto, deque(), 0.0, 1.0

    def __call__(self, img):
        img = 1.3 * img - 0.3 * F.conv2d(img, self.kernel, padding=2)
        if self.auto:
            Imin, Imax = np.clip(torch.min(img).item(), 0.0, 0.45), np.clip(torch.max(img).item(), 0.55, 1.0)
            if len(self.bounds) > 10:
                self.bounds.popleft()
            self.bounds.append((Imin, Imax))
            self.Imin, self.Imax = np.median([b[0] for b in self.bounds]), np.median([b[1] for b in self.bounds])
        img = 255.0 * (img - self.Imin) / (self.Imax - self.Imin)
        img.clamp_(0.0, 255.0)
        return img.byte().float().div(255)


def time_calls(fn, x, iters, warmup):
    for _ in range(warmup):
        fn(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn(x)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only-hip", action="store_true", help="time the HIP path only (for a kernel trace)")
    a = ap.parse_args()
    torch.manual_seed(0)
    res = {"metric": "e2vid_postprocess_us_per_call", "iters": a.iters, "warmup": a.warmup, "cases": []}
    for shape in ((1, 1, 440, 640), (8, 1, 480, 640)):
        x = (0.1 + 0.8 * torch.rand(*shape)).cuda()
        for auto in (False, True):
            post = PostProcessor(torch.device("cuda"), argparse.Namespace(auto_hdr=auto))
            out = torch.empty(shape[0], shape[2], shape[3], dtype=torch.uint8, device="cuda")
            from openess_amd import hip
            kw = {"hdr_state": post.hdr_state} if auto else {"bounds": (0.0, 1.0)}
            hip_us = time_calls(lambda t: hip.e2vid_postprocess(t, post.gaussian_kernel, 0.3, out_u8=out, **kw), x, a.iters, a.warmup)
            row = {"shape": list(shape), "mode": "auto_hdr" if auto else "fixed", "hip_us": round(hip_us, 2),
                   "algorithmic_bytes": int(np.prod(shape)) * 5}
            if not a.only_hip:
                row["torch_us"] = round(time_calls(TorchPost(auto), x, a.iters, a.warmup), 2)
                row["speedup"] = round(row["torch_us"] / hip_us, 2)
            res["cases"].append(row)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
