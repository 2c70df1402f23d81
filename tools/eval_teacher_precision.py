#!/usr/bin/env python3
"""What bf16 storage does to the pretraining target: the same frames through the bf16 image teacher (DilationFeatureExtractor.
forward, the training path) and the fp32 one (forward_fp32, the reference's arithmetic), seeded random weights
with damped residual branches (tests/synth.py) unless --chaotic, BatchNorm in train mode as the reference leaves it.  Each
precision runs on its own copy of the module, so the running statistics one run moves never reach the other.  Prints one JSON
line:
  pixel_cos_mean / pixel_cos_min        cosine between the two unit-norm feature vectors of a pixel
  superpixel_cos_mean / superpixel_cos_min   the same for the superpixel means (hip.segment_mean on fp32 features), the
                                        contrastive targets of stage 1
  rel_rms                               |bf16 - fp32|_rms / |fp32|_rms
  bf16_ms / fp32_ms                     milliseconds per batch (HIP events, median of the batches after --warmup)

    python tools/eval_teacher_precision.py [--batch 2] [--height 64] [--width 96] [--batches 2] [--warmup 1]"""
import argparse
import copy
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openess_amd import hip  # noqa: E402
from openess_amd.models.image_model import DilationFeatureExtractor  # noqa: E402
from tests.synth import damp_residual, fill_by_name  # noqa: E402


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    y = fn()
    e1.record()
    torch.cuda.synchronize()
    return y, e0.elapsed_time(e1)


def _cos(a, b, dim):
    return F.cosine_similarity(a.double(), b.double(), dim=dim)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=96)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--superpixel-size", type=int, default=25)
    ap.add_argument("--chaotic", action="store_true", help="plain random weights: rounding noise grows block by block")
    a = ap.parse_args(argv)
    if a.height % 8 or a.width % 8:
        ap.error("height and width must be multiples of 8 (the synthetic superpixels are 8 x 8 cells)")
    t = DilationFeatureExtractor(None)
    fill_by_name(t.encoder, 13)
    fill_by_name(t.decoder[0], 14)
    if not a.chaotic:
        damp_residual(t.encoder)
    t.cuda().train()
    nets = {"bf16": t, "fp32": copy.deepcopy(t)}              # separate running statistics
    gen = torch.Generator().manual_seed(a.height * 7 + a.width)
    B, H, W, sps = a.batch, a.height, a.width, a.superpixel_size
    acc = {k: [] for k in ("pix", "sp")}
    ms = {"bf16": [], "fp32": []}
    err2 = ref2 = 0.0
    with torch.no_grad():
        for i in range(a.warmup + a.batches):
            img = torch.rand(B, 3, H, W, generator=gen).cuda()
            sp = torch.randint(0, sps, (B, H // 8, W // 8), generator=gen).repeat_interleave(8, 1).repeat_interleave(8, 2).cuda()
            fb, tb = _timed(lambda: nets["bf16"](img))
            ff, tf = _timed(lambda: nets["fp32"].forward_fp32(img))
            if i < a.warmup:
                continue
            ms["bf16"].append(tb)
            ms["fp32"].append(tf)
            fb = fb.float()
            acc["pix"].append(_cos(fb, ff, 1).reshape(-1))
            S = B * sps
            kb, cnt = hip.superpixel_pool(fb, sp, sps, S, with_count=True)
            kf = hip.superpixel_pool(ff, sp, sps, S)
            acc["sp"].append(_cos(kb, kf, 1)[cnt > 0])
            err2 += float((fb.double() - ff.double()).pow(2).sum())
            ref2 += float(ff.double().pow(2).sum())
    pix, spc = torch.cat(acc["pix"]), torch.cat(acc["sp"])
    med = lambda v: round(sorted(v)[len(v) // 2], 3)          # noqa: E731
    res = {"metric": "teacher_bf16_vs_fp32", "size": f"{B}x3x{H}x{W}", "batches": a.batches, "weights": "chaotic" if a.chaotic else "damped",
           "pixel_cos_mean": float(pix.mean()), "pixel_cos_min": float(pix.min()),
           "superpixel_cos_mean": float(spc.mean()), "superpixel_cos_min": float(spc.min()), "superpixels": int(spc.numel()),
           "rel_rms": (err2 / ref2) ** 0.5, "bf16_ms": med(ms["bf16"]), "fp32_ms": med(ms["fp32"]),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
