#!/usr/bin/env python3
"""EventPreprocessor's hot-pixel removal and flip inside the event kernels at the training size:
8 x 100 x 440 x 640 fp32 events (20 sub-windows of 5 bins, 901 MB), about 200 hot pixels.

  kernels_us      per kernel, without and with the options (`plain` / `pre`): the statistics of all 20 sub-windows in one launch
                  (+ its finalize launch), the NHWC8 bf16 re-layout of one sub-window, the fused events -> head -> encoder-0
                  kernel of one sub-window (the last two with the statistics formed beforehand).  HIP events around --iters
                  back-to-back launches; --rounds rounds with the variants interleaved; medians, and min .. max of the rounds.
  kernels_gbps    the event bytes the kernel reads (all 100 channels for the statistics, 5 for the others) over that time
  encoder_loop_ms ms per sub-window of the E2VID encoder loop (ImageReconstructor.update_reconstruction over the 20
                  sub-windows with the latents dropped: fused head + skewed schedule), without and with the options

    python tools/bench_event_pre.py [--iters 20] [--warmup 3] [--rounds 5] [--baseline-only]
--baseline-only measures the option-less variants alone (it then also runs on a tree that has no options: the comparison with
the parent commit).  Prints one JSON line.  No figure from it is asserted in a test."""
import argparse
import ctypes
import json
import os
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openess_amd import _lib, hip  # noqa: E402
from openess_amd.e2vid.image_reconstructor import ImageReconstructor  # noqa: E402
from openess_amd.e2vid.run_reconstruction import load_model  # noqa: E402

B, NWIN, C, H, W = 8, 20, 5, 440, 640
N_HOT = 200


def timed_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--baseline-only", action="store_true")
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    lib = _lib.load()
    gen = torch.Generator(device=device).manual_seed(1205)
    ev = torch.empty((B, NWIN * C, H, W), device=device)
    for b in range(B):                                       # (sample by sample: no second 901 MB temporary)
        ev[b] = torch.randn((NWIN * C, H, W), device=device, generator=gen) * (torch.rand((NWIN * C, H, W), device=device, generator=gen) < 0.3)
    rng = np.random.default_rng(7)
    rows = np.stack([rng.integers(0, W, N_HOT), rng.integers(0, H, N_HOT)], 1)
    variants = ["plain"]
    pre = cpre = None
    hot_file = None
    if not a.baseline_only:
        variants.append("pre")
        mask = torch.zeros((H, W), dtype=torch.uint8)
        mask[rows[:, 1], rows[:, 0]] = 1
        pre = hip.EventPre(mask.to(device), True)
        cpre = pre.bind(ev)
        import tempfile
        fd, hot_file = tempfile.mkstemp(prefix="hot_pixels_", suffix=".txt")
        os.close(fd)
        np.savetxt(hot_file, rows, fmt="%d", delimiter=",")
    model = load_model('random').to(device).eval()
    unet = model.unetrecurrent
    ph, pe = unet.head._packed(8), unet.encoders[0].conv._packed(32)
    st, ptr = hip._stream, hip._ptr
    stats_buf = torch.empty(lib.oess_masked_stats_doubles(NWIN), dtype=torch.float64, device=device)
    x8 = torch.empty((B, H, W, 8), dtype=torch.bfloat16, device=device)
    enc = torch.empty((B, H // 2, W // 2, 64), dtype=torch.bfloat16, device=device)
    c0 = 7 * C
    row = {}                                                 # the statistics row of sub-window 7, per variant

    def stats(v):
        if v == "pre":
            _lib.check(lib.oess_masked_stats_slices_pre_f32(ptr(ev), B, NWIN * C, C, NWIN, H, W, ctypes.byref(cpre), ptr(stats_buf), st()), "stats")
        else:
            _lib.check(lib.oess_masked_stats_slices_f32(ptr(ev), B, NWIN * C, C, NWIN, H * W, ptr(stats_buf), st()), "stats")

    def nhwc8(v):
        if v == "pre":
            _lib.check(lib.oess_event_slice_to_nhwc8_pre_bf16(ptr(ev), B, NWIN * C, c0, C, H, W, ctypes.byref(cpre), ptr(row[v]), 1, ptr(x8), st()), "nhwc8")
        else:
            _lib.check(lib.oess_event_slice_to_nhwc8_bf16(ptr(ev), B, NWIN * C, c0, C, H * W, ptr(row[v]), 1, ptr(x8), st()), "nhwc8")

    def head(v):
        if v == "pre":
            _lib.check(lib.oess_e2vid_events_head_enc0_pre_bf16(ptr(ev), B, NWIN * C, c0, C, H, W, ctypes.byref(cpre), ptr(row[v]), 1, ptr(ph.packed),
                                                                ptr(ph.bias), 1, ptr(pe.packed), ptr(pe.bias), 1, ptr(enc), 64, st()), "head")
        else:
            _lib.check(lib.oess_e2vid_events_head_enc0_bf16(ptr(ev), B, NWIN * C, c0, C, H, W, ptr(row[v]), 1, ptr(ph.packed), ptr(ph.bias), 1,
                                                            ptr(pe.packed), ptr(pe.bias), 1, ptr(enc), 64, st()), "head")

    for v in variants:
        stats(v)
        row[v] = stats_buf[4 * 7:4 * 8].clone()
    recs = {"plain": ImageReconstructor(model, H, W, C, device, SimpleNamespace())}
    if not a.baseline_only:
        recs["pre"] = ImageReconstructor(model, H, W, C, device, SimpleNamespace(hot_pixels_file=hot_file, flip=True))

    def loop(v):
        rec = recs[v]
        rec.last_states_for_each_channel = {'grayscale': None}
        for i in range(NWIN):
            rec.update_reconstruction(ev, channel_slice=(i * C, C), need_latents=False)

    kernels = {"stats_20_slices": (stats, B * NWIN * C * H * W * 4), "slice_to_nhwc8": (nhwc8, B * C * H * W * 4),
               "events_head_enc0": (head, B * C * H * W * 4)}
    samples = {k: {v: [] for v in variants} for k in list(kernels) + ["encoder_loop"]}
    for _ in range(a.rounds):
        for k, (fn, _) in kernels.items():
            for v in variants:
                samples[k][v].append(timed_us(lambda: fn(v), a.iters, a.warmup))
        for v in variants:
            samples["encoder_loop"][v].append(timed_us(lambda: loop(v), max(1, a.iters // 10), 1) / NWIN * 1e-3)
    if hot_file:
        os.remove(hot_file)
    med = lambda xs: statistics.median(xs)
    res = {"metric": "event_pre_kernels", "shape": [B, NWIN * C, H, W], "sub_windows": NWIN, "hot_pixels": int(N_HOT), "flip": True,
           "iters": a.iters, "warmup": a.warmup, "rounds": a.rounds, "kernels_us": {}, "kernels_us_min_max": {}, "kernels_gbps": {}}
    for k, (_, nbytes) in kernels.items():
        res["kernels_us"][k] = {v: round(med(samples[k][v]), 1) for v in variants}
        res["kernels_us_min_max"][k] = {v: [round(min(samples[k][v]), 1), round(max(samples[k][v]), 1)] for v in variants}
        res["kernels_gbps"][k] = {v: round(nbytes / (med(samples[k][v]) * 1e-6) / 1e9, 1) for v in variants}
    res["encoder_loop_ms_per_window"] = {v: round(med(samples["encoder_loop"][v]), 4) for v in variants}
    res["encoder_loop_ms_per_window_min_max"] = {v: [round(min(samples["encoder_loop"][v]), 4), round(max(samples["encoder_loop"][v]), 4)]
                                                 for v in variants}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
