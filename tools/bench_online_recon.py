#!/usr/bin/env python3
"""`recon_sources: online_e2vid` at the training size: 8 x 440 x 640, 20 sub-windows of 100 000 events, 5 bins.

  parts_ms        ms per batch of the online source by part, each timed alone with HIP events around --iters back-to-back calls:
                  voxelizer (with the H2D copies of the pinned event columns) | encoder loop (sub-windows 0 .. 18, latents
                  dropped) | decoder (sub-window 19 with reconstruct=True: its encoder pass, residual blocks, decoders,
                  prediction; timed as the whole sequence minus the encoder loop) | post-process (PostProcessor.process_u8) |
                  augment (hip.recon_augment with every augmentation on, and with everything off)
  augment_gbps    algorithmic bytes of the augment kernel (1 B read + 12 B written per pixel) over its time
  step_ms         the frame2recon pre-training step (PretrainStep, contrastive) with the PNG-shaped resident input in slot 2
                  and with the online source producing slot 2 of step i + 1 on a side stream under step i, interleaved in one
                  process (--rounds blocks of --steps steps each, medians), and their ratio

    python tools/bench_online_recon.py [--iters 10] [--warmup 3] [--steps 6] [--rounds 3] [--precision bf16]
Prints one JSON line.  No figure from it is asserted in a test."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openess_amd import hip  # noqa: E402
from openess_amd.datasets import _synth  # noqa: E402
from openess_amd.DSEC.dataset.sequence_ov import voxelize_raw_batch  # noqa: E402
from openess_amd.e2vid.image_reconstructor import ImageReconstructor, PostProcessor  # noqa: E402
from openess_amd.e2vid.run_reconstruction import load_model  # noqa: E402
from openess_amd.training.base_trainer_ov import online_recon_image  # noqa: E402

B, H_SENSOR, W, CROP, NWIN, NEV, C = 8, 480, 640, 40, 20, 100000, 5
H = H_SENSOR - CROP


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


def events(device):
    cols = {k: [] for k in 'xytp'}
    for b in range(B):
        for k, v in zip('xytp', _synth.dsec_raw_events(NWIN * NEV, H_SENSOR, W, seed=1205 + b)):
            cols[k].append(torch.from_numpy(v))
    ev = {k: torch.cat(v).pin_memory() for k, v in cols.items()}
    ev['seg_offsets'] = torch.arange(B * NWIN + 1, dtype=torch.int64) * NEV
    ev['flip'] = [False] * B
    return ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    ev = events(device)
    rmap = torch.from_numpy(_synth.rectify_map(H_SENSOR, W)[None]).to(device)
    model = load_model('random').to(device).eval()
    rec = ImageReconstructor(model, H, W, C, device, SimpleNamespace(precision=a.precision))
    post = PostProcessor(device)
    rng = np.random.default_rng(3)
    aug = {'flip': [int(i & 1) for i in range(B)], 'brightness': rng.uniform(0.8, 1.2, B).tolist(),
           'contrast': rng.uniform(0.8, 1.2, B).tolist(), 'noise_seed': rng.integers(1, 2 ** 62, B).tolist()}
    fp32 = a.precision == 'fp32'

    def voxelize():
        return voxelize_raw_batch(ev, device, rmap, C, H_SENSOR, W, CROP, NWIN)
    vox = voxelize()

    def encoders():
        rec.last_states_for_each_channel = {'grayscale': None}
        for i in range(NWIN - 1):
            rec.update_reconstruction(vox, channel_slice=(i * C, C), **({'latents_only': True} if fp32 else {'need_latents': False}))

    state = {}
    res = {"metric": "online_recon_ms_per_batch", "shape": [B, H, W], "sub_windows": NWIN, "events_per_sub_window": NEV,
           "precision": a.precision, "iters": a.iters, "warmup": a.warmup, "parts_ms": {}}
    res["parts_ms"]["voxelizer"] = round(timed(voxelize, a.iters, a.warmup), 3)
    res["parts_ms"]["encoder_loop"] = round(timed(encoders, a.iters, a.warmup), 3)
    # the decoder call alone: whole sequence minus the encoder loop (the recurrent states are consumed by the call)
    def sequence():
        encoders()
        state['img'] = rec.update_reconstruction(vox, channel_slice=((NWIN - 1) * C, C), reconstruct=True)[0]
        rec.last_states_for_each_channel = {'grayscale': None}
    res["parts_ms"]["decoder"] = round(timed(sequence, a.iters, a.warmup) - res["parts_ms"]["encoder_loop"], 3)
    img = state['img'][:, :1]
    res["parts_ms"]["postprocess"] = round(timed(lambda: post.process_u8(img), a.iters * 5, a.warmup), 3)
    u8 = post.process_u8(img)
    out = torch.empty(B, 3, H, W, device=device)
    t_aug = timed(lambda: hip.recon_augment(u8, aug['flip'], aug['brightness'], aug['contrast'], aug['noise_seed'], out=out),
                  a.iters * 5, a.warmup)
    res["parts_ms"]["augment"] = round(t_aug, 4)
    res["augment_algorithmic_bytes"] = B * H * W * 13
    res["augment_gbps"] = round(B * H * W * 13 / (t_aug * 1e-3) / 1e9, 1)
    off = {'flip': [0] * B, 'brightness': [1.0] * B, 'contrast': [1.0] * B, 'noise_seed': [0] * B}
    t_off = timed(lambda: hip.recon_augment(u8, off['flip'], off['brightness'], off['contrast'], off['noise_seed'], out=out),
                  a.iters * 5, a.warmup)
    res["augment_all_off_ms"] = round(t_off, 4)
    res["augment_all_off_gbps"] = round(B * H * W * 13 / (t_off * 1e-3) / 1e9, 1)
    res["source_ms"] = round(timed(lambda: online_recon_image(rec, post, voxelize(), NWIN, C, aug), a.iters, a.warmup), 3)

    # ---- the frame2recon pre-training step: resident slot 2 against the online source on a side stream
    from openess_amd.training.pretrain_step import PretrainStep
    torch.manual_seed(1205)
    step = PretrainStep(config_option="frame2recon", img_size=(H, W), nr_events_data=NWIN, nr_temporal_bins=C,
                        if_spatial_contrastive=True, superpixel_size=100, device=device)
    frame = torch.rand(B, 3, H, W, device=device)
    resident = torch.rand(B, 3, H, W, device=device)
    pl = torch.randint(0, 11, (B, H, W), device=device)
    g = 10
    sp = ((torch.arange(H, device=device) * g // H)[:, None] * g + (torch.arange(W, device=device) * g // W)[None]).expand(B, H, W).contiguous()
    S = (B - 1) * 100 + g * g
    side = torch.cuda.Stream(device=device)

    def train(slot2):
        for opt in step.optimizers_dict.values():
            opt.zero_grad()
        t_loss, _, _ = step.task_train_step((frame, None, slot2, pl, sp, S))
        t_loss.backward()
        for opt in step.optimizers_dict.values():
            opt.step()

    def produce():
        with torch.cuda.stream(side):
            t = online_recon_image(rec, post, voxelize(), NWIN, C, aug)
            ready = torch.cuda.Event()
            ready.record(side)
        return t, ready

    def run_resident(n):
        for _ in range(n):
            train(resident)

    def run_online(n):
        side.wait_stream(torch.cuda.current_stream(device))
        nxt = produce()
        for i in range(n):
            t, ready = nxt
            torch.cuda.current_stream(device).wait_event(ready)
            t.record_stream(torch.cuda.current_stream(device))
            train(t)
            nxt = produce() if i + 1 < n else None
        torch.cuda.current_stream(device).wait_stream(side)

    def block(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(a.steps)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    run_resident(2), run_online(2)                   # warm-up of both (allocator, workspaces, packed weights)
    t_res, t_on = [], []
    for _ in range(a.rounds):
        t_res.append(block(run_resident))
        t_on.append(block(run_online))
    res["step_ms"] = {"resident": round(statistics.median(t_res), 2), "online": round(statistics.median(t_on), 2),
                      "resident_blocks": [round(v, 2) for v in t_res], "online_blocks": [round(v, 2) for v in t_on],
                      "steps_per_block": a.steps}
    res["step_ratio_online_over_resident"] = round(statistics.median(t_on) / statistics.median(t_res), 4)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
