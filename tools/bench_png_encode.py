#!/usr/bin/env python3
"""Time the GPU PNG encoder against Pillow on the same host, on the three kinds of map tools/segment.py writes:

    python tools/bench_png_encode.py [--batch 8] [--height 440] [--width 640] [--rounds 7] [--iters 20] [--seed 0]

  labels   11 classes in 20 x 20 blocks (u8)
  colours  the flat colour image of those labels (u8 x 3)
  overlay  the colours blended 50 % over Gaussian grey noise (--overlay recon)

Per kind and batch: µs of hip.png_encode_batch alone (device events around --iters calls), ms of hip.png_encode_files (encode,
sizes, copy of the used columns, bytes on the host), ms of the host path (device-to-host copy of the maps, then Pillow's
save into a BytesIO per map, default settings), and the file bytes of both.  --rounds interleaved rounds; medians with
best - worst.  Every GPU file is checked once against Pillow's decoder before anything is timed.  Prints one JSON line."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_maps(batch, H, W, seed):
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 11, (batch, (H + 19) // 20, (W + 19) // 20)).astype(np.uint8)
    labels = np.ascontiguousarray(cells.repeat(20, 1).repeat(20, 2)[:, :H, :W])
    palette = rng.integers(0, 256, (11, 3)).astype(np.uint8)
    colours = np.ascontiguousarray(palette[labels])
    grey = np.clip(rng.normal(128.0, 40.0, (batch, H, W)), 0, 255).astype(np.uint8)
    overlay = ((128 * colours.astype(np.int32) + 128 * grey[..., None].astype(np.int32) + 128) >> 8).astype(np.uint8)
    return {"labels": labels, "colours": colours, "overlay": np.ascontiguousarray(overlay)}


def summary(values, digits):
    return {"median": round(statistics.median(values), digits), "best": round(min(values), digits), "worst": round(max(values), digits)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=440)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    import torch
    from PIL import Image
    from openess_amd import hip
    if not torch.cuda.is_available():
        raise SystemExit("bench_png_encode needs a GPU")
    maps = make_maps(a.batch, a.height, a.width, a.seed)
    dev = {k: torch.from_numpy(v).cuda() for k, v in maps.items()}

    def pillow(t):
        host = t.cpu().numpy()
        sizes = []
        for m in host:
            buf = io.BytesIO()
            Image.fromarray(m).save(buf, format="PNG")
            sizes.append(buf.tell())
        return sizes

    out = {"metric": "png_encode", "batch": a.batch, "height": a.height, "width": a.width, "rounds": a.rounds, "iters": a.iters,
           "device": torch.cuda.get_device_name(0), "maps": {}}
    bytes_gpu, bytes_host = {}, {}
    for k, t in dev.items():                                  # warm-up and one check of every file
        files = hip.png_encode_files(t)
        for f, m in zip(files, maps[k]):
            with Image.open(io.BytesIO(f)) as im:
                assert np.array_equal(np.asarray(im), m), k
        bytes_gpu[k] = [len(f) for f in files]
        bytes_host[k] = pillow(t)
    times = {k: {"encode_us": [], "files_ms": [], "pillow_ms": []} for k in dev}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for k, t in dev.items():
            buf = hip.png_encode_batch(t)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.iters):
                hip.png_encode_batch(t, out=buf)
            e1.record()
            torch.cuda.synchronize()
            times[k]["encode_us"].append(1e3 * e0.elapsed_time(e1) / a.iters)
            t0 = time.perf_counter()
            hip.png_encode_files(t)
            times[k]["files_ms"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            pillow(t)
            times[k]["pillow_ms"].append(1e3 * (time.perf_counter() - t0))
    for k in dev:
        out["maps"][k] = {"encode_us_per_batch": summary(times[k]["encode_us"], 1), "files_ms_per_batch": summary(times[k]["files_ms"], 3),
                          "pillow_ms_per_batch": summary(times[k]["pillow_ms"], 3), "gpu_bytes_per_file": round(sum(bytes_gpu[k]) / a.batch),
                          "pillow_bytes_per_file": round(sum(bytes_host[k]) / a.batch)}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
