"""K39: the fused ensemble render (hip.ensemble_render: labels + confidence + blended colour from the mean class probability of V
logit maps) against the same outputs composed from existing ops -- per view hip.bilinear_resize(x.float(), size) -> softmax(1) ->
flip, then mean -> max(1) -> palette gather -> torch blend -- at 8 x {11, 19} -> 440 x 640 with V = 2 (28 x 40 and its mirror
image) and V = 6 (21 x 30, 28 x 40, 35 x 50, each with its mirror image) in fp32 and bf16, and the same-size V = 2 at
8 x 11 x 440 x 640; then Segmenter.predict with and without flip=True for frame2recon and for the event student at 440 x 640.

    python tools/bench_tta.py [--iters 20] [--rounds 7] [--batch 8] [--skip-networks]

Per case, interleaved rounds (HIP events around `iters` calls): median / best / worst of the rounds in us, the peak bytes each form
allocates on top of its inputs, and GB/s over the bytes the fused form writes (1 + 4 + 3 per pixel).  The two forms are compared
first: the confidences within 1e-5, the labels on all but near-ties.  One JSON line at the end."""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from openess_amd import hip  # noqa: E402
from bench_segment import SIZE, compare, settings_440x640  # noqa: E402  (the project's protocol: interleaved rounds, medians)

LOW = ((28, 40),)
MULTI = ((21, 30), (28, 40), (35, 50))
# K, view sizes (each with its mirror image), label
CASES = ((11, LOW, "V=2"), (19, LOW, "V=2"), (11, MULTI, "V=6"), (19, MULTI, "V=6"), (11, (SIZE,), "V=2 same size"))


def composed_render(views, flips, size, palette, grey, alpha256):
    p = 0
    for x, f in zip(views, flips):
        v = x.float() if tuple(x.shape[-2:]) == tuple(size) else hip.bilinear_resize(x.float(), size=size)
        q = v.softmax(1)
        p = p + (q.flip(-1) if f else q)
    conf, labels = (p / len(views)).max(1)
    c = palette[labels].int()
    rgb = ((alpha256 * c + (256 - alpha256) * grey[..., None].int() + 128) >> 8).to(torch.uint8)
    return {'labels': labels.to(torch.uint8), 'conf': conf, 'rgb': rgb}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--skip-networks", action="store_true", help="the kernel comparison only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta.py measures on the GPU: none found")
    B = a.batch
    torch.manual_seed(0)
    res = {'batch': B, 'size': list(SIZE), 'unit': 'us', 'kernel': [], 'device': torch.cuda.get_device_name(0)}
    written = B * SIZE[0] * SIZE[1] * 8
    with torch.no_grad():
        for K, sizes, label in CASES:
            for dtype in (torch.float32, torch.bfloat16):
                views, flips = [], []
                for h, w in sizes:
                    for f in (False, True):
                        views.append((torch.randn(B, h, w, K, device="cuda") * 3).to(dtype).permute(0, 3, 1, 2))      # NHWC
                        flips.append(f)
                palette = torch.randint(0, 256, (K, 3), device="cuda").to(torch.uint8)
                grey = torch.randint(0, 256, (B, *SIZE), device="cuda").to(torch.uint8)

                def fused():
                    return hip.ensemble_render(views, flips=flips, size=SIZE, palette=palette, background=grey, alpha=0.5)

                def composed():
                    return composed_render(views, flips, SIZE, palette, grey, 128)

                f, c = fused(), composed()
                dev = float((f['conf'] - c['conf']).abs().max())
                agree = f['labels'] == c['labels']
                assert dev <= 1e-5 and float(agree.float().mean()) > 0.999 and torch.equal(f['rgb'][agree], c['rgb'][agree])
                del f, c, agree
                r = compare({'fused': fused, 'composed': composed}, a.rounds, a.iters)
                row = {'K': K, 'views': [list(s) for s in sizes for _ in (0, 1)], 'V': len(views), 'same_size': sizes[0] == SIZE,
                       'dtype': str(dtype).split('.')[-1], **r, 'written_bytes': written,
                       'fused_GBps': written / r['fused']['median'] / 1e3, 'conf_max_abs_diff_to_composed': dev}
                res['kernel'].append(row)
                print(f"{B} x {K} {label:14s} {row['dtype']:8s}: fused {r['fused']['median']:8.1f} us ({r['fused']['best']:.1f} - "
                      f"{r['fused']['worst']:.1f}), {row['fused_GBps']:6.1f} GB/s written, peak {r['fused']['peak_bytes'] / 1e6:6.1f} MB   "
                      f"composed {r['composed']['median']:8.1f} us ({r['composed']['best']:.1f} - {r['composed']['worst']:.1f}), "
                      f"peak {r['composed']['peak_bytes'] / 1e6:7.1f} MB", flush=True)
                del views, grey
        if not a.skip_networks:
            from openess_amd.inference import Segmenter
            with tempfile.TemporaryDirectory() as folder:
                cfg = settings_440x640(folder, B)
                seg = Segmenter(cfg, 'frame2recon', ckpt_dir=folder)
                batch = (None, None, torch.rand(B, 3, *SIZE, device="cuda"))
                r = compare({'plain': lambda: seg.predict(batch)['labels'], 'flip': lambda: seg.predict(batch, flip=True)['labels']},
                            a.rounds, max(2, a.iters // 5))
                res['frame2recon'] = {'precision': 'bf16', **r}
                print(f"frame2recon bf16 {B} x 3 x 440 x 640: predict {r['plain']['median'] / 1e3:7.2f} ms, peak "
                      f"{r['plain']['peak_bytes'] / 1e6:7.1f} MB   predict(flip=True) {r['flip']['median'] / 1e3:7.2f} ms, peak "
                      f"{r['flip']['peak_bytes'] / 1e6:7.1f} MB", flush=True)
                del seg, batch
                seg = Segmenter(cfg, 'frame2voxel', ckpt_dir=folder)
                n, C = seg.settings.nr_events_data_b, seg.settings.input_channels_b
                ev = (torch.randn(1, n * C, *SIZE, device="cuda") * (torch.rand(1, n * C, *SIZE, device="cuda") > 0.7)).contiguous()
                r = compare({'plain': lambda: seg.predict_events(ev)['labels'], 'flip': lambda: seg.predict_events(ev, flip=True)['labels']},
                            a.rounds, max(2, a.iters // 5))
                res['event_student'] = {'precision': 'bf16', 'windows_per_frame': n, **r}
                print(f"frame2voxel bf16 1 x 440 x 640 ({n} windows a frame): predict_events {r['plain']['median'] / 1e3:7.2f} ms   "
                      f"predict_events(flip=True) {r['flip']['median'] / 1e3:7.2f} ms", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
