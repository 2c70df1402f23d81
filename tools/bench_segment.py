"""K35: the fused segmentation render (hip.segment_render: labels + confidence + blended colour from stride-level logits) against
the same outputs composed from existing ops (hip.bilinear_resize(x.float(), size) -> softmax -> max -> palette gather -> torch
blend), at 8 x {11, 19} x 28 x 40 -> 440 x 640 in fp32 and bf16, and the same-size form at 8 x 11 x 440 x 640; then
Segmenter.predict for frame2recon against trainer.val_logits(...).argmax(1), and the frames per second of the event student at
440 x 640, stateless (nr_events_data windows per prediction) against stateful (one window per prediction).

    python tools/bench_segment.py [--iters 50] [--rounds 7] [--batch 8] [--skip-networks]

Per shape, interleaved rounds (HIP events around `iters` calls): median / best / worst of the rounds in us, the peak bytes each form
allocates on top of its input, and GB/s over the bytes the fused form writes (1 + 4 + 3 per pixel).  The labels and colours of the
two forms are compared with torch.equal first.  One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openess_amd import hip  # noqa: E402

SHAPES = ((11, 28, 40, (440, 640)), (19, 28, 40, (440, 640)), (11, 440, 640, None))
SIZE = (440, 640)
BASE = os.path.join(ROOT, "tests", "configs", "finetune_dsec_synthetic.yaml")


def timed(fn, iters):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us


def peak_bytes(fn):
    """largest allocation `fn` holds on top of what is live before it"""
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del r
    return peak


def summary(ts):
    return {'median': statistics.median(ts), 'best': min(ts), 'worst': max(ts)}


def compare(runs, rounds, iters):
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            times[k].append(timed(fn, iters))
    return {k: dict(summary(v), peak_bytes=peak_bytes(runs[k])) for k, v in times.items()}


def composed_render(x, size, palette, grey, alpha256):
    v = x.float() if size is None else hip.bilinear_resize(x.float(), size=size)
    conf, labels = v.softmax(1).max(1)
    c = palette[labels].int()
    rgb = ((alpha256 * c + (256 - alpha256) * grey[..., None].int() + 128) >> 8).to(torch.uint8)
    return {'labels': labels.to(torch.uint8), 'conf': conf, 'rgb': rgb}


def settings_440x640(folder, batch):
    cfg = yaml.load(open(BASE), yaml.Loader)
    cfg['dataset']['DSEC_events']['shape'] = list(SIZE)
    cfg['optim']['batch_size_b'] = batch
    path = os.path.join(folder, "segment_440x640.yaml")
    with open(path, "w") as f:
        f.write(yaml.dump(cfg))
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--skip-networks", action="store_true", help="the kernel comparison only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_segment.py measures on the GPU: none found")
    B = a.batch
    torch.manual_seed(0)
    res = {'batch': B, 'size': list(SIZE), 'unit': 'us', 'kernel': [], 'device': torch.cuda.get_device_name(0)}
    written = B * SIZE[0] * SIZE[1] * 8
    with torch.no_grad():
        for K, h, w, size in SHAPES:
            for dtype in (torch.float32, torch.bfloat16):
                x = (torch.randn(B, h, w, K, device="cuda") * 3).to(dtype).permute(0, 3, 1, 2)     # NHWC, as the heads leave their logits
                palette = torch.randint(0, 256, (K, 3), device="cuda").to(torch.uint8)
                grey = torch.randint(0, 256, (B, *SIZE), device="cuda").to(torch.uint8)

                def fused():
                    return hip.segment_render(x, size=size, palette=palette, background=grey, alpha=0.5)

                def composed():
                    return composed_render(x, size, palette, grey, 128)

                f, c = fused(), composed()
                v = x.float() if size is None else hip.bilinear_resize(x.float(), size=size)
                assert torch.equal(f['labels'].long(), v.argmax(1))
                # softmax(...).max's index may differ from the logits' argmax where two probabilities round to one float
                agree = f['labels'] == c['labels']
                assert float(agree.float().mean()) > 0.999 and torch.equal(f['rgb'][agree], c['rgb'][agree])
                dev = float((f['conf'] - c['conf']).abs().max())
                del f, c, v, agree
                r = compare({'fused': fused, 'composed': composed}, a.rounds, a.iters)
                row = {'K': K, 'h': h, 'w': w, 'same_size': size is None, 'dtype': str(dtype).split('.')[-1], **r,
                       'written_bytes': written, 'fused_GBps': written / r['fused']['median'] / 1e3,
                       'conf_max_abs_diff_to_composed': dev}
                res['kernel'].append(row)
                print(f"{B} x {K} x {h} x {w} {row['dtype']:8s}: fused {r['fused']['median']:7.1f} us ({r['fused']['best']:.1f} - "
                      f"{r['fused']['worst']:.1f}), {row['fused_GBps']:6.0f} GB/s written, peak {r['fused']['peak_bytes'] / 1e6:6.1f} MB   "
                      f"composed {r['composed']['median']:7.1f} us ({r['composed']['best']:.1f} - {r['composed']['worst']:.1f}), "
                      f"peak {r['composed']['peak_bytes'] / 1e6:6.1f} MB", flush=True)
        if not a.skip_networks:
            from openess_amd.inference import Segmenter
            with tempfile.TemporaryDirectory() as folder:
                cfg = settings_440x640(folder, B)
                seg = Segmenter(cfg, 'frame2recon', ckpt_dir=folder)
                batch = (None, None, torch.rand(B, 3, *SIZE, device="cuda"))
                runs = {'predict': lambda: seg.predict(batch)['labels'],
                        'val_logits_argmax': lambda: seg.trainer.val_logits(batch, 'bf16').argmax(1)}
                assert torch.equal(runs['predict']().long(), runs['val_logits_argmax']())
                r = compare(runs, a.rounds, max(2, a.iters // 10))
                res['frame2recon'] = {'precision': 'bf16', **r}
                print(f"frame2recon bf16 {B} x 3 x 440 x 640: predict {r['predict']['median'] / 1e3:7.2f} ms, peak "
                      f"{r['predict']['peak_bytes'] / 1e6:7.1f} MB   val_logits(...).argmax(1) {r['val_logits_argmax']['median'] / 1e3:7.2f} ms, "
                      f"peak {r['val_logits_argmax']['peak_bytes'] / 1e6:7.1f} MB", flush=True)
                del seg, batch, runs
                seg = Segmenter(cfg, 'frame2voxel', ckpt_dir=folder)
                n, C = seg.settings.nr_events_data_b, seg.settings.input_channels_b
                ev = (torch.randn(1, n * C, *SIZE, device="cuda") * (torch.rand(1, n * C, *SIZE, device="cuda") > 0.7)).contiguous()
                one = ev[:, :C].contiguous()
                runs = {'stateless': lambda: seg.predict_events(ev)['labels'],
                        'stateful': lambda: seg.predict_events(one, stateful=True)['labels']}
                r = compare(runs, a.rounds, max(2, a.iters // 5))
                res['event_student'] = {'precision': 'bf16', 'windows_per_stateless_frame': n,
                                        **{k: dict(v, fps=1e6 / v['median']) for k, v in r.items()}}
                print(f"frame2voxel bf16 1 x 440 x 640: stateless ({n} windows a frame) {1e6 / r['stateless']['median']:6.1f} frames/s, "
                      f"stateful (1 window a frame) {1e6 / r['stateful']['median']:6.1f} frames/s", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
