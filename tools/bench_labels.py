"""K31: class labels from stride-level logits, fused (hip.argmax_labels) against composed (hip.bilinear_resize(...).argmax(1), the
path before K31), at the online teacher's geometry: 8 x {11, 19} x 28 x 40 -> 440 x 640, fp32 and bf16 logits.

    python tools/bench_labels.py [--iters 50] [--rounds 7] [--batch 8]

Per shape, interleaved rounds (HIP events around `iters` calls), median / best / worst of the rounds in us, and the peak bytes each
form allocates on top of its input (torch's allocator statistics); the labels of the two forms are compared with torch.equal
first.  Then the online-teacher half of PretrainStep.front both ways on a randomly initialised ViT-B/16 tower, fp32 and bf16:
tower(frame).argmax(dim=1) against tower.labels(frame).  One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openess_amd import hip  # noqa: E402

SHAPES = ((11, 28, 40), (19, 28, 40))
SIZE = (440, 640)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_labels.py measures on the GPU: none found")
    B = a.batch
    torch.manual_seed(0)
    res = {'batch': B, 'size': list(SIZE), 'unit': 'us', 'kernel': [], 'teacher_half': []}
    with torch.no_grad():
        for K, h, w in SHAPES:
            for dtype in (torch.float32, torch.bfloat16):
                x = torch.randn(B, h, w, K, device="cuda").to(dtype).permute(0, 3, 1, 2)       # NHWC, as the head leaves its logits

                def fused():
                    return hip.argmax_labels(x, size=SIZE)

                def composed():
                    return hip.bilinear_resize(x.float(), size=SIZE).argmax(1)

                assert torch.equal(fused(), composed())
                r = compare({'fused': fused, 'composed': composed}, a.rounds, a.iters)
                row = {'K': K, 'h': h, 'w': w, 'dtype': str(dtype).split('.')[-1], **r,
                       'label_bytes': B * SIZE[0] * SIZE[1] * 8, 'full_resolution_bytes': B * K * SIZE[0] * SIZE[1] * 4}
                res['kernel'].append(row)
                print(f"{B} x {K} x {h} x {w} {row['dtype']:8s}: fused {r['fused']['median']:7.1f} us ({r['fused']['best']:.1f} - "
                      f"{r['fused']['worst']:.1f}), peak {r['fused']['peak_bytes'] / 1e6:6.1f} MB   composed {r['composed']['median']:7.1f} us "
                      f"({r['composed']['best']:.1f} - {r['composed']['worst']:.1f}), peak {r['composed']['peak_bytes'] / 1e6:6.1f} MB", flush=True)
        from openess_amd.models.maskclip_model import maskClipFeatureExtractor
        tower = maskClipFeatureExtractor(text_categories=11).cuda().eval()
        frame = torch.rand(B, 3, *SIZE, device="cuda")
        for precision in ('bf16', 'fp32'):
            logits_form = tower.forward_fp32 if precision == 'fp32' else tower

            def with_logits():
                return logits_form(frame).argmax(dim=1)

            def with_labels():
                return tower.labels(frame, precision=precision)

            assert torch.equal(with_logits(), with_labels())
            r = compare({'online_labels': with_labels, 'online_teacher': with_logits}, a.rounds, max(2, a.iters // 5))
            res['teacher_half'].append({'precision': precision, 'K': 11, **r})
            print(f"online-teacher half of front, {precision}: online_labels {r['online_labels']['median']:8.1f} us "
                  f"({r['online_labels']['best']:.1f} - {r['online_labels']['worst']:.1f})   online_teacher(...).argmax "
                  f"{r['online_teacher']['median']:8.1f} us ({r['online_teacher']['best']:.1f} - {r['online_teacher']['worst']:.1f})",
                  flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
