"""K36: the fused head + render (hip.vocab_render: the composed linear head, the per-class maximum over its names, labels +
confidence + colour, in one pass over the 32-channel map) at 8 x 32 x 440 x 640 bf16 and P in {11, 36, 128} names against
  conv_grouped   the head as a convolution (engine.conv2d_infer, fp32 logits [B, P, H, W]) -> hip.segment_render(class_offsets=...)
  conv_torch     the same convolution -> torch amax per class -> softmax -> max -> palette gather
and the grouped upsampling render at 8 x 36 x 28 x 40 -> 440 x 640 (frame2recon's path) against hip.bilinear_resize -> torch.

    python tools/bench_vocab.py [--iters 30] [--rounds 7] [--batch 8]

Interleaved rounds (HIP events around `iters` calls): median / best / worst of the rounds in us, the peak bytes each form allocates
on top of its input, and GB/s over the bytes the fused pass moves (2 C read + 8 written per pixel).  The labels of the forms are
compared first (the convolution runs bf16 weights, the fused head fp32 ones: the agreement is reported, not asserted).  One JSON line
at the end."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from openess_amd import engine, hip  # noqa: E402
from bench_segment import compare  # noqa: E402

SIZE, C = (440, 640), 32
NAMES = (11, 36, 128)
SIZES_36 = [1, 2, 1, 5, 3, 1, 1, 5, 13, 1, 3]            # the reference's pseudo-label writer: 36 names in 11 classes


def offsets_for(P):
    if P == 36:
        sizes = SIZES_36
    elif P == 11:
        sizes = [1] * 11
    else:
        sizes = [P // 32] * 32                            # 128 names: 32 classes of four
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + n)
    return offs


def group_amax(v, offs):
    return torch.stack([v[:, a:b].amax(1) for a, b in zip(offs[:-1], offs[1:])], 1)


def torch_render(v, offs, palette):
    conf, labels = group_amax(v, offs).softmax(1).max(1)
    return {'labels': labels.to(torch.uint8), 'conf': conf, 'rgb': palette[labels]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vocab.py measures on the GPU: none found")
    B = a.batch
    torch.manual_seed(0)
    res = {'batch': B, 'size': list(SIZE), 'channels': C, 'unit': 'us', 'head': [], 'device': torch.cuda.get_device_name(0)}
    moved = B * SIZE[0] * SIZE[1] * (2 * C + 8)
    with torch.no_grad():
        x = torch.randn(B, *SIZE, C, device="cuda").to(torch.bfloat16).permute(0, 3, 1, 2)       # NHWC, as decoder_scale_4 leaves it
        for P in NAMES:
            offs = offsets_for(P)
            K = len(offs) - 1
            w, b = 0.3 * torch.randn(P, C, device="cuda"), torch.randn(P, device="cuda")
            palette = torch.randint(0, 256, (K, 3), device="cuda").to(torch.uint8)
            pw = engine.PackedWeight().get(w[:, :, None, None], b, None, cin_pad=C)
            grouped = None if K == P else offs

            def fused():
                return hip.vocab_render(x, w, b, class_offsets=grouped, palette=palette)

            def conv_grouped():
                return hip.segment_render(engine.conv2d_infer(x, pw, P, 1, out_f32=True), palette=palette, class_offsets=offs)

            def conv_torch():
                return torch_render(engine.conv2d_infer(x, pw, P, 1, out_f32=True), offs, palette)

            f, g, t = fused(), conv_grouped(), conv_torch()
            agree = {'conv_grouped': float((f['labels'] == g['labels']).float().mean()),
                     'conv_torch': float((f['labels'] == t['labels']).float().mean())}
            assert torch.equal(g['labels'], t['labels'])                   # the same logits: the same labels
            del f, g, t
            r = compare({'fused': fused, 'conv_grouped': conv_grouped, 'conv_torch': conv_torch}, a.rounds, a.iters)
            r['fused']['GBps'] = moved / r['fused']['median'] * 1e-3
            rec = {'names': P, 'classes': K, 'label_agreement_with_fused': agree, 'logit_tensor_bytes': B * P * SIZE[0] * SIZE[1] * 4, **r}
            res['head'].append(rec)
            print(f"[bench_vocab] P={P} K={K}: " + ", ".join(f"{k} {v['median']:.1f} us (peak {v['peak_bytes']})" for k, v in r.items())
                  + f"; fused {r['fused']['GBps']:.0f} GB/s; agreement {agree}", flush=True)
        # frame2recon: stride-level logits of 36 names -> 440 x 640
        offs = offsets_for(36)
        low = (torch.randn(B, 28, 40, 36, device="cuda") * 3).permute(0, 3, 1, 2)
        palette = torch.randint(0, 256, (11, 3), device="cuda").to(torch.uint8)

        def up_fused():
            return hip.segment_render(low, size=SIZE, palette=palette, class_offsets=offs)

        def up_torch():
            return torch_render(hip.bilinear_resize(low, size=SIZE), offs, palette)

        assert torch.equal(up_fused()['labels'], up_torch()['labels'])
        r = compare({'fused': up_fused, 'resize_torch': up_torch}, a.rounds, a.iters)
        r['fused']['GBps_written'] = B * SIZE[0] * SIZE[1] * 8 / r['fused']['median'] * 1e-3
        res['upsampling'] = {'names': 36, 'classes': 11, 'from': [28, 40], **r}
        print("[bench_vocab] 8 x 36 x 28 x 40 -> 440 x 640: " + ", ".join(f"{k} {v['median']:.1f} us (peak {v['peak_bytes']})" for k, v in r.items()),
              flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
