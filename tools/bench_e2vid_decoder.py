"""K30: the bf16 upsample-conv decoder of E2VID at the online reconstruction source's geometry (B = 8, 440 x 640: decoder inputs
256 @ 55 x 80, 128 @ 110 x 160, 64 @ 220 x 320).

    python tools/bench_e2vid_decoder.py [--iters 20] [--rounds 5] [--batch 8]

Per level, interleaved rounds, median and best (HIP events):
  kernel      oess_upsample_bilinear2x_sum_nhwc_bf16 alone, with the GB/s of its algorithmic bytes (2 reads of P C, 1 write of 4 P C)
  fused       UpsampleConvLayer.forward(x, skip): the kernel + the 5 x 5 conv (BatchNorm folded, ReLU fused)
  composed    the same layer from pieces that existed before: x + skip in torch (bf16), hip.bilinear_resize (bf16), the same conv
  transposed  TransposedConvLayer of the same channel counts on x + skip: zero insertion + the 5 x 5 conv
and the accuracy of the decoder input against torch fp32 on the same operands: one rounding (fused) against three (composed).
Then the decoder stack (three levels) of an upsample-conv model: bf16 forward against forward_f32.  One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openess_amd import engine, hip  # noqa: E402
from openess_amd.e2vid.model.submodules import TransposedConvLayer, UpsampleConvLayer  # noqa: E402

LEVELS = ((256, 55, 80), (128, 110, 160), (64, 220, 320))


def timed(fn, iters):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def summary(ts):
    return {'median': statistics.median(ts), 'best': min(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    B = a.batch
    dev = torch.device("cuda")
    torch.manual_seed(0)
    res = {'batch': B, 'levels': []}
    ups, xs, skips = [], [], []
    with torch.no_grad():
        for C, H, W in LEVELS:
            up = UpsampleConvLayer(C, C // 2, 5, padding=2, norm='BN').cuda().eval()
            tr = TransposedConvLayer(C, C // 2, 5, padding=2, norm='BN').cuda().eval()
            x = engine.from_nhwc((torch.randn(B, H, W, C, device=dev) * 0.5).bfloat16())
            skip = engine.from_nhwc((torch.randn(B, H, W, C, device=dev) * 0.5).bfloat16())
            ups.append(up), xs.append(x), skips.append(skip)
            out = torch.empty(B, 2 * H, 2 * W, C, dtype=torch.bfloat16, device=dev)
            c = up.conv2d
            pw = up._pw.get(c.weight, c.bias, up.bn)

            def kernel():
                hip.upsample2x_sum_nhwc(engine.nhwc(x), engine.nhwc(skip), out=out)

            def fused():
                up(x, skip=skip)

            def composed_input():
                return engine.nhwc(hip.bilinear_resize(x + skip, scale_factor=2))

            def composed():
                hip.conv2d_nhwc(composed_input(), pw.packed, pw.bias, C // 2, 5, 5, 1, 2, 1, relu=True)

            def transposed():
                tr(x + skip)

            runs = {'kernel': kernel, 'fused': fused, 'composed': composed, 'transposed': transposed}
            times = {k: [] for k in runs}
            for _ in range(a.rounds):
                for k, fn in runs.items():
                    times[k].append(timed(fn, a.iters))
            P = B * H * W
            nbytes = (2 * P * C + 4 * P * C) * 2
            lv = {'C': C, 'H': H, 'W': W, 'ms': {k: summary(v) for k, v in times.items()}, 'kernel_bytes': nbytes,
                  'kernel_gbps': nbytes / statistics.median(times['kernel']) / 1e6}
            # accuracy of the decoder input: one rounding against three, on the same operands
            ref = F.interpolate(x.float() + skip.float(), scale_factor=2, mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
            kernel()
            e1, e3 = (out.float() - ref).abs(), (composed_input().float() - ref).abs()
            lv['input_error'] = {'fused_max': float(e1.max()), 'fused_mean': float(e1.mean()), 'composed_max': float(e3.max()),
                                 'composed_mean': float(e3.mean())}
            res['levels'].append(lv)
            print(f"{C:3d} @ {H} x {W}: kernel {lv['ms']['kernel']['median'] * 1e3:7.1f} us ({lv['kernel_gbps']:6.0f} GB/s)   "
                  f"fused {lv['ms']['fused']['median'] * 1e3:7.1f} us   composed {lv['ms']['composed']['median'] * 1e3:7.1f} us   "
                  f"transposed {lv['ms']['transposed']['median'] * 1e3:7.1f} us   input error mean {e1.mean():.2e} (1 rounding) "
                  f"{e3.mean():.2e} (3 roundings)", flush=True)
            del out, ref, e1, e3

        # ---- the decoder stack: bf16 forward against forward_f32 on the same layers (level l's output feeds level l + 1)
        xs32 = [t.float() for t in xs]
        skips32 = [t.float() for t in skips]

        def stack_bf16():
            h = xs[0]
            for up, skip in zip(ups, skips):
                h = up(h, skip=skip)

        def stack_fp32():
            h = xs32[0]
            for up, skip in zip(ups, skips32):
                h = up.forward_f32(h, skip=skip)

        st = {'bf16': [], 'fp32': []}
        for _ in range(a.rounds):
            st['bf16'].append(timed(stack_bf16, max(2, a.iters // 4)))
            st['fp32'].append(timed(stack_fp32, max(2, a.iters // 4)))
        res['decoder_stack_ms'] = {k: summary(v) for k, v in st.items()}
        print(f"decoder stack: bf16 {res['decoder_stack_ms']['bf16']['median']:.3f} ms   fp32 {res['decoder_stack_ms']['fp32']['median']:.3f} ms",
              flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
