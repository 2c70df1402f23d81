"""K28: one ConvGRU level at BASELINE size (B = 8, 110 x 160, C = 128) and the per-window time of a ConvGRU E2VID model.

    python tools/bench_convgru.py [--iters 20] [--rounds 5] [--batch 8] [--windows 12]

Part 1, interleaved rounds (fused, unfused, gates alone, output alone), median and best per step:
  fused    ConvGRU.step: oess_convgru_gates_bf16 + oess_convgru_out_bf16 on the h | x | r*h buffer (two launches)
  unfused  the same step from hip.conv2d_nhwc (fp32 pre-activations) plus torch pointwise ops on a cat(x, h) and a cat(x, r*h)
           buffer; x is written into both once, outside the timed step (as an encoder conv would), the blend is in place
  gates / output alone, with the TFLOP/s of their convolutions (2 * P * 2C * 2C * 9 and 2 * P * C * 2C * 9 FLOP)
Part 2: ImageReconstructor.update_reconstruction per window (latents only, as the trainers call it) for the lightweight
  architecture with ConvGRU blocks next to the ConvLSTM one (skewed schedule and fused head included: what a user gets).
Prints one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openess_amd import engine, hip  # noqa: E402
from openess_amd.e2vid.image_reconstructor import ImageReconstructor  # noqa: E402
from openess_amd.e2vid.model.model import E2VID_LIGHTWEIGHT_CONFIG, E2VIDRecurrent  # noqa: E402
from openess_amd.e2vid.model.submodules import ConvGRU  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--windows", type=int, default=12)
    a = ap.parse_args()
    B, H, W, C = a.batch, 110, 160, 128
    dev = torch.device("cuda")
    torch.manual_seed(0)
    blk = ConvGRU(C, C, 3).cuda()
    st = blk.new_state(B, H, W, dev)
    buf = engine.nhwc(st['hxr'])
    buf.copy_(torch.randn(B, H, W, 3 * C, device=dev) * 0.5)
    st['h32'].copy_(buf[..., :C].float())
    st['fresh'] = False
    pa, pb = blk._packed('gates', False), blk._packed('out', False)
    # unfused: plain packings in the reference's channel order on a cat(x, h) buffer and a cat(x, r*h) one
    with torch.no_grad():
        wur = torch.cat([blk.update_gate.weight, blk.reset_gate.weight], 0)
        bur = torch.cat([blk.update_gate.bias, blk.reset_gate.bias]).float().contiguous()
        p_ur, p_o = hip.pack_conv_weight(wur), hip.pack_conv_weight(blk.out_gate.weight)
        b_o = blk.out_gate.bias.detach().float().contiguous()
    xh = torch.empty(B, H, W, 2 * C, dtype=torch.bfloat16, device=dev)
    xr = torch.empty(B, H, W, 2 * C, dtype=torch.bfloat16, device=dev)
    xh[..., :C] = buf[..., C:2 * C]
    xh[..., C:] = buf[..., :C]
    xr[..., :C] = xh[..., :C]
    h32 = st['h32'].clone()

    def fused():
        blk.step(st)

    def unfused():
        pre = hip.conv2d_nhwc(xh, p_ur, bur, 2 * C, 3, 3, 1, 1, 1, out_f32=True)
        u, r = torch.sigmoid(pre[..., :C]), torch.sigmoid(pre[..., C:])
        xr[..., C:] = (r * h32).bfloat16()
        o = torch.tanh(hip.conv2d_nhwc(xr, p_o, b_o, C, 3, 3, 1, 1, 1, out_f32=True))
        h32.mul_(1 - u).addcmul_(o, u)
        xh[..., C:] = h32.bfloat16()

    def gates():
        hip.convgru_gates(buf[..., :2 * C], pa.packed, pa.bias, st['h32'], st['u'], buf[..., 2 * C:], 3, 1)

    def output():
        hip.convgru_out(buf[..., C:], pb.packed, pb.bias, st['u'], st['h32'], buf[..., :C], 3, 1)

    runs = {'fused': fused, 'unfused': unfused, 'gates': gates, 'output': output}
    times = {k: [] for k in runs}
    with torch.no_grad():
        for _ in range(a.rounds):
            for k, fn in runs.items():
                times[k].append(timed(fn, a.iters))
    P = B * H * W
    flops = {'gates': 2.0 * P * 2 * C * 2 * C * 9, 'output': 2.0 * P * C * 2 * C * 9}
    res = {'level': [B, H, W, C], 'ms_per_step': {}, 'tflops': {}}
    for k in runs:
        med, best = statistics.median(times[k]), min(times[k])
        res['ms_per_step'][k] = {'median': med, 'best': best}
        line = f"{k:8s} {med * 1e3:8.1f} us median   best {best * 1e3:8.1f} us"
        if k in flops:
            res['tflops'][k] = flops[k] / med / 1e9
            line += f"   {res['tflops'][k]:7.1f} TFLOP/s"
        print(line, flush=True)

    # ---- part 2: per-window time of the whole front end, ConvGRU next to ConvLSTM
    Hs, Ws = 440, 640
    ev = (torch.randn(B, 5 * 4, Hs, Ws, device=dev) * (torch.rand(B, 5 * 4, Hs, Ws, device=dev) > 0.8)).contiguous()
    recs = {}
    for name in ('convlstm', 'convgru'):
        torch.manual_seed(1)
        m = E2VIDRecurrent(dict(E2VID_LIGHTWEIGHT_CONFIG, recurrent_block_type=name)).eval().cuda()
        recs[name] = ImageReconstructor(m, Hs, Ws, 5, dev)
    win = {k: [] for k in recs}

    def windows(rec):
        for i in range(a.windows):
            rec.update_reconstruction(ev, channel_slice=(5 * (i % 4), 5), need_latents=(i == a.windows - 1))

    for _ in range(a.rounds):
        for name, rec in recs.items():
            win[name].append(timed(lambda: windows(rec), 2) / a.windows)
    res['ms_per_window'] = {'size': [B, Hs, Ws]}
    for name in recs:
        med, best = statistics.median(win[name]), min(win[name])
        res['ms_per_window'][name] = {'median': med, 'best': best}
        print(f"{name:8s} {med:8.3f} ms per window median   best {best:8.3f} ms", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
