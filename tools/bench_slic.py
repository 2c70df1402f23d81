"""hip.slic_superpixels at the workload's size: 8 x 3 x 440 x 640, n = 100, 10 rounds.  HIP events, the median of
interleaved rounds (whole call | whole call with the connectivity pass | Lab pass | one assignment | one update | the
connectivity pass alone on the whole call's labels), the Lab pass's GB/s over its 24 bytes per pixel, and the connectivity pass's
five phases (events between its launches, a run of their own after the timed rounds).

    python tools/bench_slic.py [--batch 8] [--hw 440 640] [--segments 100] [--rounds 15]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hw", type=int, nargs=2, default=(440, 640))
    ap.add_argument("--segments", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=15)
    args = ap.parse_args(argv)
    import torch
    from openess_amd import hip
    B, (H, W), n = args.batch, args.hw, args.segments
    torch.manual_seed(0)
    small = torch.rand(B, 3, H // 8 + 1, W // 8 + 1, device='cuda')
    x = torch.nn.functional.interpolate(small, size=(H, W), mode='bilinear') + 0.05 * torch.rand(B, 3, H, W, device='cuda')
    x = x.clamp_(0, 1).contiguous()
    ny, nx, step = hip.slic_lattice(H, W, n)
    lab, cen = hip.slic_lab(x, lattice=(ny, nx))
    labels = hip.slic_assign(lab, cen, None, step, lattice=(ny, nx))
    final = hip.slic_superpixels(x, n)
    min_size, max_size, bound = hip.slic_connectivity_sizes(H, W, ny * nx)
    parts = {'whole': lambda: hip.slic_superpixels(x, n), 'whole_connected': lambda: hip.slic_superpixels(x, n, enforce_connectivity=True),
             'lab': lambda: hip.slic_lab(x, lattice=(ny, nx)),
             'assign': lambda: hip.slic_assign(lab, cen, labels, step), 'update': lambda: hip.slic_update(lab, labels, cen),
             'connectivity': lambda: hip.slic_enforce_connectivity(final, min_size)}
    for f in parts.values():
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in parts}
    for _ in range(args.rounds):
        for k, f in parts.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in times.items()}
    phases = [hip.slic_connectivity_phase_ms(final, min_size) for _ in range(args.rounds)]
    connected, kept = hip.slic_enforce_connectivity(final, min_size, return_counts=True)
    out = {'shape': [B, 3, H, W], 'segments': n, 'centres': ny * nx, 'step': step, 'ms': {k: round(v, 4) for k, v in med.items()},
           'ms_min': {k: round(min(v), 4) for k, v in times.items()},
           'lab_GBps': round(B * H * W * 24 / (med['lab'] * 1e-3) / 1e9, 1),
           'connectivity': {'min_size': min_size, 'max_size': max_size, 'bound': bound, 'kept_per_sample': kept.tolist(),
                            'pixels_relabelled': int((connected != final).sum()),
                            'ms_minus_whole': round(med['whole_connected'] - med['whole'], 4),
                            'phase_ms': {k: round(statistics.median(p[k] for p in phases), 4) for k in phases[0]}}}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
