#!/usr/bin/env python3
"""Every dispatch decision of the bf16 convolution family over a grid of calls, one line per call (no GPU):
    python tools/conv_route_sweep.py > new.txt;  OESS_LIB_PATH=/other/liboess.so python tools/conv_route_sweep.py > old.txt
Two builds of the same ABI dispatch alike iff the two files are byte-identical.  The pinned rows of tests/conv_route_cases.py are
the smallest case per route; this grid crosses the thresholds between them.  The last lines count the calls, the refusals and the
hits per route (stderr repeats them); fewer than OESS_ROUTE_COUNT routes seen is an error exit."""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
for _k in [k for k in os.environ if k.startswith("OESS_W128_")]:      # the A/B knobs of the w128 rules move routes
    del os.environ[_k]

from openess_amd import _lib, hip                      # noqa: E402
from tests import conv_route_cases as rc               # noqa: E402

BATCHES = (1, 8)
MAPS = ((1, 1), (9, 20), (28, 40), (55, 80), (110, 160), (220, 320), (440, 640))
CINS = (8, 32, 64, 96, 256, 1024, 2048)
COUTS = (4, 12, 32, 64, 72, 128, 256, 512, 2048)
FILTERS = ((1, 1, 0, 1), (3, 1, 1, 1), (3, 1, 4, 4), (3, 1, 8, 8), (3, 2, 1, 1), (5, 1, 2, 1), (5, 2, 2, 1))    # R, stride, pad, dil
LSTM_C, LSTM_CIN, LSTM_K = (32, 64, 96, 128, 256), (64, 96, 128, 512), (1, 3, 5)
# refused calls (the negative results are part of the output): (B, H, W, Cin), Cout, R, stride, pad, dil, keywords
BAD_CONV = (
    ((1, 9, 20, 12), 72, 1, 1, 0, 1, {}),                                        # Cin % 8
    ((0, 9, 20, 64), 72, 1, 1, 0, 1, {}),                                        # empty batch
    ((1, 2, 2, 64), 72, 5, 1, 0, 1, {}),                                         # filter larger than the map
    ((1, 9, 20, 64), 72, 3, 1, -1, 1, {}),
    ((1, 9, 20, 64), 72, 3, 1, 1, 0, {}),
    ((1, 9, 20, 64), 72, 3, 0, 1, 1, {}),
    ((1, 9, 20, 64), 72, 1, 1, 0, 1, dict(in_pix_stride=60)),                    # stride % 8, stride < Cin
    ((1, 9, 20, 64), 72, 1, 1, 0, 1, dict(in_pix_stride=56)),
    ((1, 9, 20, 64), 72, 1, 1, 0, 1, dict(out_pix_stride=76)),                   # bf16 rows of Cout % 8 == 0 need stride % 8 == 0
    ((1, 9, 20, 64), 72, 1, 1, 0, 1, dict(out_pix_stride=64)),
    ((1, 9, 20, 64), 72, 1, 1, 0, 1, dict(residual=True, res_pix_stride=76)),
    ((1, 9, 20, 64), 72, 1, 1, 0, 1, dict(residual=True, out_f32=True)),
    ((1, 9, 20, 64), 72, 1, 1, 0, 1, dict(tile_stats=True, bias=True)),
    ((1, 9, 20, 64), 72, 1, 1, 0, 1, dict(tile_stats=True, relu=True)),
    ((8, 20000, 20000, 8), 8, 1, 1, 0, 1, {}),                                   # M >= 2^31
)
BAD_LSTM = (                                                                     # (B, H, W, Cin), C, k, pad, keywords
    ((1, 9, 20, 128), 48, 3, 1, {}),                                             # C % 32
    ((1, 9, 20, 128), 0, 3, 1, {}),
    ((1, 9, 20, 128), 64, 3, 1, dict(hidden_pix_stride=65)),
    ((1, 9, 20, 128), 64, 3, 1, dict(hidden_pix_stride=32)),
    ((1, 9, 20, 128), 64, 3, 1, dict(in_pix_stride=1 << 23)),                    # beyond 32-bit buffer offsets: no fused kernel
    ((1, 9, 20, 100), 64, 3, 1, {}),
)


def main():
    lib = _lib.load()
    count = lib.oess_conv2d_route_count()
    seen, calls, refused = {}, 0, 0
    out = sys.stdout

    def line(tag, fn):
        nonlocal calls, refused
        calls += 1
        try:
            r = fn()
            seen[r & 0xff] = seen.get(r & 0xff, 0) + 1
            out.write(f"{tag} -> {r}\n")
        except Exception as e:                                                   # noqa: BLE001 (refusals are results)
            refused += 1
            out.write(f"{tag} -> refused: {type(e).__name__} {e}\n")

    for B, (H, W), Cin, Cout, (R, stride, pad, dil) in itertools.product(BATCHES, MAPS, CINS, COUTS, FILTERS):
        geom = (B, H, W, Cin, Cout, R, stride, pad, dil)
        for stats, f32 in ((0, 0), (1, 0), (0, 1)):
            ws = lib.oess_conv2d_fwd_workspace_bytes(B, H, W, Cin, Cout, R, R, stride, pad, dil, stats, f32)
            out.write(f"ws {geom} stats={stats} f32={f32} -> {ws}\n")
        for variant, a in rc.VARIANTS.items():
            ps_in, ps_out, ps_res = rc.strides(geom, variant)
            for splitk, aligned in itertools.product((True, False), (True, False)):
                line(f"conv {geom} {variant} splitk={int(splitk)} aligned={int(aligned)}",
                     lambda: hip.conv2d_route((B, H, W, Cin), None, a.get("bias", False), Cout, R, R, stride, pad, dil,
                                              relu=a.get("relu", False), residual=a.get("residual", False),
                                              out_f32=a.get("out_f32", False), tile_stats=a.get("tile_stats", False),
                                              allow_splitk=splitk, in_pix_stride=ps_in, out_pix_stride=ps_out,
                                              res_pix_stride=ps_res, out_aligned16=aligned))
    for B, (H, W), C, Cin, k in itertools.product(BATCHES, MAPS, LSTM_C, LSTM_CIN, LSTM_K):
        for extra in (0, 8):                                                     # cat(x, h) dense / a slice of a wider buffer
            line(f"lstm {(B, H, W, Cin)} C={C} k={k} in_extra={extra}",
                 lambda: hip.convlstm_route((B, H, W, Cin), C, k, k // 2, hidden_pix_stride=C + extra, in_pix_stride=Cin + extra))
    for shape, Cout, R, stride, pad, dil, kw in BAD_CONV:
        rest = {k: v for k, v in kw.items() if k != "bias"}
        line(f"bad conv {shape} {Cout} {R} {stride} {pad} {dil} {sorted(kw.items())}",
             lambda: hip.conv2d_route(shape, None, kw.get("bias", False), Cout, R, R, stride, pad, dil, **rest))
    for shape, C, k, pad, kw in BAD_LSTM:
        line(f"bad lstm {shape} C={C} k={k} {sorted(kw.items())}", lambda: hip.convlstm_route(shape, C, k, pad, **kw))
    tail = [f"calls {calls} refused {refused} routes seen {len(seen)} of {count}"]
    tail += [f"route {r:2d} {hip.conv2d_route_name(r)}: {n}" for r, n in sorted(seen.items())]
    out.write("\n".join(tail) + "\n")
    print("\n".join(tail), file=sys.stderr)
    return 0 if len(seen) == count else 1


if __name__ == "__main__":
    sys.exit(main())
