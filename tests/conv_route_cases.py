"""Shared convolution dispatch cases: every row is a full call description of hip.conv2d_nhwc (or hip.convlstm_fused) plus
the kernel each of its call variants is MEANT to reach, by the OESS_ROUTE_* names of include/oess.h.
tests/test_conv_routes.py (no GPU) asserts the library's own dispatch plan agrees and that the table reaches every route the
library declares; tests/test_hip_conv_exact.py runs the same rows on the GPU, so a parity case cannot drift to another kernel
without the CPU test failing first.

Geometry is (B, H, W, Cin, Cout, R, stride, pad, dil) with S = R.  Sizes are the smallest the route's conditions allow, with the
edges that kernel tiles over: ragged last 128-row tile, tiles that cross image and batch borders, Cout % 8 == 4, R S Cin not a
multiple of 64, W smaller than a tile row, H = 1 / W = 1.  Only the two w128 rows and the 256-tile row are large: those rules need
ceil(M / 256) * Cout / 256 >= 2 x 256 CUs, or >= 400.

The w128 and 256-tile rows count tiles against the device's CU count: their routes hold for 256 CUs, which is the MI355X and
what the library assumes on a machine without a GPU; on another GPU those rows (and only those) would name another kernel.
The OESS_W128_* environment knobs also move them, so test_conv_routes.py clears them.

No route is unreachable: test_conv_routes.py requires the table to cover all of them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_routes():
    """{name: value} of the OESS_ROUTE_* kernel values of include/oess.h (without OESS_ROUTE_COUNT)."""
    txt = open(os.path.join(ROOT, "include", "oess.h")).read()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+OESS_ROUTE_([A-Z0-9_]+)\s+(\d+)\b", txt)}
    count = d.pop("COUNT")
    assert sorted(d.values()) == list(range(1, count + 1)), "OESS_ROUTE_* values must be 1 .. OESS_ROUTE_COUNT"
    return d


# Call variants.  in_extra / out_extra: the operand is a channel slice [8 : 8 + C] of a buffer that many channels wider (16-byte
# aligned, neighbours asserted untouched); res_extra: the residual is a channel slice [0 : Cout] of a wider buffer.
VARIANTS = {
    "plain": {},
    "bias_relu": dict(bias=True, relu=True),
    "f32": dict(bias=True, relu=True, out_f32=True),
    "res": dict(bias=True, relu=True, residual=True, res_extra=8),
    "slice": dict(bias=True, in_extra=16, out_extra=16),
    "stats": dict(tile_stats=True),
}


def c8(c):
    return (c + 7) // 8 * 8


def strides(geom, variant):
    """(in_pix_stride, out_pix_stride, res_pix_stride) of a variant's views, in elements."""
    Cin, Cout = geom[3], geom[4]
    a = VARIANTS[variant]
    return (Cin + a.get("in_extra", 0), c8(Cout) + a["out_extra"] if "out_extra" in a else Cout,
            c8(Cout) + a["res_extra"] if a.get("residual") else 0)


def _all(route, **other):
    d = {v: route for v in VARIANTS}
    d.update(other)
    return d


SK = lambda kind, ks: (kind, ks)      # split-K routes carry their slice count

# (name, geometry, {variant: route}, what the row is for)
ROUTE_CASES = [
    ("smallcin", (1, 9, 70, 8, 32, 5, 1, 2, 1),
     _all("SMALLCIN", f32="DMA32_SLOWK", res="DMA32_SLOWK", stats="DMA32_SLOWK"),
     "Cin = 8 stencil: ragged 8 x 64 patches; fp32 out / residual / statistics leave it for the general BN = 32 kernel"),
    ("smallcin_cout12", (2, 7, 9, 8, 12, 5, 1, 2, 1),
     _all("SMALLCIN", f32="DMA32_SLOWK", res="DMA32_SLOWK", stats="DMA32_SLOWK"),
     "Cout % 8 == 4, W smaller than a patch row, two images"),
    ("fallback128", (1, 5, 7, 4096, 136, 3, 1, 1, 1), _all("FALLBACK_128"),
     "K = 36864 >= 32768: the reciprocal tap decode does not apply; ragged second Cout tile"),
    ("fallback64", (1, 5, 7, 4096, 40, 3, 1, 1, 1), _all("FALLBACK_64"), "the same at BN = 64"),
    ("fallback32", (1, 5, 7, 4096, 12, 3, 1, 1, 1), _all("FALLBACK_32"), "the same at BN = 32, Cout % 8 == 4"),
    ("s2halo", (1, 9, 35, 32, 64, 5, 2, 2, 1),
     _all("S2_HALO", f32="DMA64_SLOWK", res="DMA64_SLOWK", stats="DMA64_SLOWK"),
     "5x5 stride 2: odd extents, ragged 8 x 16 patches, K = 800 (Kpad 832)"),
    ("s2halo_b2", (2, 10, 36, 32, 128, 5, 2, 2, 1),
     _all("S2_HALO", f32="DMA128_SLOWK", res="DMA128_SLOWK", stats="DMA128_SLOWK"),
     "even extents, two images, two 64-channel tiles"),
    ("ring_1x1", (1, 5, 7, 1024, 72, 1, 1, 0, 1), _all("SMALLMAP_RING"), "small-map 512-thread ring: one ragged tile, 16 slabs"),
    ("ring_1x1_b2", (2, 9, 11, 1024, 136, 1, 1, 0, 1), _all("SMALLMAP_RING"), "ragged M tile across a batch border, ragged Cout tile"),
    ("ring_3x3_valid", (1, 9, 11, 128, 132, 3, 1, 0, 1), _all("SMALLMAP_RING"), "3x3 without padding (not the row-halo form), 18 slabs"),
    ("w128_3x3", (2, 260, 254, 64, 256, 3, 1, 1, 1),
     _all("CONV3X3_W128", bias_relu="HALO3X3", f32="HALO3X3", res="HALO3X3", slice="HALO3X3"),
     "conv3x3_w128_kernel needs >= 512 tiles of 256 x 256 and a raw result; with a bias it falls back to the row-halo kernel. "
     "W = 254: 256-row tiles cross image rows; M = 132080 is ragged"),
    ("halo", (1, 9, 20, 64, 72, 3, 1, 1, 1), _all("HALO3X3"), "row-halo 3x3: W smaller than a tile row, ragged second M tile"),
    ("halo_b2", (2, 9, 10, 64, 132, 3, 1, 1, 1), _all("HALO3X3"), "a tile that crosses the batch border, ragged Cout tile"),
    ("halo_h1", (1, 1, 40, 64, 72, 3, 1, 1, 1), _all("HALO3X3"), "H = 1: every tap row but the centre is padding"),
    ("dma128_w1", (1, 40, 1, 64, 72, 3, 1, 1, 1), _all("DMA128_FASTK"), "W = 1: the row-halo rows do not fit, general kernel"),
    ("dma128_dil2", (3, 5, 4, 128, 256, 3, 1, 2, 2), _all("DMA128_FASTK"),
     "dilated 3x3 on a 5 x 4 map (every tap mostly padding): too many halo rows for the row-halo kernel"),
    ("splitk_ks5", (1, 15, 17, 256, 132, 3, 1, 1, 1), _all(SK("SPLITK_FASTK", 5), stats="HALO3X3"),
     "split-K, 36 slabs in 5 slices, M = 255 (ragged); with statistics the 64-row alternative is off and the row-halo kernel wins"),
    ("splitk_ks8", (2, 14, 20, 512, 256, 3, 1, 12, 12), _all(SK("SPLITK_FASTK", 8)), "ASPP class: dil 12 on a 14 x 20 map, 72 slabs in 8"),
    ("splitk_slowk_ks4", (1, 15, 17, 232, 132, 3, 1, 1, 1), _all(SK("SPLITK_SLOWK", 4)),
     "split-K with Cin % 64 != 0: K = 2088 (Kpad 2112), slabs straddle taps"),
    ("splitk_slowk_ks5", (1, 11, 23, 264, 76, 3, 1, 0, 1), _all(SK("SPLITK_SLOWK", 5)), "no padding, Cout % 8 == 4, K = 2376"),
    ("w128_1x1", (2, 257, 256, 256, 256, 1, 1, 0, 1), _all("CONV1X1_W128", f32="TILE256", res="TILE256"),
     "conv1x1_w128_kernel needs >= 512 tiles of 256 x 256; fp32 out / residual fall back to the 256 x 256 tile kernel. M = 131584"),
    ("tile256", (1, 320, 321, 256, 256, 1, 1, 0, 1), {"plain": "TILE256", "stats": "TILE256", "slice": "TILE256"},
     "402 tiles of 256 x 256 (>= 400, < 2 x CUs): the 256-tile kernel with statistics, whose rows 2t hold 256-row sums and rows "
     "2t + 1 are zero; M = 102720 leaves a 64-row last tile and an odd number (803) of statistics rows"),
    ("ring32", (1, 9, 20, 96, 72, 1, 1, 0, 1), _all("RING32"), "BK = 32 ring: K = 96 (Kpad 128), ragged M tile"),
    ("ring32_k32", (2, 9, 10, 32, 132, 1, 1, 0, 1), _all("RING32"), "a single 32-wide slab, batch border, ragged Cout tile"),
    ("ring32_2x2", (1, 9, 20, 64, 72, 2, 1, 0, 1), _all("RING32"), "2x2 taps through the BK = 32 ring"),
    ("tile64", (1, 16, 16, 320, 72, 1, 1, 0, 1), _all("TILE64_FASTK", stats="DMA128_FASTK"),
     "64-row tiles (M = 256: four half tiles beat two); statistics keep the 128-row kernel"),
    ("tile64_slowk", (1, 15, 17, 328, 132, 1, 1, 0, 1), _all("TILE64_SLOWK", stats="DMA128_SLOWK"), "Cin % 64 != 0, ragged last 64-row tile"),
    ("tile64_3x3_c24", (1, 15, 17, 24, 132, 3, 1, 1, 1), _all("TILE64_SLOWK", stats="DMA128_SLOWK"), "3x3 at Cin = 24: K = 216, three taps per slab"),
    ("dma128", (1, 9, 20, 320, 72, 1, 1, 0, 1), _all("DMA128_FASTK"), "general kernel BN = 128, fastk, ragged M tile"),
    ("dma128_slowk", (1, 9, 20, 328, 76, 1, 1, 0, 1), _all("DMA128_SLOWK"), "Cin % 64 != 0, Cout % 8 == 4"),
    ("dma128_s2", (2, 9, 10, 40, 132, 3, 2, 1, 1), _all("DMA128_SLOWK"), "3x3 stride 2 on odd / even extents, two images in one tile"),
    ("dma64", (1, 9, 20, 64, 40, 3, 1, 1, 1), _all("DMA64_FASTK"), "general kernel BN = 64 with fastk"),
    ("dma64_slowk", (2, 9, 10, 72, 36, 3, 1, 2, 2), _all("DMA64_SLOWK"), "dilated, Cout % 8 == 4, K = 648"),
    ("dma32", (1, 9, 20, 64, 12, 3, 1, 1, 1), _all("DMA32_FASTK"), "general kernel BN = 32 with fastk, Cout % 8 == 4"),
    ("dma32_slowk", (2, 9, 10, 72, 8, 3, 2, 0, 1), _all("DMA32_SLOWK"), "stride 2 without padding"),
    ("dma32_tiny", (1, 1, 9, 64, 4, 1, 1, 0, 1), _all("DMA32_FASTK"), "H = 1, nine pixels, four channels"),
]

# ConvLSTM (hip.convlstm_fused): ((B, H, W, Cx + C), C, k, pad) -> route.  These rows are route assertions only; parity is
# tests/test_hip_convlstm.py's, which runs every one of these routes (and the grouped, w128 and unfused gate kernels) on exact
# cases whose gate epilogue saturates -- bit for bit -- and under a float64 bound (cases and their routes: tests/convlstm_cases.py).
LSTM_ROUTE_CASES = [
    ("lstm_halo", ((1, 9, 20, 128), 64, 3, 1), "HALO3X3_LSTM", "3x3, Cin % 64 == 0: row-halo kernel with the fused cell update"),
    ("lstm_5x5", ((1, 9, 20, 128), 64, 5, 2), "LSTM_FASTK", "5x5 gates: general kernel with the fused cell update"),
    ("lstm_c96", ((2, 9, 10, 96), 32, 3, 1), "LSTM_SLOWK", "Cin % 64 != 0"),
]


def route_value(routes, r):
    return routes[r[0]] | r[1] << 8 if isinstance(r, tuple) else routes[r]
