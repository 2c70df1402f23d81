"""Dispatch coverage table of the bf16 weight gradient (oess_conv2d_wgrad_bf16), shared by tests/test_wgrad_routes.py (CPU: every
row resolves through oess_conv2d_wgrad_route, the plan the launch itself executes) and tests/test_hip_wgrad_exact.py (GPU:
every row that launches is bit-exact against float64).

A row is (name, geom, x_ps, dy_ps, workspace_bytes, want_kernel, want_slices, why):
  geom             (B, H, W, Cin_x, Cin, Cout, R, S, stride, pad, dil); Cin_x = channels present in x, Cin = the weight's
  x_ps, dy_ps      pixel strides in elements.  SLICE: the operand is the channel slice [8 : 8 + C] of a buffer 16 channels wider
                   (what the engine passes: slices of concat buffers); a number: the pixels lie that far apart in one flat
                   buffer (the 2 GiB rows)
  workspace_bytes  the bytes on offer; `per` below is one partial slice, tiles_m * tmv * tiles_n * 128 * 4
  want_kernel      a name of OESS_WGRAD_* in include/oess.h, or "ENOMEM" / "EINVAL" for a call that returns before any launch
  want_slices      partial tiles summed per element: < 16 -> wgrad_reduce_kernel, >= 16 -> wgrad_reduce_wide_kernel

K-steps are 64 output pixels; the LDS-DMA kernels walk a slice's pixels flat across row and image boundaries, the register-staged
and strip kernels take one output row (of a 64-pixel strip) per step."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SLICE = "slice"
DEFAULT_WS = 256 << 20            # what hip.conv2d_wgrad offers without a caller-owned workspace
HUGE_PS = 12064520                # 90 pixels this far apart span (89 * 12064520 + C) * 2 >= 0x7ffffff0 bytes for C >= 8
BELOW_PS = 12064512               # the multiple of 8 below: (89 * 12064512 + 16) * 2 = 2147483168 < 0x7ffffff0
ERRORS = {"EINVAL": -22, "ENOMEM": -12}


def header_kernels():
    """{name: value} of the OESS_WGRAD_* kernel values of include/oess.h."""
    txt = open(os.path.join(ROOT, "include", "oess.h")).read()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+OESS_WGRAD_([A-Z]+_\d+)\s+(\d+)\b", txt)}
    assert sorted(d.values()) == list(range(1, len(d) + 1)), "OESS_WGRAD_* values must be 1 .. count"
    return d


def strides(geom, x_ps, dy_ps):
    """the pixel strides of a row's call (SLICE resolved)"""
    Cin_x, Cout = geom[3], geom[5]
    return (Cin_x + 16 if x_ps == SLICE else x_ps), (Cout + 16 if dy_ps == SLICE else dy_ps)


def out_size(geom):
    B, H, W, Cin_x, Cin, Cout, R, S, stride, pad, dil = geom
    return (H + 2 * pad - dil * (R - 1) - 1) // stride + 1, (W + 2 * pad - dil * (S - 1) - 1) // stride + 1


_STEM = (2, 5, 13, 8, 5, 24, 5, 5, 1, 2, 1)            # per = 1 * 32 * 2 * 128 * 4 = 32768
_S2 = (3, 7, 70, 72, 72, 40, 3, 3, 2, 1, 1)            # per = 1 * 64 * 6 * 128 * 4 = 196608; Ho x Wo = 4 x 35
_DIL = (1, 11, 13, 48, 48, 136, 3, 3, 1, 2, 2)         # per = 2 * 128 * 4 * 128 * 4 = 524288; Ho x Wo = 11 x 13
_STRIP32 = (1, 250, 400, 64, 64, 32, 3, 3, 1, 1, 1)    # per = 32 * 5 * 128 * 4 = 81920
_REG = lambda Cout: (2, 5, 9, 16, 16, Cout, 3, 3, 1, 1, 1)

WGRAD_CASES = [
    ("dma32_5x5_stem", _STEM, SLICE, SLICE, DEFAULT_WS, "DMA_32", 10,
     "one output row of 13 pixels per slice; Kdim 200 ends inside the second 128-wide tile; Cin 5 < Cin_x 8 (channels 5..7 hold "
     "7.0 and must not reach the result); Cout 24 on the 32-row tile"),
    ("dma32_5x5_stem_ws4", _STEM, SLICE, SLICE, 4 * 32768, "DMA_32", 4,
     "the workspace clamps 10 slices to 4: three rows (39 pixels) per slice, the last slice one row; narrow reduce, one unrolled round"),
    ("dma32_5x5_stem_ws1", _STEM, SLICE, SLICE, 32768, "DMA_32", 1,
     "one slice walks all 130 pixels flat: three K-steps (the 2-stage ring wraps), across the image boundary, last step 2 pixels"),
    ("dma64_s2", _S2, SLICE, SLICE, DEFAULT_WS, "DMA_64", 12, "stride 2, Cout 40 on the 64-row tile, Kdim 648 ends inside the sixth tile"),
    ("dma64_s2_ws2", _S2, SLICE, SLICE, 2 * 196608, "DMA_64", 2,
     "two slices of 6 rows of 35 pixels: four K-steps with a ragged last one (18 pixels), each slice crosses an image boundary"),
    ("dma64_s2_ws1", _S2, SLICE, SLICE, 196608, "DMA_64", 1, "exactly one partial slice fits: 420 pixels, seven K-steps, three images"),
    ("dma64_s2_enomem", _S2, SLICE, SLICE, 196608 - 1, "ENOMEM", 0, "one byte short of one partial slice: no launch, dW untouched"),
    ("dma128_dil", _DIL, SLICE, SLICE, DEFAULT_WS, "DMA_128", 11, "dilation 2; two M tiles, the second with 8 valid rows of 128"),
    ("dma128_dil_ws3", _DIL, SLICE, SLICE, 3 * 524288 + 100, "DMA_128", 3,
     "a workspace that is no multiple of a slice: 3 slices of 4, 4 and 3 rows; the 100 spare bytes stay untouched"),
    ("dma128_dil_ws1", _DIL, SLICE, SLICE, 524288, "DMA_128", 1, "one slice of 143 pixels: three K-steps on the 128-row tile, last step 15 pixels"),
    ("dma128_1x1", (2, 10, 12, 32, 32, 256, 1, 1, 1, 0, 1), SLICE, SLICE, DEFAULT_WS, "DMA_128", 20,
     "1x1 head: one N tile with 32 valid columns, two full M tiles, wide reduce with 20 slices (lanes 0..3 add three, 4..7 two)"),
    ("dma32_1x3", (2, 6, 67, 16, 16, 8, 1, 3, 1, 1, 1), SLICE, SLICE, DEFAULT_WS, "DMA_32", 16,
     "R != S (tap = r * S + s on a 1 x 3 window); Wo 67 = a full K-step + 3 pixels; 16 slices: the wide-reduce threshold"),
    ("dma32_1x3_15", (3, 3, 67, 16, 16, 8, 1, 3, 1, 1, 1), SLICE, SLICE, DEFAULT_WS, "DMA_32", 15,
     "15 slices: the narrow reduce's last size, three unrolled rounds of 4 plus a tail of 3"),
    ("wide40", (2, 20, 9, 16, 16, 16, 3, 3, 1, 1, 1), SLICE, SLICE, DEFAULT_WS, "DMA_32", 40,
     "wide reduce, 40 slices: every split lane takes one unrolled round of 4 and one tail element"),
    ("wide70", (2, 35, 9, 16, 16, 72, 3, 3, 1, 1, 1), SLICE, SLICE, DEFAULT_WS, "DMA_128", 70,
     "wide reduce, 70 slices: lanes 0..5 take two unrolled rounds and a tail, lanes 6, 7 two rounds and no tail"),
    ("strip32", _STRIP32, SLICE, SLICE, DEFAULT_WS, "STRIP_32", 441,
     "7 strips with a 16-pixel last strip x 63 row ranges of 4 rows, the last range 2 rows"),
    ("strip32_fallback", _STRIP32, SLICE, SLICE, 16 << 20, "DMA_32", 84,
     "441 units x 81920 bytes do not fit 16 MiB: the strip layer falls back to the tiled kernel (same inputs as strip32)"),
    ("strip64", (2, 200, 258, 128, 128, 48, 3, 3, 1, 1, 1), SLICE, SLICE, DEFAULT_WS, "STRIP_64", 250,
     "two 64-channel chunks, a 2-pixel last strip, Cout 48 on the 64-row tile, 10 strips x 25 row ranges of 8 rows"),
    ("reg32", _REG(24), HUGE_PS, SLICE, DEFAULT_WS, "REG_32", 10, "x spans 2147484592 bytes: 64-bit addressing of x above 2^31"),
    ("reg64", _REG(40), SLICE, HUGE_PS, DEFAULT_WS, "REG_64", 10, "dy is the operand that spans more than 0x7ffffff0 bytes"),
    ("reg128", _REG(136), HUGE_PS, SLICE, DEFAULT_WS, "REG_128", 10, "register-staged 128-row tile, second M tile with 8 valid rows"),
    ("dma_below_2g", _REG(24), BELOW_PS, SLICE, DEFAULT_WS, "DMA_32", 10,
     "x ends at byte 2147483168, the last multiple-of-8 stride under 0x7ffffff0: 32-bit buffer offsets just below the limit"),
]

# Calls that oess_conv2d_wgrad_bf16 itself refuses with OESS_EINVAL before any launch (the query refuses the same numbers):
# (name, geom, x_ps, dy_ps)
EINVAL_CASES = [
    ("cin_x_below_cin", (2, 5, 9, 8, 16, 24, 3, 3, 1, 1, 1), 8, 24),
    ("cin_x_mod_8", (2, 5, 9, 12, 12, 24, 3, 3, 1, 1, 1), 16, 24),
    ("cout_mod_8", (2, 5, 9, 16, 16, 20, 3, 3, 1, 1, 1), 16, 24),
    ("x_stride_mod_8", (2, 5, 9, 16, 16, 24, 3, 3, 1, 1, 1), 20, 24),
    ("dy_stride_mod_8", (2, 5, 9, 16, 16, 24, 3, 3, 1, 1, 1), 16, 28),
    ("no_output_rows", (2, 2, 9, 16, 16, 24, 5, 3, 1, 0, 1), 16, 24),
]
