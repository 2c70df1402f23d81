"""Shared cases of the bilinear resize / L2-normalise kernels' tests (openess_amd/csrc/resize_ops.hip, the fused bilinear_l2 kernels
of norm_ops.hip, the index rule of bilinear_axis.h; tests/test_hip_resize_routes.py on the GPU, tests/test_resize_cases.py on the
CPU) and of the CPU measurement that sets their bounds (tools/exp_resize_bounds.py):

  * resize_route / l2norm_route / fused_route / pool_route restate the dispatch arithmetic of the entries; every case records the
    route it must take and REQUIRED_BRANCHES is covered by their union;
  * float64 references on the bf16 / fp32 operands: the bilinear forward with the source index and lambda computed in fp32 as
    src_index does and the blend in float64, its adjoint as the transpose of the same two per-axis weight matrices, F.normalize
    with the eps clamp and its adjoint, and the composed scatter_mean(normalize(upsample)) backward of the pooled node;
  * fp32 CPU models of the kernels' rounding points, written from the code and the comments of the kernels and not by calling
    them: they prove the exact cases exact in both associations (ATen's of resize_fwd_kernel, columns first of up_rows), measure how
    far correct fp32 arithmetic sits from float64, and take the mutations the CPU test holds the criteria against;
  * layouts that put an operand into a channel slice of a wider NaN-filled buffer;
  * exact integer data (|v| <= 3, dyadic weights, every sum below 2^24 after scaling: asserted) and three non-exact families.

Nothing here needs a GPU."""
import functools
import math

import torch

from tests.norm_cases import _TINY, err_bf16, err_fp32, ulp_bf16  # noqa: F401  (the same measures as the normalisation bounds)

SEED = 7411
THREADS = 256
GRID_CAP = 262144                                         # grid_for
FUSED_SCALAR_CAP = 16384                                  # bilinear_l2_kernel's grid
NT_BYTES = 256 << 20                                      # above it the fused vector kernel stores non-temporally
LDS_LIMIT = 64 * 1024
LIMIT = 1 << 24                                           # integers below it are exact in fp32, in any order of addition
EPS_TEST = 2.0 ** -10                                     # the eps the L2 entries receive here: 1 / eps is exact
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
DTYPES = {"bf16": BF16, "f32": F32}
FAMILIES = ("randn", "large_offset", "one_hot_pixel")
# name -> (c0, extra columns): pixel stride C + extra.  slice_vec keeps 16-byte alignment and a stride that is a multiple of the
# vector width for bf16 and fp32; slice_odd breaks both (4- / 8-byte offset, stride C + 6), so the scalar kernels run on any C
LAYOUTS = {"dense": (0, 0), "slice_vec": (8, 8), "slice_odd": (2, 6)}
# layouts of (input, output) of the two-operand entries: the two never share one; the first two keep the vector route
LAYOUT_PAIRS = (("dense", "slice_vec"), ("slice_vec", "dense"), ("slice_odd", "dense"), ("dense", "slice_odd"))
# (y, g, gx) of the L2 backward and (feat, gin) + its neighbours: three operands, two vector layouts, so y and gx share one on
# the vector route and nowhere else
LAYOUT_TRIPLES = (("dense", "slice_vec", "dense"), ("slice_vec", "dense", "slice_vec"), ("slice_odd", "dense", "slice_vec"),
                  ("dense", "slice_odd", "slice_vec"), ("slice_vec", "dense", "slice_odd"))
MUTATIONS = ("other_align_mode", "no_edge_clamp", "no_max0", "short_candidates", "swap_x_weights", "tmp_bf16", "strided_as_dense",
             "l2_no_clamp", "l2_proj_x", "carry_lost")

# ---- bounds: four times the largest figure of the fp32 models against float64 over FAMILIES x BOUNDED_GEOMS (resize), the L2
# shapes and the fused shapes (tools/exp_resize_bounds.py prints them; DESIGN.md carries them; tests/test_resize_cases.py
# re-measures them).  The measures are the *_figures functions below.
MODEL_FIGURE = {
    "resize_fwd_bf16": 1.26e-7,    # randn, (7,10)->(110,160) C=256, up_rows order
    "resize_fwd_f32": 1.92e-7,     # randn, (7,10)->(110,157) C=11
    "resize_bwd_bf16": 3.09e-8,    # large_offset, (7,10)->(110,160) C=256
    "resize_bwd_f32": 3.63e-7,     # large_offset, (7,10)->(110,157) C=11
    "l2_fwd_y": 1.62e-7,           # large_offset, fp32 P=37 C=256
    "l2_fwd_inv": 1.11e-7,         # randn, fp32 P=37 C=64
    "l2_bwd": 1.03e-7,             # randn, fp32 P=37 C=256
    "fused_y": 5.28e-7,            # randn, (11,16) x4 C=512, vector kernel
    "fused_inv": 2.52e-7,          # one_hot_pixel, (11,16) x4 C=192, scalar kernel
    "pool_bwd": 7.75e-9,           # (2,33)->(8,129) C=64: the pooled backward at the one geometry where it is not exact
}
BOUND = {k: 4.0 * v for k, v in MODEL_FIGURE.items()}
RSQRT_ULP = 2.0 ** -23                                    # one fp32 ulp (relative) added for the vector kernel's rsqrtf


def cdiv(a, b):
    return (a + b - 1) // b


def _gen(*key):
    h = SEED
    for k in key:
        for ch in str(k):
            h = (h * 1000003 + ord(ch)) % (1 << 31)
    return torch.Generator().manual_seed(h)


# --------------------------------------------------------------------------------------------- dispatch, restated
def vec_ok(layout, C, bf16):
    """resize_shared.h: C and the pixel stride multiples of the vector width, the pointer 16-byte aligned (the buffer itself is)"""
    c0, extra = LAYOUTS[layout]
    v, size = (8, 2) if bf16 else (4, 4)
    return C % v == 0 and (C + extra) % v == 0 and (c0 * size) % 16 == 0


def resize_route(bf16, H, W, C, Ho, Wo, layouts=("dense", "dense"), backward=False):
    """oess_resize_bilinear_nhwc_fwd / _bwd: one workgroup per output row (forward, x pass) or input row (y pass)"""
    vec = all(vec_ok(l, C, bf16) for l in layouts)
    r = dict(vec=vec, kernel="vec" if vec else "scalar", up_rows=False)
    if backward:
        return r
    lds = W * C * 4
    if bf16 and vec and Wo >= 4 * W and Ho >= 2 * H and (C >> 3) <= THREADS and lds <= LDS_LIMIT:
        cv = C >> 3
        ppi = THREADS // cv
        r.update(kernel="up_rows", up_rows=True, lds_bytes=lds, pixel_lanes=ppi, idle_lanes=THREADS - ppi * cv)
    else:
        r["lds_bytes"] = lds
    return r


def _lpp(C, bf16):
    v = 8 if bf16 else 4
    lpp = C // v if C % v == 0 else 0
    return lpp if lpp in (8, 16, 32, 64) else 0


def l2norm_route(bf16, P, C, layouts=("dense", "dense")):
    """oess_l2norm_nhwc_fwd / _bwd: LPP lanes per pixel on the vector route, one wave per pixel (4 per block) on the generic one"""
    lpp = _lpp(C, bf16)
    if lpp and all(vec_ok(l, C, bf16) for l in layouts):
        blocks = cdiv(P * lpp, THREADS)
        return dict(kernel="vec", lpp=lpp, grid=max(1, min(blocks, GRID_CAP)), capped=blocks > GRID_CAP)
    blocks = cdiv(P * 64, THREADS)
    return dict(kernel="generic", lpp=0, grid=max(1, min(blocks, GRID_CAP)), capped=blocks > GRID_CAP, lane_trips=cdiv(C, 64))


def fused_route(B, H, W, C, scale, layouts=("dense", "dense")):
    """oess_bilinear_l2norm_nhwc_bf16 (C % 64 == 0, C <= 512)"""
    assert C % 64 == 0 and C <= 512
    total = B * H * scale * W * scale
    lpp = _lpp(C, True)
    if lpp and all(vec_ok(l, C, True) for l in layouts):
        ppb = THREADS // lpp
        return dict(kernel="vec", lpp=lpp, run_len=cdiv(W * scale, ppb), grid=B * H * scale, capped=False,
                    nt_out=total * C * 2 > NT_BYTES)
    blocks = cdiv(total, 4)
    return dict(kernel="scalar", lpp=0, cpl=C // 64, grid=min(blocks, FUSED_SCALAR_CAP), capped=blocks > FUSED_SCALAR_CAP, nt_out=False)


def pool_route(W, C):
    """l2pool_bwd_x_kernel<LPP>: G = 256 / LPP input columns per iteration; column `base` of a later iteration takes its left
    neighbour's share from the LDS carry slot"""
    lpp = _lpp(C, True)
    assert lpp
    G = THREADS // lpp
    return dict(lpp=lpp, G=G, iterations=cdiv(W, G), carry_used=W > G)


REQUIRED_BRANCHES = frozenset((
    "resize_up_rows", "resize_up_rows_idle_lanes", "resize_up_rows_one_pixel_lane", "resize_up_rows_one_vector",
    "resize_up_rows_lds_over", "resize_up_rows_lds_fits_at_limit", "resize_up_rows_cv_over", "resize_up_rows_not_wo", "resize_up_rows_not_f32",
    "resize_vec_bf16", "resize_vec_f32", "resize_scalar_bf16_c", "resize_scalar_f32_c", "resize_scalar_bf16_layout", "resize_scalar_f32_layout",
    "resize_bwd_vec", "resize_bwd_scalar",
    "l2_vec_lpp8", "l2_vec_lpp16", "l2_vec_lpp32", "l2_vec_lpp64", "l2_generic_c", "l2_generic_layout", "l2_generic_lane_trips_2",
    "l2_grid_capped", "l2_grid_not_capped",
    "fused_vec_lpp8", "fused_vec_lpp16", "fused_vec_lpp32", "fused_vec_lpp64", "fused_scalar_cpl3", "fused_scalar_cpl5", "fused_scalar_cpl7",
    "fused_scalar_layout", "fused_scalar_capped", "fused_scalar_not_capped", "fused_nt", "fused_not_nt", "fused_run_len_1", "fused_run_len_gt1",
    "pool_lpp8", "pool_lpp16", "pool_lpp32", "pool_lpp64", "pool_carry_lpp8", "pool_carry_lpp16", "pool_carry_lpp32", "pool_carry_lpp64",
    "pool_no_carry"))


# --------------------------------------------------------------------------------------------- cases
# exact geometries: (H, W, Ho, Wo, align)
GEOMS = (
    (3, 5, 12, 20, False), (3, 5, 6, 20, False), (3, 5, 3, 20, False),                                 # x4 / x2: up_rows twice, then not
    (5, 3, 17, 9, True), (2, 9, 9, 17, True), (7, 7, 49, 49, True), (3, 3, 9, 9, True),                # align, dyadic ratio
    (8, 6, 4, 4, False), (9, 5, 5, 3, True), (40, 24, 5, 3, False),                                     # downsampling
    (1, 1, 5, 7, True), (4, 4, 1, 1, True), (5, 7, 5, 7, True), (5, 7, 5, 7, False), (1, 9, 4, 36, False),      # degenerate
)
GENERIC_CHANNELS = {"bf16": (8, 24, 11), "f32": (4, 12, 11, 1)}
RESIZE_B = 2
# limits of up_rows: (name, H, W, C, Ho, Wo, route of the dense-class layouts)
UP_ROWS_LIMITS = (
    ("lds_over", 2, 65, 256, 4, 260, dict(kernel="vec", up_rows=False, lds_bytes=66560)),
    ("lds_fits", 2, 64, 256, 4, 256, dict(kernel="up_rows", lds_bytes=65536, pixel_lanes=8, idle_lanes=0)),
    ("cv_over", 2, 2, 2056, 4, 8, dict(kernel="vec", up_rows=False)),
    ("one_pixel_lane", 2, 2, 2048, 4, 8, dict(kernel="up_rows", pixel_lanes=1, idle_lanes=0)),
    ("idle_lanes", 3, 5, 192, 12, 20, dict(kernel="up_rows", pixel_lanes=10, idle_lanes=16)),
    ("one_vector", 3, 5, 8, 12, 20, dict(kernel="up_rows", pixel_lanes=256, idle_lanes=0)),
)


# the geometries with Wo >= 4 W and Ho >= 2 H: bf16 with C % 8 == 0 takes up_rows there
UP_ROWS_GEOMS = ((3, 5, 12, 20, False), (3, 5, 6, 20, False), (7, 7, 49, 49, True), (1, 1, 5, 7, True), (1, 9, 4, 36, False))


def resize_cases():
    """(name, dtype, H, W, C, Ho, Wo, align, expected route on the vector layouts): every exact resize case"""
    out = []
    for geom in GEOMS:
        H, W, Ho, Wo, align = geom
        for dt, chans in GENERIC_CHANNELS.items():
            for C in chans:
                if C % (8 if dt == "bf16" else 4):
                    kernel = "scalar"
                else:
                    kernel = "up_rows" if dt == "bf16" and geom in UP_ROWS_GEOMS else "vec"
                out.append((f"{H}x{W}-{Ho}x{Wo}-{'a' if align else 'n'}", dt, H, W, C, Ho, Wo, align, dict(kernel=kernel)))
    for (name, H, W, C, Ho, Wo, expect) in UP_ROWS_LIMITS:
        out.append((name, "bf16", H, W, C, Ho, Wo, False, expect))
    return out


# bounded resize cases: (dtype, H, W, C, Ho, Wo, align): the workload ratios at small size, a downsampling, a non-integer ratio
BOUNDED_GEOMS = (("bf16", 7, 10, 256, 110, 160, False), ("bf16", 11, 16, 64, 44, 64, True), ("f32", 6, 6, 12, 3, 4, False),
                 ("f32", 7, 10, 11, 110, 157, False), ("bf16", 7, 10, 24, 110, 157, False), ("f32", 11, 16, 4, 44, 64, True))

L2_VEC_CHANNELS = {"f32": (32, 64, 128, 256), "bf16": (64, 128, 256, 512)}
L2_GENERIC_CHANNELS = (96, 40, 1, 3)
L2_PIXELS = (1, 5, 37)
L2_CAP_CASE = ("f32", 4 * GRID_CAP + 5, 3)                # 12 MB: crosses the grid cap of the generic kernel once


def l2_cases():
    """(dtype, P, C) of every exact L2 case but the grid-cap one"""
    out = []
    for dt in ("f32", "bf16"):
        for C in L2_VEC_CHANNELS[dt] + L2_GENERIC_CHANNELS:
            for P in L2_PIXELS:
                out.append((dt, P, C))
    return out


FUSED_EXACT_GEOMS = ((3, 3, 3), (7, 7, 7), (1, 7, 7), (3, 1, 3), (5, 6, 1))           # (H, W, scale), normalize = 0
FUSED_VEC_CHANNELS, FUSED_SCALAR_CHANNELS = (64, 128, 256, 512), (192, 320, 448)
FUSED_BOUNDED_GEOMS = tuple((H, W, s) for (H, W) in ((5, 7), (11, 16)) for s in (2, 3, 4))
FUSED_CAP_CASE = (1, 65, 65, 192, 4)                      # (B, H, W, C, scale): 67600 output pixels > 4 x 16384
FUSED_NT_CASE = (5, 64, 64, 512, 4)                       # 335 MB output
FUSED_B = 2

# The issue's wide geometry is (2, 33) -> (8, 129); its vertical ratio 1/7 is not dyadic, so no bit-exact answer exists there.
# The width, which is what the case is for (33 > 32 columns: LPP 8 carries), is kept and Ho is 9 (ratio 1/8).
POOL_GEOMS = ((3, 3, 9, 9), (7, 7, 49, 49), (2, 33, 9, 129))
POOL_ISSUE_WIDE = (2, 33, 8, 129)                         # the issue's geometry itself: bounded (BOUND["pool_bwd"]), every C
POOL_CHANNELS = (64, 128, 256, 512)
POOL_B, POOL_SPS, POOL_COUNT = 2, 6, 64.0
POOL_S = 2 * POOL_SPS - 2                                 # the last two ids of sample 1 fall at or above S


def branches():
    """names of REQUIRED_BRANCHES the cases enter, from the restated routes"""
    out = set()
    for (name, dt, H, W, C, Ho, Wo, align, _) in resize_cases():
        bf = dt == "bf16"
        for pair in LAYOUT_PAIRS:
            r = resize_route(bf, H, W, C, Ho, Wo, pair)
            rb = resize_route(bf, H, W, C, Ho, Wo, pair, backward=True)
            out.add("resize_bwd_vec" if rb["vec"] else "resize_bwd_scalar")
            if r["up_rows"]:
                out.add("resize_up_rows")
                out.update(k for k, on in (("resize_up_rows_idle_lanes", r["idle_lanes"] > 0), ("resize_up_rows_one_pixel_lane", r["pixel_lanes"] == 1),
                                           ("resize_up_rows_one_vector", C == 8 and Wo < r["pixel_lanes"]),
                                           ("resize_up_rows_lds_fits_at_limit", r["lds_bytes"] == LDS_LIMIT)) if on)
            elif r["vec"]:
                out.add("resize_vec_bf16" if bf else "resize_vec_f32")
                up = Wo >= 4 * W and Ho >= 2 * H
                out.update(k for k, on in (("resize_up_rows_lds_over", bf and up and r["lds_bytes"] > LDS_LIMIT),
                                           ("resize_up_rows_cv_over", bf and up and (C >> 3) > THREADS),
                                           ("resize_up_rows_not_wo", bf and Wo >= 4 * W and not up), ("resize_up_rows_not_f32", up and not bf)) if on)
            else:
                by_c = C % (8 if bf else 4) != 0
                out.add(f"resize_scalar_{dt}_{'c' if by_c else 'layout'}")
    for (dt, P, C) in l2_cases() + [L2_CAP_CASE]:
        for pair in LAYOUT_PAIRS if (dt, P, C) != L2_CAP_CASE else (("dense", "dense"),):
            r = l2norm_route(dt == "bf16", P, C, pair)
            out.add("l2_grid_capped" if r["capped"] else "l2_grid_not_capped")
            if r["kernel"] == "vec":
                out.add(f"l2_vec_lpp{r['lpp']}")
            else:
                out.add("l2_generic_layout" if _lpp(C, dt == "bf16") else "l2_generic_c")
                if r["lane_trips"] == 2:
                    out.add("l2_generic_lane_trips_2")
    for (B, H, W, C, scale, pair) in fused_cases():
        r = fused_route(B, H, W, C, scale, pair)
        if r["kernel"] == "vec":
            out.add(f"fused_vec_lpp{r['lpp']}")
            out.add("fused_run_len_1" if r["run_len"] == 1 else "fused_run_len_gt1")
        else:
            out.add(f"fused_scalar_cpl{r['cpl']}" if not _lpp(C, True) else "fused_scalar_layout")
            out.add("fused_scalar_capped" if r["capped"] else "fused_scalar_not_capped")
        out.add("fused_nt" if r["nt_out"] else "fused_not_nt")
    for (H, W, Ho, Wo) in POOL_GEOMS:
        for C in POOL_CHANNELS:
            r = pool_route(W, C)
            out.add(f"pool_lpp{r['lpp']}")
            out.add(f"pool_carry_lpp{r['lpp']}" if r["carry_used"] else "pool_no_carry")
    return out


def fused_cases():
    """(B, H, W, C, scale, (input layout, output layout)) of every fused call the GPU test makes"""
    out = []
    for (H, W, s) in FUSED_EXACT_GEOMS + FUSED_BOUNDED_GEOMS:
        for C in FUSED_VEC_CHANNELS:
            out += [(FUSED_B, H, W, C, s, pair) for pair in LAYOUT_PAIRS[:2]]
        for C in FUSED_SCALAR_CHANNELS:
            out += [(FUSED_B, H, W, C, s, pair) for pair in LAYOUT_PAIRS[:2]]
        out += [(FUSED_B, H, W, 64, s, pair) for pair in LAYOUT_PAIRS[2:]]
    out.append(FUSED_CAP_CASE + (("dense", "slice_vec"),))
    out.append(FUSED_NT_CASE + (("dense", "dense"),))
    out.append((1,) + FUSED_NT_CASE[1:] + (("dense", "dense"),))
    return out


# --------------------------------------------------------------------------------------------- layouts
def place(t, layout, device="cpu", fill=math.nan):
    """t [..., C] as the channel slice [c0 : c0 + C] of a [pixels, C + extra] buffer filled with `fill`: (buffer, view of t's shape)"""
    c0, extra = LAYOUTS[layout]
    C = t.shape[-1]
    n = t.numel() // C
    buf = torch.full((n, C + extra), fill, dtype=t.dtype, device=device)
    view = buf[:, c0:c0 + C].view(t.shape)
    view.copy_(t.to(device))
    return buf, view


def place_out(shape, dtype, layout, device="cpu"):
    """an output buffer of NaN: (buffer, view)"""
    return place(torch.full(tuple(shape), math.nan, dtype=dtype), layout, device)


def surroundings_untouched(buf, layout, C):
    c0, _ = LAYOUTS[layout]
    return bool(torch.isnan(buf[:, :c0]).all()) and bool(torch.isnan(buf[:, c0 + C:]).all())


def layout_stride(layout, C):
    return C + LAYOUTS[layout][1]


def kernel_view(buf, view, mutate=None):
    """what a kernel reads as the operand: the view; 'strided_as_dense' reads with pixel stride C from the view's first element"""
    if mutate == "strided_as_dense":
        return buf.reshape(-1)[view.storage_offset() - buf.storage_offset():][:view.numel()].view(view.shape)
    return view


# --------------------------------------------------------------------------------------------- data
def ints(shape, *key, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen("ints", *key)).to(F64)


def _pick(values, shape, g):
    return torch.tensor(values, dtype=F64)[torch.randint(0, len(values), tuple(shape), generator=g)]


def cast(ref, dtype):
    """the float64 reference rounded once to the output type (a -0 of the reference is +0: the kernels add into a +0 sum)"""
    return (ref + 0.0).to(dtype)


def assert_dyadic(v, q, what=""):
    """every value of v is an integer multiple of 2^-q and its magnitude times 2^q stays below 2^24"""
    s = v.double() * 2.0 ** q
    assert bool((s == s.round()).all()), f"{what}: not a multiple of 2^-{q}"
    assert float(s.abs().max()) < LIMIT, f"{what}: {float(s.abs().max())} >= 2^24 after scaling by 2^{q}"


def family_map(family, shape, *key):
    """fp32 values of a non-exact family, shape [B, H, W, C] or [P, C]"""
    g = _gen("family", family, *shape, *key)
    if family == "randn":
        return torch.randn(*shape, generator=g)
    if family == "large_offset":                          # values near 100, differences near 1: cancellation in b - a
        return 100.0 + torch.randn(*shape, generator=g)
    assert family == "one_hot_pixel"                      # one non-zero pixel per sample (every channel of it)
    x = torch.zeros(*shape)
    flat = x.view(shape[0], -1, shape[-1]) if len(shape) == 4 else x.view(1, -1, shape[-1])
    for b in range(flat.shape[0]):
        flat[b, int(torch.randint(0, flat.shape[1], (1,), generator=g))] = torch.randn(shape[-1], generator=g) + 2.0
    return x


# --------------------------------------------------------------------------------------------- fp32 arithmetic of the models
# Products, sums and differences of fp32 tensors are IEEE on every host.  A host's vectorised fp32 sqrt is not always correctly
# rounded (an AVX-512 build of torch returned sqrtf(168) one ulp high), and a library sum adds in a host-dependent order, so the
# models form sqrt and the divide in float64 and round once -- with 53 >= 2 x 24 + 2 bits that is the correctly rounded fp32
# operation -- and add channels in a fixed tree.
def div32(a, b):
    """fl32(a / b) of fp32 operands"""
    return (torch.as_tensor(a, dtype=F32).double() / torch.as_tensor(b, dtype=F32).double()).float()


def sqrt32(a):
    """fl32(sqrt(a)) of an fp32 operand"""
    return torch.sqrt(a.float().double()).float()


# --------------------------------------------------------------------------------------------- the index rule, in fp32
def axis_index(inn, out, align, mutate=None):
    """make_axis + src_index of bilinear_axis.h for dst = 0 .. out - 1, every operation in fp32: (scale, i0, i1, lambda)"""
    use_align = (not align) if mutate == "other_align_mode" else bool(align)
    if use_align:
        scale = div32(float(inn - 1), float(out - 1)) if out > 1 else torch.zeros((), dtype=F32)
    else:
        scale = div32(float(inn), float(out))
    d = torch.arange(out, dtype=F32)
    if use_align:
        s = scale * d
    else:
        s = scale * (d + 0.5) - 0.5
        if mutate != "no_max0":
            s = s.clamp_min(0.0)
    i0 = s.to(torch.int64).clamp(max=inn - 1)             # (int) truncates towards zero
    i1 = i0 + 1 if mutate == "no_edge_clamp" else torch.where(i0 < inn - 1, i0 + 1, i0)
    lam = s - i0.to(F32)
    return scale, i0, i1, lam


def candidates(inn, out, align, mutate=None):
    """candidates() of bilinear_axis.h for i = 0 .. in - 1 in fp32: (lo, hi), inclusive"""
    scale = axis_index(inn, out, align, mutate)[0]
    use_align = (not align) if mutate == "other_align_mode" else bool(align)
    if float(scale) <= 0.0:
        lo, hi = torch.zeros(inn, dtype=torch.int64), torch.full((inn,), out - 1, dtype=torch.int64)
    else:
        inv = div32(1.0, scale)
        i = torch.arange(inn, dtype=F32)
        if use_align:
            a, b = (i - 1.0) * inv, (i + 1.0) * inv
        else:
            a, b = (i - 0.5) * inv - 0.5, (i + 1.5) * inv - 0.5
        lo = (torch.floor(a).to(torch.int64) - 2).clamp(min=0)
        hi = (torch.ceil(b).to(torch.int64) + 2).clamp(max=out - 1)
    if mutate == "short_candidates":                      # `ox < hi` for `ox <= hi`
        hi = hi - 1
    return lo, hi


def axis_weights32(inn, out, align, mutate=None, swap=False):
    """weight_for(dst, i) in fp32 for every (dst, i) the gather visits: [out, in], zero outside the candidate range"""
    _, i0, i1, lam = axis_index(inn, out, align, mutate)
    w0, w1 = (lam, 1.0 - lam) if swap else (1.0 - lam, lam)
    i = torch.arange(inn)[None, :]
    zero = torch.zeros((), dtype=F32)
    Wm = torch.where(i0[:, None] == i, w0[:, None], zero) + torch.where(i1[:, None] == i, w1[:, None], zero)
    lo, hi = candidates(inn, out, align, mutate)
    o = torch.arange(out)[:, None]
    return torch.where((o >= lo[None, :]) & (o <= hi[None, :]), Wm, zero)


def axis_matrix64(inn, out, align):
    """the float64 weight matrix [out, in] of one axis: fp32 index and lambda (as src_index leaves them), 1 - lambda in float64"""
    _, i0, i1, lam = axis_index(inn, out, align)
    M = torch.zeros(out, inn, dtype=F64)
    o = torch.arange(out)
    M.index_put_((o, i0), 1.0 - lam.double(), accumulate=True)
    M.index_put_((o, i1), lam.double(), accumulate=True)
    return M


# --------------------------------------------------------------------------------------------- float64 references
def resize_fwd64(x, Ho, Wo, align):
    """[B, H, W, C] -> [B, Ho, Wo, C]: My x Mx^T in float64"""
    B, H, W, C = x.shape
    return torch.einsum("oh,bhwc,pw->bopc", axis_matrix64(H, Ho, align), x.double(), axis_matrix64(W, Wo, align))


def resize_bwd64(g, H, W, align):
    """the adjoint: the transpose of the same two matrices"""
    B, Ho, Wo, C = g.shape
    return torch.einsum("oh,bopc,pw->bhwc", axis_matrix64(H, Ho, align), g.double(), axis_matrix64(W, Wo, align))


def eps32(eps):
    """the fp32 value the entries receive"""
    return float(torch.tensor(eps, dtype=F32))


def clamp_threshold(eps):
    """1.0f / eps as the backward kernels form it: the threshold is compared with an operand, so the reference takes the same one"""
    return float(div32(1.0, eps))


def l2_fwd64(x, eps):
    """F.normalize(x, dim=-1, eps): (y, 1 / max(|x|, eps)) in float64"""
    xd = x.double()
    inv = 1.0 / xd.norm(dim=-1).clamp_min(eps32(eps))
    return xd * inv[..., None], inv


def l2_bwd64(y, g, inv, eps):
    """gx = inv (g - y <y, g>); where the norm was clamped (inv >= 1 / eps: |x| <= eps, y = x / eps) gx = g / eps = inv g"""
    yd, gd, iv = y.double(), g.double(), inv.double()[..., None]
    dot = (yd * gd).sum(-1, keepdim=True)
    return torch.where(iv >= clamp_threshold(eps), iv * gd, iv * (gd - yd * dot))


def pool_table64(gk, count):
    """gk / (count + 1e-6) with the denominator formed in fp32 as pool_table_kernel forms it, the quotient in float64"""
    den = (count.float() + torch.tensor(1e-6, dtype=F32)).double()
    return gk.double() / den[:, None]


def pool_pixel_grad64(ids, table, B, sps):
    """the gradient row of every output pixel: table[ids + b sps], zero where that falls outside the table"""
    S, C = table.shape
    n = ids.numel() // B
    gid = ids.view(B, n) + (torch.arange(B) * sps)[:, None]
    ok = (gid >= 0) & (gid < S)
    return torch.where(ok[..., None], table[gid.clamp(0, S - 1)], torch.zeros((), dtype=F64))


def pool_bwd64(feat, inv, ids, gk, count, sps, H, W, eps):
    """d/dx of scatter_mean(normalize(upsample(x))) from the saved normalised map feat [B, Ho, Wo, C] and inv [B, Ho, Wo]"""
    B, Ho, Wo, C = feat.shape
    g = pool_pixel_grad64(ids, pool_table64(gk, count), B, sps).view(B, Ho, Wo, C)
    return resize_bwd64(l2_bwd64(feat, g, inv.view(B, Ho, Wo), eps), H, W, True)


# --------------------------------------------------------------------------------------------- fp32 models
def _pad_nan(xf):
    """one NaN row and column behind H and W: what an index one past the edge reads"""
    B, H, W, C = xf.shape
    p = torch.full((B, H + 1, W + 1, C), math.nan, dtype=F32)
    p[:, :H, :W] = xf
    return p


def resize_fwd_model(x, Ho, Wo, align, order="aten", mutate=None):
    """resize_fwd_kernel (order 'aten': hy (hx p00 + wx p01) + wy (hx p10 + wx p11)) or resize_up_rows_bf16_kernel (order
    'up_rows': V = hy a + wy d, then hx V[x0] + wx V[x1]) in fp32, one rounding to the output type"""
    B, H, W, C = x.shape
    xf = x.float()
    _, y0, y1, wy = axis_index(H, Ho, align, mutate)
    _, x0, x1, wx = axis_index(W, Wo, align, mutate)
    if mutate == "no_edge_clamp":
        xf = _pad_nan(xf)
    hy, hx = 1.0 - wy, 1.0 - wx
    if mutate == "swap_x_weights":
        hx, wx = wx, hx
    hy, wy, hx, wx = hy[:, None, None], wy[:, None, None], hx[:, None], wx[:, None]
    r0, r1 = xf[:, y0], xf[:, y1]
    if order == "aten":
        r = hy * (hx * r0[:, :, x0] + wx * r0[:, :, x1]) + wy * (hx * r1[:, :, x0] + wx * r1[:, :, x1])
    else:
        V = hy * r0 + wy * r1
        r = hx * V[:, :, x0] + wx * V[:, :, x1]
    return r.to(x.dtype)


def _gather_axis(t, Wm, dim):
    """acc[i] = sum over dst ascending of w(dst, i) t[dst] in fp32 along `dim` (1 or 2 of [B, Y, X, C]), as the kernels add"""
    out, inn = Wm.shape
    shape = list(t.shape)
    shape[dim] = inn
    acc = torch.zeros(shape, dtype=F32)
    wshape = [1, 1, 1, 1]
    wshape[dim] = inn
    for o in range(out):
        acc = acc + Wm[o].view(wshape) * t.select(dim, o).unsqueeze(dim)
    return acc


def resize_bwd_model(g, H, W, align, mutate=None):
    """resize_bwd_x_kernel then resize_bwd_y_kernel: fp32 gathers over the candidate range in ascending order, a dense fp32
    intermediate, one rounding to the gradient's type"""
    B, Ho, Wo, C = g.shape
    tmp = _gather_axis(g.float(), axis_weights32(W, Wo, align, mutate, swap=mutate == "swap_x_weights"), 2)
    if mutate == "tmp_bf16":
        tmp = tmp.bfloat16().float()
    return _gather_axis(tmp, axis_weights32(H, Ho, align, mutate), 1).to(g.dtype)


def _sum32(t):
    """a channel sum in fp32 by halving, the same on every host (exact data: any order gives the same bits; otherwise one correct
    order among the kernels' many)"""
    t = t.float()
    n = 1
    while n < t.shape[-1]:
        n *= 2
    if n != t.shape[-1]:
        t = torch.cat([t, torch.zeros(t.shape[:-1] + (n - t.shape[-1],), dtype=F32)], dim=-1)
    while n > 1:
        n //= 2
        t = t[..., :n] + t[..., n:]
    return t[..., 0]


def l2_fwd_model(x, eps, mutate=None):
    """l2norm_fwd(_vec)_kernel: ss in fp32, inv = 1.0f / fmaxf(sqrtf(ss), eps), y = x inv rounded once: (y, inv).  sqrtf, the
    divide go through sqrt32 / div32"""
    xf = x.float()
    n = sqrt32(_sum32(xf * xf))
    if mutate != "l2_no_clamp":
        n = torch.maximum(n, torch.tensor(eps, dtype=F32))
    inv = div32(1.0, n)
    return (xf * inv[..., None]).to(x.dtype), inv


def l2_bwd_model(y, g, inv, eps, mutate=None, x=None):
    """l2norm_bwd(_vec)_kernel: dot in fp32, clamped = inv >= 1.0f / eps, r = clamped ? inv g : inv (g - y dot).
    mutate 'l2_proj_x': the projection is taken with x for y"""
    yf, gf, iv = (x if mutate == "l2_proj_x" else y).float(), g.float(), inv.float()[..., None]
    dot = _sum32(yf * gf)[..., None]
    full = iv * (gf - yf * dot)
    if mutate == "l2_no_clamp":
        return full.to(g.dtype)
    return torch.where(iv >= div32(1.0, eps), iv * gf, full).to(g.dtype)


def fused_model(x, scale, normalize, kernel):
    """bilinear_l2_vec_kernel (kernel 'vec': columns blended vertically, L + (R - L) wx; inv = 1 / sqrt(max(ss, 1e-24)) for its
    rsqrtf) or bilinear_l2_kernel ('scalar': a + (b - a) wx per row, top + (bot - top) wy; inv = 1 / max(sqrt(ss), 1e-12)):
    (bf16 out, fp32 inv or None)"""
    B, H, W, C = x.shape
    xf = x.float()
    _, y0, y1, wy = axis_index(H, H * scale, True)
    _, x0, x1, wx = axis_index(W, W * scale, True)
    wy, wx = wy[:, None, None], wx[:, None]
    r0, r1 = xf[:, y0], xf[:, y1]
    if kernel == "vec":
        col = r0 + (r1 - r0) * wy
        L, R = col[:, :, x0], col[:, :, x1]
        v = L + (R - L) * wx
    else:
        top = r0[:, :, x0] + (r0[:, :, x1] - r0[:, :, x0]) * wx
        bot = r1[:, :, x0] + (r1[:, :, x1] - r1[:, :, x0]) * wx
        v = top + (bot - top) * wy
    if not normalize:
        return v.bfloat16(), None
    ss = _sum32(v * v)
    inv = div32(1.0, sqrt32(ss.clamp_min(1e-24))) if kernel == "vec" else div32(1.0, sqrt32(ss).clamp_min(1e-12))
    return (v * inv[..., None]).bfloat16(), inv


def pool_bwd_model(feat, inv, ids, gk, count, sps, H, W, eps, mutate=None):
    """pool_table_kernel, l2pool_bwd_x_kernel<LPP>, resize_bwd_y_kernel<bf16>: every output pixel forms its L2 adjoint row
    r = g - f <f, g> (dot 0 where inv >= 1 / eps) once, adds inv (1 - lam) r to its left column's A and inv lam r to B, the share of
    the right neighbour; tmp[ix] = A(ix) + B(ix - 1).  mutate 'carry_lost': B(ix - 1) is dropped where ix opens an iteration;
    'tmp_bf16': the intermediate is rounded to bf16 before the y pass"""
    B, Ho, Wo, C = feat.shape
    S = gk.shape[0]
    f32 = F32
    table = div32(gk, (count.float() + torch.tensor(1e-6, dtype=f32))[:, None])
    n = Ho * Wo
    gid = ids.view(B, n) + (torch.arange(B) * sps)[:, None]
    ok = ((gid >= 0) & (gid < S)).view(B, Ho, Wo)
    g = table[gid.clamp(0, S - 1)].view(B, Ho, Wo, C)
    f = feat.float()
    iv = inv.float().view(B, Ho, Wo)
    dot = _sum32(f * g)
    dot = torch.where(iv >= div32(1.0, eps), torch.zeros((), dtype=f32), dot)
    r = g - f * dot[..., None]
    _, x0, x1, lam = axis_index(W, Wo, True)
    A, Bq = torch.zeros(B, Ho, W, C, dtype=f32), torch.zeros(B, Ho, W, C, dtype=f32)
    for ox in range(Wo):
        same = int(x1[ox]) == int(x0[ox])
        wa = iv[:, :, ox] if same else iv[:, :, ox] * (1.0 - lam[ox])
        keep = ok[:, :, ox, None]
        zero = torch.zeros((), dtype=f32)
        A[:, :, int(x0[ox])] = A[:, :, int(x0[ox])] + torch.where(keep, wa[..., None] * r[:, :, ox], zero)
        if not same:
            wb = iv[:, :, ox] * lam[ox]
            Bq[:, :, int(x0[ox])] = Bq[:, :, int(x0[ox])] + torch.where(keep, wb[..., None] * r[:, :, ox], zero)
    G = pool_route(W, C)["G"]
    tmp = A.clone()
    for ix in range(1, W):
        if mutate == "carry_lost" and ix % G == 0:
            continue
        tmp[:, :, ix] = A[:, :, ix] + Bq[:, :, ix - 1]
    if mutate == "tmp_bf16":
        tmp = tmp.bfloat16().float()
    return _gather_axis(tmp, axis_weights32(H, Ho, True), 1).bfloat16()


# --------------------------------------------------------------------------------------------- exact data
@functools.lru_cache(maxsize=None)
def exact_resize(dt, H, W, C, Ho, Wo, align, B=RESIZE_B):
    """x and g: integers in [-3, 3].  The weights are dyadic with a common denominator of at most 64 per pixel (asserted on the
    reference): the forward is then a multiple of 1/64 below 4 in magnitude, exact in bf16 (|v| 64 < 256), and every sum of
    the adjoint stays below 2^24 in units of 2^-12 (asserted on the sum of magnitudes)."""
    dtype = DTYPES[dt]
    x = ints((B, H, W, C), "rx", dt, H, W, C, Ho, Wo, align)
    g = ints((B, Ho, Wo, C), "rg", dt, H, W, C, Ho, Wo, align)
    My, Mx = axis_matrix64(H, Ho, align), axis_matrix64(W, Wo, align)
    assert_dyadic(My, 3, "My")
    assert_dyadic(Mx, 3, "Mx")
    assert bool((My >= 0).all()) and bool((Mx >= 0).all())
    y = resize_fwd64(x, Ho, Wo, align)
    assert_dyadic(y, 6, "forward")
    assert float(y.abs().max()) * 64 < 256
    gin = resize_bwd64(g, H, W, align)
    assert_dyadic(resize_bwd64(g.abs(), H, W, align), 6, "adjoint sum of magnitudes")
    if dt == "bf16":
        assert bool((y.bfloat16().double() == y).all())
    return dict(x=x.to(dtype), g=g.to(dtype), y=cast(y, dtype), gin=cast(gin, dtype), gin64=gin)


def l2_special_rows(C):
    """rows for the eps clamp with eps = 2^-10, each one-hot so that the norm is the magnitude itself: zero, just below eps,
    just above eps, exactly eps, and an integer one-hot"""
    rows = torch.zeros(5, C, dtype=F64)
    rows[1, 0] = EPS_TEST * (1.0 - 2.0 ** -8)
    rows[2, C - 1] = -EPS_TEST * (1.0 + 2.0 ** -7)
    rows[3, C // 2] = EPS_TEST
    rows[4, C // 3] = 3.0
    return rows


@functools.lru_cache(maxsize=None)
def exact_l2(dt, P, C):
    """forward: integer x (sum of squares exact in any order; sqrtf, the divide and the product are correctly rounded, so the fp32
    model is the answer to the bit) with the special rows from P >= 5.  backward: y multiples of 1/4 with |y| <= 1, integer g, inv a
    power of two with some at and above 1 / eps: every product and sum is exact, the float64 reference cast once is the answer."""
    dtype = DTYPES[dt]
    x = ints((P, C), "l2x", dt, P, C)
    if P >= 5:
        x[:5] = l2_special_rows(C)
    assert int((x * x).sum(-1).max()) < LIMIT
    xt = x.to(dtype)
    assert bool((xt.double() == x).all())
    g = _gen("l2b", dt, P, C)
    y = torch.randint(-4, 5, (P, C), generator=g).to(F64) / 4.0
    gy = torch.randint(-3, 4, (P, C), generator=g).to(F64)
    inv = _pick((0.5, 1.0, 2.0, 512.0, 1024.0, 2048.0), (P,), g)
    if P >= 5:
        inv[:5] = torch.tensor((1.0, 512.0, 1024.0, 2048.0, 0.5), dtype=F64)
    else:
        inv[0] = 1024.0
    gx = l2_bwd64(y, gy, inv, EPS_TEST)
    assert_dyadic((y * gy).abs().sum(-1), 2, "dot")
    assert_dyadic(gx / inv[:, None], 4, "g - y dot")
    assert_dyadic(gx, 5, "gx")
    return dict(x=xt, y=y.to(dtype), g=gy.to(dtype), inv=inv.float(), gx=cast(gx, dtype), gx64=gx)


@functools.lru_cache(maxsize=None)
def exact_fused(H, W, scale, C, B=FUSED_B):
    """normalize = 0: the align_corners bilinear of integers at a dyadic ratio, exact in bf16"""
    x = ints((B, H, W, C), "fx", H, W, scale, C)
    y = resize_fwd64(x, H * scale, W * scale, True)
    assert_dyadic(axis_matrix64(H, H * scale, True), 3)
    assert_dyadic(axis_matrix64(W, W * scale, True), 3)
    assert bool((y.bfloat16().double() == y).all())
    return dict(x=x.bfloat16(), y=cast(y, BF16))


def pool_ids(B, Ho, Wo, sps):
    """sample 0: runs of three equal ids (the held table row is reused) with -1 at every 11th pixel; sample 1: an id that changes
    at every pixel, all of 0 .. sps - 1, so the last two (+ sps) fall at or above S = 2 sps - 2"""
    n = Ho * Wo
    p = torch.arange(n)
    a = (p // 3) % sps
    a = torch.where(p % 11 == 10, torch.full_like(a, -1), a)
    b = (p * 5 + 3) % sps
    ids = torch.stack([a, b] + [b] * (B - 2)).to(torch.int64)
    assert bool((b[1:] != b[:-1]).all())
    return ids.reshape(-1)


@functools.lru_cache(maxsize=None)
def exact_pool(H, W, Ho, Wo, C, B=POOL_B):
    """gk integers in [-3, 3], count 64 (fl32(64 + 1e-6) == 64: the table is gk / 64), feat multiples of 1/4 with |f| <= 1/2,
    inv in {1, 2, 4} with two pixels clamped (1 / eps and 2 / eps, eps = 2^-10).  Every term of the adjoint is a multiple of 2^-16
    (2^-10 for r, 2^-3 per axis weight) and the sums of magnitudes stay below 2^24 in that unit (asserted)."""
    g = _gen("pool", H, W, Ho, Wo, C)
    S, sps = POOL_S, POOL_SPS
    assert float(torch.tensor(POOL_COUNT, dtype=F32) + torch.tensor(1e-6, dtype=F32)) == POOL_COUNT
    assert float(torch.tensor(16.0, dtype=F32) + torch.tensor(1e-6, dtype=F32)) != 16.0
    gk = torch.randint(-3, 4, (S, C), generator=g).to(F64)
    count = torch.full((S,), POOL_COUNT, dtype=F32)
    feat = torch.randint(-2, 3, (B, Ho, Wo, C), generator=g).to(F64) / 4.0
    inv = _pick((1.0, 2.0, 4.0), (B * Ho * Wo,), g)
    inv[Wo + 1], inv[Ho * Wo + 2 * Wo + 2] = 1.0 / EPS_TEST, 2.0 / EPS_TEST
    ids = pool_ids(B, Ho, Wo, sps)
    gid = ids.view(B, -1) + (torch.arange(B) * sps)[:, None]
    assert bool((gid < 0).any()) and bool((gid >= S).any()) and bool(((gid >= 0) & (gid < S)).any())
    assert_dyadic(axis_matrix64(H, Ho, True), 3)
    assert_dyadic(axis_matrix64(W, Wo, True), 3)
    gp = pool_pixel_grad64(ids, pool_table64(gk, count), B, sps).view(B, Ho, Wo, C)
    assert_dyadic((feat * gp).abs().sum(-1), 8, "dot")
    r = l2_bwd64(feat, gp, inv.view(B, Ho, Wo), EPS_TEST)
    assert_dyadic(r, 10, "adjoint row")
    assert_dyadic(resize_bwd64(r.abs(), H, W, True), 16, "adjoint sum of magnitudes")
    gin = pool_bwd64(feat, inv, ids, gk, count, sps, H, W, EPS_TEST)
    return dict(feat=feat.bfloat16(), inv=inv.float(), ids=ids, gk=gk.float(), count=count, gin=cast(gin, BF16), gin64=gin, S=S, sps=sps)


# --------------------------------------------------------------------------------------------- the measurement
def resize_fwd_figure(got, x, Ho, Wo, align):
    """distance to float64 over the bilinear blend of |x| (bf16: less the half ulp of the one final rounding)"""
    ref, scale = resize_fwd64(x, Ho, Wo, align), resize_fwd64(x.double().abs(), Ho, Wo, align)
    return (err_bf16 if got.dtype == BF16 else err_fp32)(got, ref, scale)


def resize_bwd_figure(got, g, H, W, align):
    """distance to float64 over the adjoint of |g|"""
    ref, scale = resize_bwd64(g, H, W, align), resize_bwd64(g.double().abs(), H, W, align)
    return (err_bf16 if got.dtype == BF16 else err_fp32)(got, ref, scale)


def l2_fwd_figures(y, inv, x, eps):
    """y: distance to float64 over |y64| (no cancellation in a sum of squares; a zero stays a zero); inv: relative"""
    y64, inv64 = l2_fwd64(x, eps)
    return dict(l2_fwd_y=(err_bf16 if y.dtype == BF16 else err_fp32)(y, y64, y64.abs()), l2_fwd_inv=err_fp32(inv, inv64, inv64))


def l2_bwd_figure(gx, y, g, inv, eps):
    """distance to float64 over inv (|g| + |y| sum |y g|)"""
    ref = l2_bwd64(y, g, inv, eps)
    scale = inv.double()[..., None] * (g.double().abs() + y.double().abs() * (y.double() * g.double()).abs().sum(-1, keepdim=True))
    return (err_bf16 if gx.dtype == BF16 else err_fp32)(gx, ref, scale)


def fused_figures(y, inv, x, scale):
    """normalize(upsample(x)): an error dv of the blend moves y_c by dv_c / n - y_c <y, dv> / n, so the natural scale of y_c is
    (A_c + |y_c| |A|) / n with A the blend of |x| and n the norm; that of inv is inv |A| / n"""
    B, H, W, C = x.shape
    v = resize_fwd64(x, H * scale, W * scale, True)
    A = resize_fwd64(x.double().abs(), H * scale, W * scale, True)
    n = v.norm(dim=-1).clamp_min(1e-12)
    An = A.norm(dim=-1)
    y64 = v / n[..., None]
    out = dict(fused_y=err_bf16(y, y64, (A + y64.abs() * An[..., None]) / n[..., None]))
    if inv is not None:
        out["fused_inv"] = err_fp32(inv.view(n.shape), 1.0 / n, (An / n).clamp_min(1.0) / n)      # a zero pixel: inv = 1e12, relative
    return out


def pool_bound():
    """the pooled backward through the wrapper, on operands no model was measured on: every output pixel's adjoint row within the L2 backward's bound plus one fp32
    ulp for the table's quotient, the gather within the bf16 resize backward's, measured over the adjoint of the rows' scale"""
    return BOUND["l2_bwd"] + BOUND["resize_bwd_bf16"] + 2.0 ** -23


def pool_figure(got, feat, inv, ids, gk, count, sps, H, W, eps):
    B, Ho, Wo, C = feat.shape
    ref = pool_bwd64(feat, inv, ids, gk, count, sps, H, W, eps)
    gp = pool_pixel_grad64(ids, pool_table64(gk, count), B, sps).view(B, Ho, Wo, C)
    iv = inv.view(B, Ho, Wo).double()[..., None]
    scale = iv * (gp.abs() + feat.double().abs() * (feat.double() * gp).abs().sum(-1, keepdim=True))
    return err_bf16(got, ref, resize_bwd64(scale, H, W, True))


@functools.lru_cache(maxsize=None)
def wide_pool(C, B=POOL_B):
    """operands of the exact pooled cases' kind at the issue's (2, 33) -> (8, 129); nothing is asserted about exactness"""
    H, W, Ho, Wo = POOL_ISSUE_WIDE
    g = _gen("widepool", C)
    S, sps = POOL_S, POOL_SPS
    return dict(gk=torch.randint(-3, 4, (S, C), generator=g).float(), count=torch.full((S,), POOL_COUNT, dtype=F32),
                feat=(torch.randint(-2, 3, (B, Ho, Wo, C), generator=g).to(F64) / 4.0).bfloat16(),
                inv=_pick((1.0, 2.0, 4.0), (B * Ho * Wo,), g).float(), ids=pool_ids(B, Ho, Wo, sps), S=S, sps=sps)


def bounded_l2_shapes():
    return [(dt, 37, C) for dt in ("f32", "bf16") for C in L2_VEC_CHANNELS[dt] + L2_GENERIC_CHANNELS]


def l2_family_inputs(family, dt, P, C):
    x = family_map(family, (P, C), "l2", dt).to(DTYPES[dt])
    g = torch.randn(P, C, generator=_gen("l2g", family, dt, P, C)).to(DTYPES[dt])
    return x, g


def resize_family_inputs(family, dt, H, W, C, Ho, Wo, B=RESIZE_B):
    x = family_map(family, (B, H, W, C), "rs", dt).to(DTYPES[dt])
    g = family_map(family, (B, Ho, Wo, C), "rsg", dt).to(DTYPES[dt])
    return x, g


def fused_family_input(family, H, W, C, B=FUSED_B):
    return family_map(family, (B, H, W, C), "fu").bfloat16()


def model_orders(dt, H, W, C, Ho, Wo):
    """the associations a correct forward may take at this shape"""
    return ("aten", "up_rows") if resize_route(dt == "bf16", H, W, C, Ho, Wo)["up_rows"] else ("aten",)


def measure(report=None):
    """the largest figure of every quantity over the bounded cases and the families: {quantity: (figure, where)}"""
    worst = {}

    def take(k, v, where):
        if report:
            report(k, v, where)
        if v > worst.get(k, (-1.0,))[0]:
            worst[k] = (v, where)

    for family in FAMILIES:
        for (dt, H, W, C, Ho, Wo, align) in BOUNDED_GEOMS:
            x, g = resize_family_inputs(family, dt, H, W, C, Ho, Wo)
            where = f"{family} {dt} ({H},{W})->({Ho},{Wo}) C={C}"
            for order in model_orders(dt, H, W, C, Ho, Wo):
                take(f"resize_fwd_{dt}", resize_fwd_figure(resize_fwd_model(x, Ho, Wo, align, order), x, Ho, Wo, align), where + " " + order)
            take(f"resize_bwd_{dt}", resize_bwd_figure(resize_bwd_model(g, H, W, align), g, H, W, align), where)
        for (dt, P, C) in bounded_l2_shapes():
            x, g = l2_family_inputs(family, dt, P, C)
            where = f"{family} {dt} P={P} C={C}"
            y, inv = l2_fwd_model(x, 1e-12)
            for k, v in l2_fwd_figures(y, inv, x, 1e-12).items():
                take(k, v, where)
            take("l2_bwd", l2_bwd_figure(l2_bwd_model(y, g, inv, 1e-12), y, g, inv, 1e-12), where)
        for (H, W, s) in FUSED_BOUNDED_GEOMS:
            for C in FUSED_VEC_CHANNELS + FUSED_SCALAR_CHANNELS:
                x = fused_family_input(family, H, W, C)
                kernels = ("vec", "scalar") if C == 64 else (fused_route(FUSED_B, H, W, C, s)["kernel"],)
                for kernel in kernels:
                    y, inv = fused_model(x, s, True, kernel)
                    for k, v in fused_figures(y, inv, x, s).items():
                        take(k, v, f"{family} ({H},{W}) x{s} C={C} {kernel}")
    H, W, Ho, Wo = POOL_ISSUE_WIDE                        # the pooled backward at the one geometry where it is not exact
    for C in POOL_CHANNELS:
        c = wide_pool(C)
        got = pool_bwd_model(c["feat"], c["inv"], c["ids"], c["gk"], c["count"], c["sps"], H, W, EPS_TEST)
        take("pool_bwd", pool_figure(got, c["feat"], c["inv"], c["ids"], c["gk"], c["count"], c["sps"], H, W, EPS_TEST), f"(2,33)->(8,129) C={C}")
    B, H, W, C, s = FUSED_CAP_CASE                        # the scalar kernel's capped grid runs bounded too (its ratio is not dyadic)
    x = fused_family_input("randn", H, W, C, B)
    for k, v in fused_figures(*fused_model(x, s, True, "scalar"), x, s).items():
        take(k, v, f"randn ({H},{W}) x{s} C={C} scalar")
    return worst
