"""Shared cases of the bf16 normalisation kernels' tests (openess_amd/csrc/norm_ops.hip: statistics, finalize, apply, InstanceNorm
backward, BatchNorm backward on its fused and three-launch routes, the one-launch tile-stats route, the nearest x2 / zero-insert /
2x2-sum copies; tests/test_hip_norm_routes.py on the GPU, tests/test_norm_cases.py on the CPU) and of the CPU measurement that
sets their bounds (tools/exp_norm_bounds.py):

  * norm_route restates the dispatch arithmetic of the file; every case records the route it must take;
  * float64 references of every operation on the bf16 / fp32 operands;
  * fp32 CPU models of the kernels' rounding points, written from the comments and the code of norm_ops.hip and not by calling
    it: they prove that the exact cases are exact for a correct implementation, measure how far correct fp32 arithmetic sits from
    float64, and take the seven mutations the CPU test holds the criteria against;
  * layout helpers that put an operand into a channel slice of a wider NaN-filled buffer;
  * exact integer data whose every sum is below 2^24 (asserted in int64), and four non-exact families.

Nothing here needs a GPU."""
import functools
import math

import torch

SEED = 5309
THREADS = 256
EPS = float(torch.tensor(1e-5, dtype=torch.float32))      # the fp32 value the entries receive
MOMENTUM = 0.1
LIMIT = 1 << 24                                           # integers below it are exact in fp32, in any order of addition
FAMILIES = ("randn", "large_mean", "constant", "single")
LAYOUTS = {"dense": (0, 0), "slice8": (8, 8), "slice24": (8, 24)}      # name -> (c0, extra columns): pixel stride C + extra
MUTATIONS = ("drop_last_pixel", "strided_as_dense", "no_group_offset", "gamma_i", "biased_running_var", "mask_from_xhat",
             "ppg_plus_1")
BOUNDED_MAX_PIXELS = 33000

# ---- cases: (name, G, ppg, C, layouts, route it must take).  Each is the smallest shape at which its branch is entered.
FWD_CASES = (
    ("one_pixel", 1, 1, 8, ("dense", "slice8"), dict(chunks=1, ppw=1, rows=256, idle=0, unrolled=False, tail=True, empty_chunks=0)),
    ("cl3_tail_only", 1, 63, 24, ("dense", "slice24"), dict(chunks=1, ppw=63, rows=85, idle=1, unrolled=False, tail=True)),
    ("cl9_x4_once", 8, 3000, 72, ("dense", "slice8"), dict(chunks=32, ppw=94, rows=28, idle=4, unrolled=True, unrolled_trips=1)),
    ("rows1_writeout", 1, 120, 2048, ("dense", "slice8"), dict(chunks=2, ppw=60, rows=1, idle=0, writeout_trips=8, unrolled=True)),
    ("empty_chunks", 1, 16385, 8, ("dense", "slice24"), dict(chunks=256, ppw=65, rows=256, empty_chunks=3, last_chunk=5, unrolled=False)),
    ("c64_x4_tail", 1, 32805, 64, ("dense", "slice8"), dict(chunks=256, ppw=129, rows=32, unrolled=True, unrolled_trips=1, tail=True)),
    ("rows256_x4", 1, 262149, 8, ("dense", "slice24"), dict(chunks=256, ppw=1025, rows=256, unrolled=True, unrolled_trips=1, tail=True)),
    ("groups_affine", 3, 130, 72, ("dense", "slice8"), dict(chunks=3, ppw=44, rows=28, idle=4, unrolled=False)),
)
CAP_CASE = ("apply_cap", 1, 32769, 2048, ("dense",), dict(rows=1, apply_gx=8192, apply_capped=True))      # GPU only: 134 MB
BN_FUSED_PIXELS = {37: 1, 1024: 16, 1050: 17, 4130: 65, 33000: 512}      # pixels -> partial rows
BN_BWD_CASES = tuple(("bn_fused", 1, P, C, ("dense", "slice8"), dict(fused=True, chunks=rows_)) for C in (64, 256)
                     for P, rows_ in BN_FUSED_PIXELS.items()) + \
    tuple(("bn_three", 1, P, C, ("dense", "slice24"), dict(fused=False)) for C in (24, 72, 200) for P in (37, 1050))
IN_BWD_CASES = (("in_x2", 8, 3000, 72, ("dense", "slice8"), dict(chunks=47, ppw=64, rows=28, unrolled=True)),
                ("in_tail_only", 2, 63, 24, ("dense", "slice24"), dict(chunks=1, ppw=63, rows=85, unrolled=False, tail=True)),
                ("in_c64", 3, 1050, 64, ("dense", "slice8"), dict(chunks=17, ppw=62, rows=32, unrolled=True)))
TILE_COUNTS = (1, 15, 16, 17, 70, 512)
TILE_CASES = tuple(("tile", 1, 128 * t - 37, C, ("dense", "slice8"), dict(tiles=t, tile_trips=(t + 15) // 16)) for C in (64, 256)
                   for t in TILE_COUNTS)
# the wrappers take a [B, C, H, W] tensor: B H W of the cases they run (kind, B, H, W, C)
WRAPPER_CASES = (("in", 8, 50, 60, 72), ("in", 2, 7, 9, 24), ("bn", 2, 21, 25, 72), ("bn", 2, 21, 25, 64), ("bn", 1, 1, 37, 24))
COPY_CASES = ((1, 1, 1, 8), (2, 3, 5, 24), (1, 7, 9, 72), (3, 5, 3, 64))          # (B, H, W, C): odd H and W
ZERO_INSERT = ((2, 0, 0), (2, 1, 2), (3, 0, 0), (3, 2, 1))                        # (stride, extra Hz, extra Wz)

# ---- bounds: four times the largest figure of the fp32 models against float64 over the families and the cases up to
# BOUNDED_MAX_PIXELS (tools/exp_norm_bounds.py prints them; DESIGN.md carries them; tests/test_norm_cases.py re-measures them).
# The measures are the err_* functions below; each is a distance normalised by the natural scale of the quantity.
MODEL_FIGURE = {
    "mean": 5.94e-8,        # large_mean, forward (8, 3000, 72)
    "rstd": 1.27e-7,        # randn, forward (1, 120, 2048)
    "y": 1.24e-7,           # large_mean, tile-stats (1, 2011, 64)
    "s1": 1.95e-8,          # large_mean, BatchNorm backward (1, 37, 24)
    "s2": 3.49e-7,          # single, BatchNorm backward (1, 37, 64)
    "dx": 9.03e-8,          # single, BatchNorm backward (1, 37, 72)
    "s2_chain": 1.66e-7,    # single, BatchNorm backward (1, 37, 64)
    "dx_chain": 6.15e-8,    # randn, BatchNorm backward (1, 1024, 256)
}
BOUND = {k: 4.0 * v for k, v in MODEL_FIGURE.items()}
RUNNING_MEAN_RTOL, RUNNING_VAR_RTOL = 2e-7, 1e-6          # what tests/test_hip_determinism.py holds the same finalize_one to
RSTD_ULPS = 2                                             # sqrt and divide in double, one cast; the second ulp covers a tie


def cdiv(a, b):
    return (a + b - 1) // b


def _gen(*key):
    h = SEED
    for k in key:
        for ch in str(k):
            h = (h * 1000003 + ord(ch)) % (1 << 31)
    return torch.Generator().manual_seed(h)


# --------------------------------------------------------------------------------------------- dispatch, restated
def stats_chunks(ppg, G, target):
    return max(1, min(cdiv(target, G), cdiv(ppg, 64)))


def stats_route(G, ppg, C, backward=False):
    """launch_stats + stats_kernel<MODE>: grid (chunks, G); cl = C / 8 lanes per pixel, rows = 256 / cl pixels in flight;
    MODE 0 unrolls by 4 (entered when p + 3 rows < p_end), MODE 1 by 2 (p + rows < p_end), then a tail loop"""
    assert C % 8 == 0 and 8 <= C <= 2048
    cl = C // 8
    rows = THREADS // cl
    chunks = stats_chunks(ppg, G, 512 if backward else 256)
    ppw = cdiv(ppg, chunks)
    nonempty = cdiv(ppg, ppw)
    last = ppg - (nonempty - 1) * ppw
    unroll = 2 if backward else 4
    trips, tail = 0, False
    for n in {min(ppw, ppg), last}:
        for row in range(rows):
            p, t = row, 0
            while p + (unroll - 1) * rows < n:
                p += unroll * rows
                t += 1
            trips = max(trips, t)
            tail = tail or p < n
    return dict(chunks=chunks, ppw=ppw, rows=rows, idle=THREADS - rows * cl, unrolled=trips > 0, unrolled_trips=trips, tail=tail,
                empty_chunks=chunks - nonempty, last_chunk=last, writeout_trips=cdiv(C, THREADS))


def apply_grid(ppg, G, C):
    rows = THREADS // (C // 8)
    gx = cdiv(ppg, rows * 4)
    cap = cdiv(8192, G)
    return dict(apply_gx=max(1, min(gx, cap)), apply_capped=gx > cap)


def _pixel_chunks(pixels, C, target):
    groups = C // 64
    ch = max(1, min(cdiv(target, groups), cdiv(pixels, 128)))
    ppc = cdiv(cdiv(pixels, ch), 32) * 32
    ch = cdiv(pixels, ppc)
    return dict(groups=groups, pixel_chunks=ch, ppc=ppc, last_pixel_chunk=pixels - (ch - 1) * ppc)


def norm_route(kind, G, ppg, C, tiles=None):
    """kind: 'fwd' (statistics + finalize + apply), 'in_bwd', 'bn_bwd' (G = 1), 'tile' (oess_norm_tile_stats_apply_nhwc_bf16)"""
    if kind == "fwd":
        return dict(stats_route(G, ppg, C), **apply_grid(ppg, G, C))
    if kind == "in_bwd":
        return dict(stats_route(G, ppg, C, backward=True), **apply_grid(ppg, G, C))
    if kind == "bn_bwd":
        assert G == 1
        r = stats_route(1, ppg, C, backward=True)
        r["fused"] = C % 64 == 0 and r["chunks"] <= 512
        r.update(_pixel_chunks(ppg, C, 2048) if r["fused"] else apply_grid(ppg, 1, C))
        return r
    assert kind == "tile" and G == 1 and C % 64 == 0 and 1 <= tiles <= 512
    return dict(_pixel_chunks(ppg, C, 1024), tiles=tiles, tile_trips=cdiv(tiles, 16))


def case_kind(name):
    return {"bn_fused": "bn_bwd", "bn_three": "bn_bwd", "tile": "tile"}.get(name, "in_bwd" if name.startswith("in_") else "fwd")


def all_cases():
    return FWD_CASES + (CAP_CASE,) + BN_BWD_CASES + IN_BWD_CASES + TILE_CASES


def route_of_case(case):
    name, G, ppg, C, _, expect = case
    return norm_route(case_kind(name), G, ppg, C, tiles=expect.get("tiles"))


REQUIRED_BRANCHES = frozenset((
    "fwd_x4", "fwd_x4_not", "fwd_tail", "fwd_empty_chunks", "fwd_idle_threads", "fwd_rows1_writeout", "fwd_one_pixel", "fwd_groups",
    "apply_cap", "apply_cap_not", "bwd_x2", "bwd_x2_not", "bwd_tail", "bwd_groups", "bn_fused", "bn_three",
    "bn_fused_rows_1", "bn_fused_rows_16", "bn_fused_rows_17", "bn_fused_rows_gt64", "bn_fused_rows_512", "bn_fused_partial_last_chunk",
    "bn_fused_many_chunks", "tile_trips_1", "tile_trips_2", "tile_trips_gt4", "tile_trips_32", "tile_partial_last_chunk",
    "tile_many_chunks"))


def branches(case):
    """names of REQUIRED_BRANCHES this case enters, from norm_route"""
    name, G, ppg, C, _, _ = case
    kind, r = case_kind(name), route_of_case(case)
    out = set()
    if kind == "fwd":
        out.add("fwd_x4" if r["unrolled"] else "fwd_x4_not")
        out.update(k for k, on in (("fwd_tail", r["tail"]), ("fwd_empty_chunks", r["empty_chunks"] > 0), ("fwd_idle_threads", r["idle"] > 0),
                                   ("fwd_rows1_writeout", r["rows"] == 1 and r["writeout_trips"] > 1), ("fwd_one_pixel", ppg == 1),
                                   ("fwd_groups", G > 1)) if on)
        out.add("apply_cap" if r["apply_capped"] else "apply_cap_not")
    elif kind in ("in_bwd", "bn_bwd"):
        out.add("bwd_x2" if r["unrolled"] else "bwd_x2_not")
        out.update(k for k, on in (("bwd_tail", r["tail"]), ("bwd_groups", G > 1)) if on)
        if kind == "bn_bwd":
            out.add("bn_fused" if r["fused"] else "bn_three")
            if r["fused"]:
                n = r["chunks"]
                out.update(k for k, on in (("bn_fused_rows_1", n == 1), ("bn_fused_rows_16", n == 16), ("bn_fused_rows_17", n == 17),
                                           ("bn_fused_rows_gt64", n > 64), ("bn_fused_rows_512", n == 512),
                                           ("bn_fused_partial_last_chunk", r["last_pixel_chunk"] % 32 != 0),
                                           ("bn_fused_many_chunks", r["pixel_chunks"] > 1)) if on)
    else:
        t = r["tile_trips"]
        out.update(k for k, on in (("tile_trips_1", t == 1), ("tile_trips_2", t == 2), ("tile_trips_gt4", t > 4), ("tile_trips_32", t == 32),
                                   ("tile_partial_last_chunk", r["last_pixel_chunk"] % 32 != 0), ("tile_many_chunks", r["pixel_chunks"] > 1))
                   if on)
    return out


# --------------------------------------------------------------------------------------------- layouts
def place(t, layout, device="cpu", fill=math.nan):
    """t [G, P, C] as the channel slice [c0 : c0 + C] of a [G P, C + extra] buffer filled with `fill`: (buffer, view [G, P, C]).
    The view's pixel stride is C + extra, c0 and the stride are multiples of 8 (16-byte accesses stay aligned)."""
    c0, extra = LAYOUTS[layout]
    G, P, C = t.shape
    buf = torch.full((G * P, C + extra), fill, dtype=t.dtype, device=device)
    view = buf[:, c0:c0 + C].view(G, P, C)
    view.copy_(t.to(device))
    return buf, view


def place_out(shape, dtype, layout, device="cpu"):
    """an output buffer of NaN: (buffer, view)"""
    return place(torch.full(shape, math.nan, dtype=dtype), layout, device)


def surroundings_untouched(buf, layout, C):
    """everything outside the slice still holds NaN"""
    c0, _ = LAYOUTS[layout]
    return bool(torch.isnan(buf[:, :c0]).all()) and bool(torch.isnan(buf[:, c0 + C:]).all())


def layout_stride(layout, C):
    """pixel stride (elements) of a [.., C] operand placed by `layout`"""
    return C + LAYOUTS[layout][1]


def kernel_view(buf, view, mutate=None):
    """what a kernel reads as operand [G, P, C]: the view itself; 'strided_as_dense' reads with pixel stride C from the view's first
    element, 'no_group_offset' reads group 0 for every group"""
    G, P, C = view.shape
    if mutate == "strided_as_dense":
        return buf.reshape(-1)[view.storage_offset() - buf.storage_offset():][:G * P * C].view(G, P, C)
    if mutate == "no_group_offset":
        return view[:1].expand(G, P, C)
    return view


# --------------------------------------------------------------------------------------------- data
def _bf16_values(shape, g):
    """random bf16 values with 0.5 <= |v| < 4, never zero"""
    mant = torch.randint(128, 256, shape, generator=g).double() / 128.0
    exp = torch.randint(-1, 2, shape, generator=g).double()
    sign = torch.randint(0, 2, shape, generator=g).double() * 2.0 - 1.0
    v = sign * mant * torch.pow(torch.tensor(2.0, dtype=torch.float64), exp)
    assert bool((v.bfloat16().double() == v).all())
    return v


def _pick(values, shape, g):
    return torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), shape, generator=g)]


def _exact_bf16(v):
    b = v.bfloat16()
    assert bool((b.double() == v.double()).all()), "not bf16-exact"
    return b


@functools.lru_cache(maxsize=4)
def exact_forward(G, ppg, C):
    """x: integers |v| <= 8.  scale: +-2^k (k = -2 .. 1) and shift: integers |v| <= 4 per (group, channel), residual: integers
    |v| <= 8.  Every sum and sum of squares is below 2^24 (int64), x scale + shift (+ residual) is bf16-exact (asserted)."""
    g = _gen("exact_forward", G, ppg, C)
    xi = torch.randint(-8, 9, (G, ppg, C), generator=g)
    S, Q = xi.sum(1), (xi * xi).sum(1)
    assert int(xi.abs().sum(1).max()) < LIMIT and int(Q.max()) < LIMIT
    scale = _pick((0.25, 0.5, 1.0, 2.0, -0.25, -0.5, -1.0, -2.0), (G, C), g)
    shift = torch.randint(-4, 5, (G, C), generator=g).double()
    ri = torch.randint(-8, 9, (G, ppg, C), generator=g)
    lin = xi.double() * scale[:, None] + shift[:, None]
    y = {(relu, res): _exact_bf16((lin + (ri.double() if res else 0.0)).clamp_min(0.0 if relu else -math.inf))
         for relu in (False, True) for res in (False, True)}
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.1
    return dict(x=_exact_bf16(xi.double()), S=S, Q=Q, scale=scale.float(), shift=shift.float(), res=_exact_bf16(ri.double()), y=y,
                gamma=gamma, beta=beta, G=G, ppg=ppg, C=C)


@functools.lru_cache(maxsize=4)
def exact_backward(G, ppg, C, with_yout):
    """x: integers |v| <= 8, dy: integers |v| <= 4, mean: integers |v| <= 2, rstd and |gamma|: powers of two.  xhat and g xhat are
    exact, s1 = sum g and s2 = sum g xhat are exact while sum |g| and sum |g (x - mean)| stay below 2^24 (int64).  y_out (when
    given) holds +0, -0, negative and positive entries independent of x: the mask is y_out > 0 and nothing else.  Without it the
    mask is xhat > 0, and x equals the mean at about one pixel in 17."""
    g = _gen("exact_backward", G, ppg, C, with_yout)
    xi = torch.randint(-8, 9, (G, ppg, C), generator=g)
    di = torch.randint(-4, 5, (G, ppg, C), generator=g)
    mean = torch.randint(-2, 3, (G, C), generator=g)
    rstd = _pick((0.25, 0.5, 1.0), (G, C), g)
    gamma = _pick((0.5, 1.0, 2.0, -0.5, -1.0, -2.0), (C,), g)
    yout = _exact_bf16(_pick((0.0, -0.0, -1.5, -0.25, 2.0, 0.0078125), (G, ppg, C), g)) if with_yout else None
    dev = xi - mean[:, None]
    if not with_yout:
        assert bool((dev == 0).any())
    out = dict(x=_exact_bf16(xi.double()), dy=_exact_bf16(di.double()), mean=mean.float(), rstd=rstd.float(), gamma=gamma.float(),
               yout=yout, G=G, ppg=ppg, C=C)
    for relu in (False, True):
        if relu:
            mask = (yout.double() > 0) if with_yout else (dev > 0)
            if with_yout:
                assert bool(mask[yout.double() == 0].logical_not().all()) and bool(((yout.double() > 0) != (dev > 0)).any())
        else:
            mask = torch.ones_like(xi, dtype=torch.bool)
        gm = di * mask
        assert int(gm.abs().sum(1).max()) < LIMIT and int((gm * dev).abs().sum(1).max()) < LIMIT
        out[relu] = dict(s1=gm.sum(1).double(), s2=(gm * dev).sum(1).double() * rstd, dres=_exact_bf16(gm.double()))
    return out


def family_inputs(family, G, ppg, C):
    """bf16 x [G, ppg, C] of a family, with dy and a residual (randn), fp32 gamma in [0.5, 1.5) and beta ~ 0.1 randn"""
    g = _gen("family", family, G, ppg, C)
    if family == "randn":                                 # N(0.5, 2)
        x = 0.5 + 2.0 * torch.randn(G, ppg, C, generator=g)
    elif family == "large_mean":                          # mean 8, spread 0.1: bf16 steps of 1/16 up there, E[x^2] is 6400 variances
        x = 8.0 + 0.1 * torch.randn(G, ppg, C, generator=g)
    elif family == "constant":                            # variance 0: rstd = 1 / sqrt(eps)
        x = _bf16_values((G, 1, C), g).float().expand(G, ppg, C)
    elif family == "single":                              # one non-zero element per (group, channel)
        x = torch.zeros(G, ppg, C)
        pos = torch.randint(0, ppg, (G, 1, C), generator=g)
        x.scatter_(1, pos, _bf16_values((G, 1, C), g).float())
    else:
        raise ValueError(family)
    return dict(x=x.bfloat16().contiguous(), dy=torch.randn(G, ppg, C, generator=g).bfloat16(),
                res=torch.randn(G, ppg, C, generator=g).bfloat16(), gamma=torch.rand(C, generator=g) + 0.5,
                beta=torch.randn(C, generator=g) * 0.1, G=G, ppg=ppg, C=C)


def tile_partials(x, tiles):
    """per-tile (sum, sum of squares) [tiles, 2, C] in fp32 of x [1, P, C]: what a convolution epilogue hands over.  Tile t holds
    pixels 128 t .. 128 t + 127; the values are the float64 sums rounded once, and they are the operands of the tile-stats entry
    (its references start from them)."""
    _, P, C = x.shape
    assert cdiv(P, 128) == tiles
    xd = torch.cat([x[0].double(), torch.zeros(tiles * 128 - P, C, dtype=torch.float64)]).view(tiles, 128, C)
    return torch.stack([xd.sum(1), (xd * xd).sum(1)], dim=1).float().contiguous()


# --------------------------------------------------------------------------------------------- float64 references
def moments64(x=None, partials=None, count=None):
    """mean, biased variance, E[x^2] per (group, channel) in float64, from x [G, P, C] or from tile partials [tiles, 2, C]"""
    if partials is not None:
        s = partials.double().sum(0)
        mean, ex2 = s[0][None] / count, s[1][None] / count
        return mean, (ex2 - mean * mean).clamp_min(0.0), ex2
    xd = x.double()
    mean = xd.mean(1)
    return mean, ((xd - mean[:, None]) ** 2).mean(1), (xd * xd).mean(1)


def forward64(x, gamma=None, beta=None, eps=EPS, res=None, relu=False, partials=None):
    """BatchNorm (G = 1) / InstanceNorm forward in float64 on the bf16 operands: mean, var, ex2, rstd, scale, shift [G, C], y and
    its natural scale (|x| + |mean|) |scale| + |beta| + |residual| [G, P, C]"""
    G, P, C = x.shape
    mean, var, ex2 = moments64(x, partials, float(P))
    rstd = 1.0 / torch.sqrt(var + eps)
    ga = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    be = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    scale, shift = ga * rstd, be - mean * ga * rstd
    xd = x.double()
    y = (xd - mean[:, None]) * scale[:, None] + be
    mag = (xd.abs() + mean.abs()[:, None]) * scale.abs()[:, None] + be.abs()
    if res is not None:
        y, mag = y + res.double(), mag + res.double().abs()
    if relu:
        y = y.clamp_min(0.0)
    return dict(mean=mean, var=var, ex2=ex2, rstd=rstd, scale=scale, shift=shift, y=y, y_scale=mag)


def running64(mean, var, count, rm0, rv0, momentum=MOMENTUM):
    """nn.BatchNorm2d's update: the running variance takes the UNBIASED estimate (the biased one when count == 1)"""
    unb = var * count / (count - 1.0) if count > 1 else var
    return (1.0 - momentum) * rm0.double() + momentum * mean[0], (1.0 - momentum) * rv0.double() + momentum * unb[0]


def running_tolerances(f64, count):
    """(atol of running_mean, atol of running_var) on top of the two relative tolerances when the statistics are bounded and not
    exact: momentum times the bound of the mean (in units of the rms), and of the variance -- d var = 2 (var + eps) d rstd / rstd
    <= 2 BOUND['rstd'] E[x^2] by the rstd measure, times count / (count - 1) <= 2"""
    return (MOMENTUM * BOUND["mean"] * float(f64["ex2"].sqrt().max()), MOMENTUM * 4.0 * BOUND["rstd"] * float(f64["ex2"].max()))


def backward64(x, dy, mean, rstd, gamma=None, relu=False, yout=None):
    """g = dy mask; s1 = sum g; s2 = sum g xhat; dx = gamma rstd (g - s1 / N - xhat s2 / N); d(residual) = g, in float64.  mean and
    rstd [G, C] are operands.  The mask comes from the stored y_out where one is given, else from xhat > 0.  Also the natural
    scales: sum |g|, sum |g xhat|, and |gamma rstd| (|g| + sum|g| / N + |xhat| sum|g xhat| / N) for dx."""
    G, P, C = x.shape
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    xh = (x.double() - mu) * rs
    g = dy.double()
    if relu:
        g = torch.where((yout.double() > 0) if yout is not None else (xh > 0), g, torch.zeros((), dtype=torch.float64))
    s1, s2 = g.sum(1), (g * xh).sum(1)
    a1, a2 = g.abs().sum(1), (g * xh).abs().sum(1)
    gr = rs if gamma is None else gamma.double() * rs
    dx = gr * (g - s1[:, None] / P - xh * s2[:, None] / P)
    dx_scale = gr.abs() * (g.abs() + a1[:, None] / P + xh.abs() * a2[:, None] / P)
    return dict(s1=s1, s2=s2, s1_scale=a1, s2_scale=a2, dx=dx, dx_scale=dx_scale, dres=g)


def upsample2x_ref(t):
    """[B, H, W, C] -> [B, 2H, 2W, C] by indexing"""
    return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def zero_insert_ref(t, s, Hz, Wz):
    B, H, W, C = t.shape
    z = torch.zeros(B, Hz, Wz, C, dtype=t.dtype, device=t.device)
    z[:, :(H - 1) * s + 1:s, :(W - 1) * s + 1:s] = t
    return z


def downsample_sum2x_ref(t):
    """[B, 2H, 2W, C] -> [B, H, W, C]: the float64 sum of each 2x2 block rounded once to bf16"""
    B, H2, W2, C = t.shape
    return t.double().view(B, H2 // 2, 2, W2 // 2, 2, C).sum(dim=(2, 4)).bfloat16()


def copy_values(B, H, W, C, key):
    """bf16 [B, H, W, C] with 0.5 <= |v| < 4: a sum of four is exact in fp32 (multiples of 2^-8 below 16)"""
    return _bf16_values((B, H, W, C), _gen("copy", B, H, W, C, key)).bfloat16()


# --------------------------------------------------------------------------------------------- error measures
_TINY = 1e-300


def ulp_bf16(ref):
    """spacing of bf16 at |ref| (float64 tensor); 0 at 0"""
    a = ref.abs()
    e = torch.floor(torch.log2(a.clamp_min(_TINY)))
    return torch.where(a > 0, torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7.0), torch.zeros((), dtype=torch.float64))


def err_fp32(got, ref, scale):
    """largest |got - ref64| / scale"""
    return float(((got.double().cpu() - ref).abs() / scale.clamp_min(_TINY)).max())


def err_bf16(got, ref, scale):
    """largest max(0, |got - ref64| - ulp_bf16(ref64) / 2) / scale: a correct kernel rounds an almost-right fp32 value once"""
    d = ((got.double().cpu() - ref).abs() - 0.5 * ulp_bf16(ref)).clamp_min(0.0)
    return float((d / scale.clamp_min(_TINY)).max())


def err_mean(mean, f):
    return err_fp32(mean, f["mean"], torch.sqrt(f["ex2"]))


def err_rstd(rstd, f, eps=EPS):
    """|rstd - ref| / ref in units of E[x^2] / (var + eps): d rstd / rstd = -dvar / (2 (var + eps)), and the variance is a
    difference of two terms of size E[x^2] whose fp32 partial sums carry the rounding"""
    return err_fp32(rstd, f["rstd"], f["rstd"] * f["ex2"] / (f["var"] + eps))


def chain_condition(f, eps=EPS):
    """>= 1: how much an error of the statistics grows on its way into xhat"""
    return (1.0 + f["ex2"] / (f["var"] + eps))[:, None]


def ulps_fp32(got, ref):
    """largest |got - ref64| in units of the fp32 spacing at |ref64|"""
    e = torch.floor(torch.log2(ref.abs().clamp_min(_TINY)))
    return float(((got.double().cpu() - ref).abs() / torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 23.0)).max())


def finalize_bounds(f, gamma, beta):
    """absolute bounds on scale and shift [G, C] for exact sums (mean is then the correctly rounded quotient and rstd within
    RSTD_ULPS ulps).  u = 2^-24.  scale = gamma rstd: rstd's 2 ulps (4u) and one product rounding.  shift = beta - mean gamma rstd:
    the rounded mean (u), two products (2u) and rstd (4u) on |mean gamma rstd|, and the subtraction's rounding of the result."""
    u = 2.0 ** -24
    G, C = f["mean"].shape
    ga = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    be = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    mgr = (f["mean"] * ga * f["rstd"]).abs()
    return 5.0 * u * f["scale"].abs(), u * (8.0 * mgr + 2.0 * (f["shift"].abs() + be.abs()))


# --------------------------------------------------------------------------------------------- fp32 models
def _lane_sum(parts):
    """partials_reduce_kernel / bn_bwd_reduce_apply_kernel / tile_stats_apply_kernel: rows [T, N] added in double by 16 lanes (lane
    tl takes rows tl, tl + 16, ... in order), then the lane sums 0 .. 15 in order"""
    T, N = parts.shape
    n = cdiv(T, 16)
    p = torch.cat([parts.double(), torch.zeros(n * 16 - T, N, dtype=torch.float64)]).view(n, 16, N)
    lane = torch.zeros(16, N, dtype=torch.float64)
    for i in range(n):
        lane = lane + p[i]
    s = lane[0].clone()
    for k in range(1, 16):
        s = s + lane[k]
    return s


def stats_model(x, dy=None, mean=None, rstd=None, relu=False, yout=None, mutate=None):
    """stats_kernel<0> (dy is None: sums of x and x^2) / stats_kernel<1> (s1 = sum g, s2 = sum g xhat) followed by the fixed-order
    reduction: thread (row, lane) of chunk k accumulates pixels p_beg + row + j rows in fp32 in order of j, the rows are added
    0 .. rows - 1 in fp32, the chunk rows in double.  Returns the double totals [G, C] (the backward entries store them as fp32).
    mutate 'drop_last_pixel': every chunk stops one pixel early; 'mask_from_xhat': the mask ignores y_out."""
    G, P, C = x.shape
    backward = dy is not None
    r = stats_route(G, P, C, backward)
    chunks, ppw, rows = r["chunks"], r["ppw"], r["rows"]
    J = cdiv(ppw, rows)
    ch, j, row = torch.arange(chunks)[:, None, None], torch.arange(J)[None, :, None], torch.arange(rows)[None, None, :]
    p = ch * ppw + row + j * rows
    p_end = ((ch + 1) * ppw).clamp(max=P) - (1 if mutate == "drop_last_pixel" else 0)
    valid = (p < p_end)[..., None]
    pc = p.clamp(max=P - 1)
    zero = torch.zeros((), dtype=torch.float32)
    out = torch.empty(2, G, C, dtype=torch.float64)
    for g in range(G):
        v = x[g].float()[pc]                                               # [chunks, J, rows, C]
        if backward:
            xh = (v - mean[g].float()) * rstd[g].float()
            gg = dy[g].float()[pc]
            if relu:
                keep = (yout[g].float()[pc] > 0) if (yout is not None and mutate != "mask_from_xhat") else (xh > 0)
                gg = torch.where(keep, gg, zero)
            t1, t2 = gg, gg * xh
        else:
            t1, t2 = v, v * v
        a1, a2 = torch.zeros(chunks, rows, C), torch.zeros(chunks, rows, C)
        for jj in range(J):
            a1 = a1 + torch.where(valid[:, jj], t1[:, jj], zero)
            a2 = a2 + torch.where(valid[:, jj], t2[:, jj], zero)
        s1, s2 = torch.zeros(chunks, C), torch.zeros(chunks, C)
        for rr in range(rows):
            s1 = s1 + a1[:, rr]
            s2 = s2 + a2[:, rr]
        out[0, g], out[1, g] = _lane_sum(s1), _lane_sum(s2)
    return out[0], out[1]


def finalize_model(S, Q, count, eps=EPS, gamma=None, beta=None, running=None, momentum=MOMENTUM, mutate=None):
    """finalize_one as written: mean and the biased variance in double (clamped at 0), rstd = (float)(1 / sqrt(var + eps)),
    scale = gamma rstd and shift = beta - (float)mean gamma rstd in fp32, the running statistics (G == 1) in fp32 with the unbiased
    variance.  mutate 'gamma_i': gamma and beta indexed by i = g C + c (NaN stands for whatever lies behind the C values);
    'biased_running_var'."""
    G, C = S.shape
    f32 = torch.float32
    cnt = float(torch.tensor(float(count), dtype=f32))
    m = S / cnt
    var = (Q / cnt - m * m).clamp_min(0.0)
    r = (1.0 / torch.sqrt(var + float(eps))).to(f32)
    ga = torch.ones(C, dtype=f32) if gamma is None else gamma.to(f32)
    be = torch.zeros(C, dtype=f32) if beta is None else beta.to(f32)
    if mutate == "gamma_i" and gamma is not None:
        pad = torch.full(((G - 1) * C,), math.nan, dtype=f32)
        ga, be = torch.cat([ga, pad]).view(G, C), torch.cat([be, pad]).view(G, C)
    m32 = m.to(f32)
    scale = ga * r
    shift = be - m32 * ga * r
    out = dict(mean=m32, rstd=r, scale=scale, shift=shift)
    if running is not None and G == 1:
        rm, rv = running
        unb = (var * cnt / (cnt - 1.0) if cnt > 1 and mutate != "biased_running_var" else var).to(f32)[0]
        mom = torch.tensor(momentum, dtype=f32)
        out["running_mean"] = (1.0 - mom) * rm.to(f32) + mom * m32[0]
        out["running_var"] = (1.0 - mom) * rv.to(f32) + mom * unb
    return out


def apply_model(x, scale, shift, res=None, relu=False):
    """apply_kernel / the apply half of tile_stats_apply_kernel: x scale + shift (+ residual) in fp32, ReLU, one RNE rounding"""
    f = x.float() * scale.float()[:, None] + shift.float()[:, None]
    if res is not None:
        f = f + res.float()
    if relu:
        f = f.clamp_min(0.0)
    return f.bfloat16()


def bwd_apply_model(x, dy, mean, rstd, s1, s2, relu=False, gamma=None, yout=None, mutate=None):
    """in_bwd_apply_kernel / the apply half of bn_bwd_reduce_apply_kernel: a1 = s1 (1.0f / ppg), a2 likewise, gr = gamma rstd,
    dx = gr (g - a1 - xhat a2) in fp32, one RNE rounding; d(residual) = g.  s1 and s2 are the fp32 sums.
    mutate 'ppg_plus_1': 1 / (ppg + 1); 'mask_from_xhat'."""
    G, P, C = x.shape
    f32 = torch.float32
    invn = torch.tensor(1.0, dtype=f32) / torch.tensor(float(P + (1 if mutate == "ppg_plus_1" else 0)), dtype=f32)
    mu, rs = mean.to(f32)[:, None], rstd.to(f32)[:, None]
    a1, a2 = (s1.to(f32) * invn)[:, None], (s2.to(f32) * invn)[:, None]
    gr = rs if gamma is None else gamma.to(f32) * rs
    xh = (x.float() - mu) * rs
    gg = dy.float()
    if relu:
        keep = (yout.float() > 0) if (yout is not None and mutate != "mask_from_xhat") else (xh > 0)
        gg = torch.where(keep, gg, torch.zeros((), dtype=f32))
    return (gr * (gg - a1 - xh * a2)).bfloat16(), gg.bfloat16()


def forward_model(x, gamma=None, beta=None, eps=EPS, res=None, relu=False, running=None, mutate=None, partials=None):
    """statistics -> finalize -> apply, as oess_norm_stats_finalize_nhwc_bf16 + oess_norm_apply_nhwc_bf16 chain them (or, with
    tile partials, as tile_stats_apply_kernel does in one launch)"""
    G, P, C = x.shape
    if partials is not None:
        S, Q = _lane_sum(partials[:, 0])[None], _lane_sum(partials[:, 1])[None]
    else:
        S, Q = stats_model(x, mutate=mutate)
    f = finalize_model(S, Q, P, eps, gamma, beta, running, mutate=mutate)
    f["S"], f["Q"] = S, Q
    f["y"] = apply_model(x, f["scale"], f["shift"], res, relu)
    return f


def backward_model(x, dy, mean, rstd, relu=False, gamma=None, yout=None, mutate=None):
    """stats_kernel<1> -> fixed-order reduction (stored as fp32) -> apply, on either BatchNorm route (they are bit-identical) and
    through oess_instnorm_bwd_nhwc_bf16"""
    S1, S2 = stats_model(x, dy, mean, rstd, relu, yout, mutate)
    s1, s2 = S1.float(), S2.float()
    dx, dres = bwd_apply_model(x, dy, mean, rstd, s1, s2, relu, gamma, yout, mutate)
    return dict(s1=s1, s2=s2, dx=dx, dres=dres)


# --------------------------------------------------------------------------------------------- the measurement
def bounded_cases():
    """(kind, name, G, ppg, C, tiles) of every case the bounded tests run: the cases above up to BOUNDED_MAX_PIXELS"""
    out = []
    for case in FWD_CASES + BN_BWD_CASES + IN_BWD_CASES + TILE_CASES:
        name, G, ppg, C, _, expect = case
        if ppg <= BOUNDED_MAX_PIXELS:
            out.append((case_kind(name), name, G, ppg, C, expect.get("tiles")))
    return out


def fp32_stats_of(x):
    """mean and rstd [G, C] in fp32 the way a forward leaves them for a backward: float64 statistics rounded once"""
    f = forward64(x)
    return f["mean"].float(), f["rstd"].float()


def forward_figures(got, f64):
    """the bounded measures of a forward result `got` (dict with mean, rstd, y) against forward64's dict"""
    return dict(mean=err_mean(got["mean"], f64), rstd=err_rstd(got["rstd"], f64), y=err_bf16(got["y"], f64["y"], f64["y_scale"]))


def backward_figures(got, b64, cond=None):
    """the bounded measures of a backward result (s1, s2, dx); with cond (chain_condition: the statistics came from the kernels
    and the reference's from float64) s2 and dx are measured in units of it, as 's2_chain' and 'dx_chain'"""
    out = dict(s1=err_fp32(got["s1"], b64["s1"], b64["s1_scale"]), s2=err_fp32(got["s2"], b64["s2"], b64["s2_scale"]))
    if cond is None:
        out["dx"] = err_bf16(got["dx"], b64["dx"], b64["dx_scale"])
    else:
        out["s2_chain"] = err_fp32(got["s2"], b64["s2"], b64["s2_scale"] * cond[:, 0])
        out["dx_chain"] = err_bf16(got["dx"], b64["dx"], b64["dx_scale"] * cond)
        del out["s2"]
    return out


def chain_case_ok(family, relu, yout_given):
    """the whole-chain backward (statistics from the kernel, float64 reference from x) has no defined answer where the ReLU mask
    is xhat > 0 and xhat is 0 up to rounding at every pixel: the constant family without a stored output"""
    return not (family == "constant" and relu and not yout_given)


def model_figures(kind, G, ppg, C, tiles, family, report=None):
    """every bounded figure of one case and family from the fp32 models: {quantity: figure}"""
    d = family_inputs(family, G, ppg, C)
    x, fig = d["x"], {}

    def take(new):
        for k, v in new.items():
            fig[k] = max(fig.get(k, 0.0), v)

    if kind in ("fwd", "tile"):
        affine = kind == "tile" or G > 1 or C % 16 == 8
        ga, be = (d["gamma"], d["beta"]) if affine else (None, None)
        part = tile_partials(x, tiles) if kind == "tile" else None
        for relu, res in ((False, None), (True, d["res"])):
            take(forward_figures(forward_model(x, ga, be, res=res, relu=relu, partials=part),
                                 forward64(x, ga, be, res=res, relu=relu, partials=part)))
    else:
        mean, rstd = fp32_stats_of(x)
        f64 = forward64(x, d["gamma"] if kind == "bn_bwd" else None, d["beta"] if kind == "bn_bwd" else None)
        ga = d["gamma"] if kind == "bn_bwd" else None
        fm = forward_model(x, ga, d["beta"] if kind == "bn_bwd" else None)
        for relu in (False, True):
            yout = apply_model(x, f64["scale"].float(), f64["shift"].float(), None, True) if (relu and kind == "bn_bwd") else None
            take(backward_figures(backward_model(x, d["dy"], mean, rstd, relu, ga, yout), backward64(x, d["dy"], mean, rstd, ga, relu, yout)))
            if chain_case_ok(family, relu, yout is not None):          # the chain: the model's own fp32 statistics against float64's
                yc = fm["y"].clamp_min(0) if yout is not None else None
                got = backward_model(x, d["dy"], fm["mean"], fm["rstd"], relu, ga, yc)
                ref = backward64(x, d["dy"], f64["mean"], f64["rstd"], ga, relu, yc)
                chain = backward_figures(got, ref, chain_condition(f64))
                take({k: chain[k] for k in ("s2_chain", "dx_chain")})
    if report:
        report(kind, G, ppg, C, tiles, family, fig)
    return fig


def measure(report=None, cases=None, families=FAMILIES):
    """the largest figure of every quantity over the bounded cases and the families"""
    worst = {}
    for (kind, name, G, ppg, C, tiles) in (bounded_cases() if cases is None else cases):
        for family in families:
            for k, v in model_figures(kind, G, ppg, C, tiles, family, report).items():
                if v > worst.get(k, (0.0,))[0]:
                    worst[k] = (v, family, kind, G, ppg, C)
    return worst
