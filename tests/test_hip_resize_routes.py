"""The bilinear resize / L2-normalise kernels on every route (resize_ops.hip, the fused bilinear_l2 kernels of norm_ops.hip, the
pooled backward), against float64 and, where the answer can be known, to the bit.  tests/resize_cases.py holds the cases, the
references, the bounds and their derivation; tests/test_resize_cases.py proves on the CPU that a correct implementation passes and
what the criteria catch.  The C entries are called directly with data_ptr()s, so a test hands them its own y / g / inv_norm / count;
every operand also runs as a channel slice of a wider NaN-filled buffer (16-byte aligned: the vector kernels; 4- or 8-byte offset
with an odd stride: the scalar ones), outputs and workspaces start as NaN and the surroundings of every slice are checked.

Each bounded figure is printed (`FIGURE quantity value bound case`) before it is asserted."""
import math

import pytest
import torch

from tests import resize_cases as rc

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = math.nan
EINVAL, ENOMEM = -22, -12
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    from openess_amd import _lib
    return _lib.load()


def _check(code, what):
    from openess_amd import _lib
    _lib.check(code, what)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(*shape):
    return torch.full(shape, NAN, dtype=F32, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32).cpu()


def _same(got, want):
    return got.dtype == want.dtype and torch.equal(_bits(got), _bits(want))


def _figure(name, value, what, extra=0.0):
    bound = rc.BOUND[name] + extra
    print(f"FIGURE {name} {value:.3e} bound {bound:.3e} {what}")
    assert value <= bound, (name, value, bound, what)


# --------------------------------------------------------------------------------------------- entry helpers
def _resize_fwd(lib, x, Ho, Wo, align, pair):
    """x [B, H, W, C] (CPU) through oess_resize_bilinear_nhwc_fwd with the layouts (input, output): the output view, on the CPU"""
    B, H, W, C = x.shape
    xbuf, xv = rc.place(x, pair[0], DEV)
    obuf, ov = rc.place_out((B, Ho, Wo, C), x.dtype, pair[1], DEV)
    _check(lib.oess_resize_bilinear_nhwc_fwd(_p(xv), rc.layout_stride(pair[0], C), B, H, W, C, int(x.dtype == BF16), Ho, Wo, int(align),
                                             _p(ov), rc.layout_stride(pair[1], C), _st()), "resize_fwd")
    out = ov.cpu()
    assert rc.surroundings_untouched(obuf, pair[1], C) and rc.surroundings_untouched(xbuf, pair[0], C) and _same(xv, x), pair
    return out


def _resize_bwd(lib, g, H, W, align, pair):
    B, Ho, Wo, C = g.shape
    gbuf, gv = rc.place(g, pair[0], DEV)
    obuf, ov = rc.place_out((B, H, W, C), g.dtype, pair[1], DEV)
    n = lib.oess_resize_bilinear_bwd_workspace_bytes(B, W, C, Ho)
    assert n == B * Ho * W * C * 4
    ws = _nan(n // 4)
    _check(lib.oess_resize_bilinear_nhwc_bwd(_p(gv), rc.layout_stride(pair[0], C), B, H, W, C, int(g.dtype == BF16), Ho, Wo, int(align),
                                             _p(ws), n, _p(ov), rc.layout_stride(pair[1], C), _st()), "resize_bwd")
    out = ov.cpu()
    assert rc.surroundings_untouched(obuf, pair[1], C) and rc.surroundings_untouched(gbuf, pair[0], C) and _same(gv, g), pair
    return out


def _l2_fwd(lib, x, eps, pair):
    P, C = x.shape
    xbuf, xv = rc.place(x, pair[0], DEV)
    obuf, ov = rc.place_out((P, C), x.dtype, pair[1], DEV)
    inv = _nan(P)
    _check(lib.oess_l2norm_nhwc_fwd(_p(xv), rc.layout_stride(pair[0], C), P, C, int(x.dtype == BF16), eps, _p(ov),
                                    rc.layout_stride(pair[1], C), _p(inv), _st()), "l2norm_fwd")
    assert rc.surroundings_untouched(obuf, pair[1], C) and rc.surroundings_untouched(xbuf, pair[0], C), pair
    return ov.cpu(), inv.cpu()


def _l2_bwd(lib, y, g, inv, eps, triple):
    P, C = y.shape
    ybuf, yv = rc.place(y, triple[0], DEV)
    gbuf, gv = rc.place(g, triple[1], DEV)
    obuf, ov = rc.place_out((P, C), y.dtype, triple[2], DEV)
    ivd = inv.to(DEV)
    _check(lib.oess_l2norm_nhwc_bwd(_p(yv), rc.layout_stride(triple[0], C), _p(gv), rc.layout_stride(triple[1], C), _p(ivd), P, C,
                                    int(y.dtype == BF16), eps, _p(ov), rc.layout_stride(triple[2], C), _st()), "l2norm_bwd")
    assert rc.surroundings_untouched(obuf, triple[2], C), triple
    return ov.cpu()


def _fused(lib, x, scale, normalize, pair, with_inv=None, device_out=False):
    """oess_bilinear_l2norm_nhwc_bf16 on x [B, H, W, C] (CPU or device): (out, inv or None)"""
    B, H, W, C = x.shape
    xbuf, xv = rc.place(x, pair[0], DEV)
    obuf, ov = rc.place_out((B, H * scale, W * scale, C), BF16, pair[1], DEV)
    inv = _nan(B * H * scale * W * scale) if (normalize if with_inv is None else with_inv) else None
    _check(lib.oess_bilinear_l2norm_nhwc_bf16(_p(xv), rc.layout_stride(pair[0], C), B, H, W, C, scale, int(normalize), _p(ov),
                                              rc.layout_stride(pair[1], C), _p(inv), _st()), "bilinear_l2norm")
    assert rc.surroundings_untouched(obuf, pair[1], C), pair
    if device_out:
        return ov, inv
    return ov.cpu(), None if inv is None else inv.cpu()


# --------------------------------------------------------------------------------------------- exact resize
def _resize_id(c):
    return f"{c[0]}-{c[1]}-C{c[4]}"


@pytest.mark.parametrize("case", rc.resize_cases(), ids=_resize_id)
def test_exact_resize(lib, case):
    """forward and backward on every layout pair: the float64 reference cast once to the output type, bit for bit"""
    _, dt, H, W, C, Ho, Wo, align, _ = case
    c = rc.exact_resize(dt, H, W, C, Ho, Wo, align)
    for pair in rc.LAYOUT_PAIRS:
        assert _same(_resize_fwd(lib, c["x"], Ho, Wo, align, pair), c["y"]), ("forward", rc.resize_route(dt == "bf16", H, W, C, Ho, Wo, pair))
        assert _same(_resize_bwd(lib, c["g"], H, W, align, pair), c["gin"]), ("backward", pair)


def test_resize_entries_refuse_bad_arguments(lib):
    x = torch.zeros(1, 2, 2, 8, dtype=BF16, device=DEV)
    o = torch.zeros(1, 4, 4, 8, dtype=BF16, device=DEV)
    ws = _nan(1 * 4 * 2 * 8)
    assert lib.oess_resize_bilinear_nhwc_fwd(_p(x), 7, 1, 2, 2, 8, 1, 4, 4, 0, _p(o), 8, _st()) == EINVAL
    assert lib.oess_resize_bilinear_nhwc_bwd(_p(o), 8, 1, 2, 2, 8, 1, 4, 4, 0, _p(ws), ws.numel() * 4 - 1, _p(x), 8, _st()) == ENOMEM
    assert lib.oess_resize_bilinear_nhwc_bwd(_p(o), 8, 1, 2, 2, 8, 1, 4, 4, 0, _p(ws) + 4, ws.numel() * 4, _p(x), 8, _st()) == ENOMEM
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws).all())


# --------------------------------------------------------------------------------------------- exact L2
@pytest.mark.parametrize("dt,P,C", rc.l2_cases(), ids=lambda v: str(v))
def test_exact_l2(lib, dt, P, C):
    """forward: y and inv_norm equal the fp32 model (an exact sum, then sqrtf, the divide and the product, each correctly rounded)
    bit for bit on every route; backward on the test's own y, g and inv_norm: the float64 reference cast once, bit for bit"""
    c = rc.exact_l2(dt, P, C)
    y, inv = rc.l2_fwd_model(c["x"], rc.EPS_TEST)
    for pair in rc.LAYOUT_PAIRS:
        gy, ginv = _l2_fwd(lib, c["x"], rc.EPS_TEST, pair)
        assert _same(gy, y) and _same(ginv, inv), ("forward", rc.l2norm_route(dt == "bf16", P, C, pair))
    for triple in rc.LAYOUT_TRIPLES:
        assert _same(_l2_bwd(lib, c["y"], c["g"], c["inv"], rc.EPS_TEST, triple), c["gx"]), ("backward", triple)


def test_exact_l2_across_the_grid_cap(lib):
    """P = 4 x 262144 + 5 pixels of 3 fp32 channels: the generic kernels' grid-stride loops run a second trip (12 MB)"""
    dt, P, C = rc.L2_CAP_CASE
    assert rc.l2norm_route(False, P, C)["capped"]
    g = rc._gen("l2cap")
    x = torch.randint(-3, 4, (P, C), generator=g).float()
    x[P - 3] = 0.0
    xd = x.to(DEV)
    y, inv = _nan(P, C), _nan(P)
    _check(lib.oess_l2norm_nhwc_fwd(_p(xd), C, P, C, 0, rc.EPS_TEST, _p(y), C, _p(inv), _st()), "l2norm_fwd")
    my, minv = rc.l2_fwd_model(x, rc.EPS_TEST)
    assert _same(y, my) and _same(inv, minv)
    yq = (torch.randint(-4, 5, (P, C), generator=g).float() / 4.0)
    gq = torch.randint(-3, 4, (P, C), generator=g).float()
    iq = rc._pick((0.5, 1.0, 2.0, 1024.0), (P,), g).float()
    gx = _nan(P, C)
    yd, gd, idv = yq.to(DEV), gq.to(DEV), iq.to(DEV)
    _check(lib.oess_l2norm_nhwc_bwd(_p(yd), C, _p(gd), C, _p(idv), P, C, 0, rc.EPS_TEST, _p(gx), C, _st()), "l2norm_bwd")
    assert _same(gx, rc.cast(rc.l2_bwd64(yq, gq, iq, rc.EPS_TEST), F32))


# --------------------------------------------------------------------------------------------- exact fused upsample
@pytest.mark.parametrize("H,W,scale", rc.FUSED_EXACT_GEOMS)
def test_exact_fused_upsample(lib, H, W, scale):
    """normalize = 0 on the vector kernels (LPP 8 .. 64), the scalar kernel (3 / 5 / 7 channels per lane) and the scalar kernel on a
    vector count through slice_odd"""
    for C in rc.FUSED_VEC_CHANNELS + rc.FUSED_SCALAR_CHANNELS:
        c = rc.exact_fused(H, W, scale, C)
        for pair in rc.LAYOUT_PAIRS if C == 64 else rc.LAYOUT_PAIRS[:2]:
            got, _ = _fused(lib, c["x"], scale, 0, pair)
            assert _same(got, c["y"]), (C, pair, rc.fused_route(rc.FUSED_B, H, W, C, scale, pair))


def test_fused_refuses_inv_norm_without_normalize(lib):
    x = torch.zeros(1, 2, 2, 64, dtype=BF16, device=DEV)
    o = _nan(1, 4, 4, 64).bfloat16()
    inv = _nan(16)
    assert lib.oess_bilinear_l2norm_nhwc_bf16(_p(x), 64, 1, 2, 2, 64, 2, 0, _p(o), 64, _p(inv), _st()) == EINVAL
    assert lib.oess_bilinear_l2norm_nhwc_bf16(_p(x), 64, 1, 2, 2, 96, 2, 1, _p(o), 96, None, _st()) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and bool(torch.isnan(inv).all())


def test_exact_fused_scalar_across_the_block_cap(lib):
    """C = 192 at (65, 65) x 4: 67600 output pixels, more than 4 x 16384, so the scalar kernel's grid-stride loop runs a second trip"""
    B, H, W, C, scale = rc.FUSED_CAP_CASE
    assert rc.fused_route(B, H, W, C, scale)["capped"]
    # (65 - 1) / (260 - 1) is not dyadic, so the case runs bounded (it is one of the shapes the model figures are taken over); the
    # second trip's pixels, the last 2064, are covered by the same figures
    x = rc.fused_family_input("randn", H, W, C, B)
    got, inv = _fused(lib, x, scale, 1, ("dense", "slice_vec"))
    for k, v in rc.fused_figures(got, inv, x, scale).items():
        _figure(k, v, "randn (65,65) x4 C=192 scalar, capped grid")
    tail = got.view(-1, C)[4 * rc.FUSED_SCALAR_CAP:]
    assert tail.shape[0] == 67600 - 65536 and not bool(torch.isnan(tail.float()).any())


# --------------------------------------------------------------------------------------------- the non-temporal store branch
NT_CASE_BYTES = 5 * 256 * 256 * 512 * 2 + 256 * 256 * 512 * 2 + (64 << 20)      # the 335 MB output, one 67 MB single, the rest


def test_fused_nt_store_equals_the_single_sample_calls(lib):
    """B = 5, C = 512, (64, 64) x 4: a 335 MB output takes the non-temporal stores production takes; each sample must equal its own
    67 MB call (plain stores) bit for bit, inv_norm included.  All on the GPU: the values themselves are held by the bounded cases."""
    free = torch.cuda.mem_get_info()[0]
    if free < NT_CASE_BYTES:
        pytest.skip(f"needs {NT_CASE_BYTES >> 20} MB of device memory, {free >> 20} MB free")
    B, H, W, C, scale = rc.FUSED_NT_CASE
    assert rc.fused_route(B, H, W, C, scale)["nt_out"] and not rc.fused_route(1, H, W, C, scale)["nt_out"]
    x = torch.randn(B, H, W, C, generator=rc._gen("nt")).bfloat16().to(DEV)
    n = H * scale * W * scale
    big = torch.full((B, n, C), NAN, dtype=BF16, device=DEV)
    binv = _nan(B * n)
    _check(lib.oess_bilinear_l2norm_nhwc_bf16(_p(x), C, B, H, W, C, scale, 1, _p(big), C, _p(binv), _st()), "bilinear_l2norm")
    one, oinv = torch.empty((n, C), dtype=BF16, device=DEV), _nan(n)
    for b in range(B):
        one.fill_(NAN)
        oinv.fill_(NAN)
        _check(lib.oess_bilinear_l2norm_nhwc_bf16(_p(x[b]), C, 1, H, W, C, scale, 1, _p(one), C, _p(oinv), _st()), "bilinear_l2norm")
        assert torch.equal(big[b].view(torch.int16), one.view(torch.int16)), b
        assert torch.equal(binv[b * n:(b + 1) * n].view(torch.int32), oinv.view(torch.int32)), b
    assert not bool(torch.isnan(binv).any())


# --------------------------------------------------------------------------------------------- exact pooled backward
def _pool_bwd(lib, c, H, W, Ho, Wo, C, pair, B=rc.POOL_B, ws_short=0, ws_shift=0, align=1):
    fbuf, fv = rc.place(c["feat"], pair[0], DEV)
    obuf, ov = rc.place_out((B, H, W, C), BF16, pair[1], DEV)
    n = lib.oess_bilinear_l2norm_pool_bwd_workspace_bytes(B, W, C, Ho, c["S"])
    assert n >= (B * Ho * W * C + c["S"] * C) * 4 and n % 4 == 0
    ws = _nan(n // 4 + 4)
    inv, ids, gk, count = (c[k].to(DEV) for k in ("inv", "ids", "gk", "count"))
    code = lib.oess_bilinear_l2norm_pool_bwd_bf16(_p(fv), rc.layout_stride(pair[0], C), _p(inv), _p(ids), _p(gk), _p(count), c["sps"], c["S"],
                                                  B, H, W, C, Ho, Wo, align, rc.EPS_TEST, _p(ws) + ws_shift, n - ws_short, _p(ov),
                                                  rc.layout_stride(pair[1], C), _st())
    torch.cuda.synchronize()
    assert rc.surroundings_untouched(obuf, pair[1], C) and rc.surroundings_untouched(fbuf, pair[0], C)
    return code, ov.cpu(), ws


@pytest.mark.parametrize("C", rc.POOL_CHANNELS)
@pytest.mark.parametrize("geom", rc.POOL_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_exact_pooled_backward(lib, geom, C):
    """count 64 in every row, integer gk, a saved map of multiples of 1/4, power-of-two inv_norm with two pixels clamped, ids below 0
    and at or above S, ids that change at every pixel: the float64 composed reference rounded once to bf16, bit for bit"""
    H, W, Ho, Wo = geom
    c = rc.exact_pool(H, W, Ho, Wo, C)
    for pair in rc.LAYOUT_PAIRS[:2]:
        code, got, _ = _pool_bwd(lib, c, H, W, Ho, Wo, C, pair)
        _check(code, "pool_bwd")
        assert _same(got, c["gin"]), (pair, rc.pool_route(W, C))


@pytest.mark.parametrize("C", rc.POOL_CHANNELS)
def test_bounded_pooled_backward_at_the_wide_geometry(lib, C):
    """(2, 33) -> (8, 129): the vertical ratio 1/7 is not dyadic, so this geometry runs against the float64 composed reference
    under four times the model's figure, like every bounded case; its dyadic neighbour (9, 129) is among the exact cases"""
    H, W, Ho, Wo = rc.POOL_ISSUE_WIDE
    c = rc.wide_pool(C)
    for pair in rc.LAYOUT_PAIRS[:2]:
        code, got, _ = _pool_bwd(lib, c, H, W, Ho, Wo, C, pair)
        _check(code, "pool_bwd")
        fig = rc.pool_figure(got, c["feat"], c["inv"], c["ids"], c["gk"], c["count"], c["sps"], H, W, rc.EPS_TEST)
        _figure("pool_bwd", fig, f"(2,33)->(8,129) C={C} {pair}")


def test_pooled_backward_refuses_bad_arguments(lib):
    H, W, Ho, Wo = rc.POOL_GEOMS[0]
    c = rc.exact_pool(H, W, Ho, Wo, 64)
    for kw, want in ((dict(ws_short=1), ENOMEM), (dict(ws_shift=4), ENOMEM)):
        code, got, ws = _pool_bwd(lib, c, H, W, Ho, Wo, 64, ("dense", "slice_vec"), **kw)
        assert code == want and bool(torch.isnan(got.float()).all()) and bool(torch.isnan(ws).all()), kw
    for pair in rc.LAYOUT_PAIRS[2:]:                      # the node has vector kernels only
        code, got, _ = _pool_bwd(lib, c, H, W, Ho, Wo, 64, pair)
        assert code == EINVAL and bool(torch.isnan(got.float()).all())
    c192 = dict(c, feat=torch.zeros(rc.POOL_B, Ho, Wo, 192, dtype=BF16), gk=torch.zeros(c["S"], 192))
    code, got, _ = _pool_bwd(lib, c192, H, W, Ho, Wo, 192, ("dense", "slice_vec"))
    assert code == EINVAL and bool(torch.isnan(got.float()).all())


# --------------------------------------------------------------------------------------------- bounded cases
@pytest.mark.parametrize("family", rc.FAMILIES)
@pytest.mark.parametrize("geom", rc.BOUNDED_GEOMS, ids=lambda g: f"{g[0]}-{g[1]}x{g[2]}-{g[4]}x{g[5]}-C{g[3]}")
def test_bounded_resize(lib, geom, family):
    dt, H, W, C, Ho, Wo, align = geom
    x, g = rc.resize_family_inputs(family, dt, H, W, C, Ho, Wo)
    err = rc.err_bf16 if dt == "bf16" else rc.err_fp32
    y64, ys = rc.resize_fwd64(x, Ho, Wo, align), rc.resize_fwd64(x.double().abs(), Ho, Wo, align)      # the measures of
    g64, gs = rc.resize_bwd64(g, H, W, align), rc.resize_bwd64(g.double().abs(), H, W, align)          # resize_*_figure, once
    for pair in (rc.LAYOUT_PAIRS[0], rc.LAYOUT_PAIRS[2], rc.LAYOUT_PAIRS[3]):
        r = rc.resize_route(dt == "bf16", H, W, C, Ho, Wo, pair)["kernel"]
        what = f"{family} {dt} ({H},{W})->({Ho},{Wo}) C={C} {r}"
        _figure(f"resize_fwd_{dt}", err(_resize_fwd(lib, x, Ho, Wo, align, pair), y64, ys), what)
        _figure(f"resize_bwd_{dt}", err(_resize_bwd(lib, g, H, W, align, pair), g64, gs), what)


@pytest.mark.parametrize("family", rc.FAMILIES)
@pytest.mark.parametrize("dt,P,C", rc.bounded_l2_shapes(), ids=lambda v: str(v))
def test_bounded_l2(lib, dt, P, C, family):
    """eps = 1e-12, as the wrappers pass it; the backward takes the model's y and inv_norm as operands"""
    x, g = rc.l2_family_inputs(family, dt, P, C)
    my, minv = rc.l2_fwd_model(x, 1e-12)
    for pair, triple in ((rc.LAYOUT_PAIRS[0], rc.LAYOUT_TRIPLES[0]), (rc.LAYOUT_PAIRS[2], rc.LAYOUT_TRIPLES[3])):
        what = f"{family} {dt} P={P} C={C} {rc.l2norm_route(dt == 'bf16', P, C, pair)['kernel']}"
        y, inv = _l2_fwd(lib, x, 1e-12, pair)
        for k, v in rc.l2_fwd_figures(y, inv, x, 1e-12).items():
            _figure(k, v, what)
        _figure("l2_bwd", rc.l2_bwd_figure(_l2_bwd(lib, my, g, minv, 1e-12, triple), my, g, minv, 1e-12), what)


@pytest.mark.parametrize("family", rc.FAMILIES)
@pytest.mark.parametrize("H,W,scale", rc.FUSED_BOUNDED_GEOMS)
def test_bounded_fused(lib, H, W, scale, family):
    """normalize = 1 with inv_norm.  The vector kernel takes rsqrtf, which is not correctly rounded: its model uses 1 / sqrt and its
    bound gets one fp32 ulp of the result added (the measures' scales are at least the result's magnitude)."""
    for C in rc.FUSED_VEC_CHANNELS + rc.FUSED_SCALAR_CHANNELS:
        x = rc.fused_family_input(family, H, W, C)
        for pair in rc.LAYOUT_PAIRS if C == 64 else rc.LAYOUT_PAIRS[:1]:
            kernel = rc.fused_route(rc.FUSED_B, H, W, C, scale, pair)["kernel"]
            y, inv = _fused(lib, x, scale, 1, pair)
            for k, v in rc.fused_figures(y, inv, x, scale).items():
                _figure(k, v, f"{family} ({H},{W}) x{scale} C={C} {kernel}", extra=rc.RSQRT_ULP if kernel == "vec" else 0.0)
            y2, none = _fused(lib, x, scale, 1, pair, with_inv=False)      # the inference form: no inv_norm, the same bits
            assert none is None and _same(y2, y)


# --------------------------------------------------------------------------------------------- the wrappers, on slices
def _nchw_slice(t, layout, grad=False):
    """t [B, H, W, C] as a logical NCHW tensor over a channel slice of a wider buffer"""
    _, view = rc.place(t, layout, DEV)
    v = view.permute(0, 3, 1, 2)
    assert not v.is_contiguous() and not v.is_contiguous(memory_format=torch.channels_last)
    return v.requires_grad_(True) if grad else v


def test_wrapper_bilinear_resize_exact_on_a_slice():
    from openess_amd import hip
    H, W, C, Ho, Wo, align = 5, 3, 24, 17, 9, True
    for dt, C in (("bf16", 24), ("f32", 12)):
        c = rc.exact_resize(dt, H, W, C, Ho, Wo, align)
        x = _nchw_slice(c["x"], "slice_vec", grad=True)
        y = hip.bilinear_resize(x, size=(Ho, Wo), align_corners=align)
        assert _same(y.detach().permute(0, 2, 3, 1), c["y"])
        y.backward(_nchw_slice(c["g"], "slice_odd"))
        assert _same(x.grad.permute(0, 2, 3, 1), c["gin"])


def test_wrapper_l2_normalize_exact_on_a_slice():
    from openess_amd import hip
    for dt, C in (("bf16", 128), ("f32", 40)):
        c = rc.exact_l2(dt, 37, C)
        my, _ = rc.l2_fwd_model(c["x"], rc.EPS_TEST)
        x = _nchw_slice(c["x"].view(1, 1, 37, C), "slice_vec", grad=True)
        y = hip.l2_normalize(x, eps=rc.EPS_TEST)
        assert _same(y.detach().permute(0, 2, 3, 1).reshape(37, C), my)
        # the node's backward reads its own y and inv_norm: the float64 adjoint on those operands, rounded once.  The data leaves it
        # bounded, not exact (y is no multiple of 1/4)
        g = _nchw_slice(c["g"].view(1, 1, 37, C), "slice_odd")
        y.backward(g)
        _, minv = rc.l2_fwd_model(c["x"], rc.EPS_TEST)
        got = x.grad.permute(0, 2, 3, 1).reshape(37, C).cpu()
        _figure("l2_bwd", rc.l2_bwd_figure(got, my, c["g"], minv, rc.EPS_TEST), f"wrapper {dt} C={C}")


def test_wrapper_bilinear_l2norm_on_a_slice(lib):
    from openess_amd import hip
    H, W, scale, C = 3, 3, 3, 128
    c = rc.exact_fused(H, W, scale, C)
    x = _nchw_slice(c["x"], "slice_vec")
    assert _same(hip.bilinear_l2norm(x, scale, False).permute(0, 2, 3, 1), c["y"])
    # normalised, inference and training form: the same bits, within the fused bound; the backward is the L2 adjoint on the node's
    # own (y, inv_norm) rounded to bf16, then the bilinear adjoint
    xg = x.detach().requires_grad_(True)
    y = hip.bilinear_l2norm_train(xg, scale)
    assert torch.equal(y.detach(), hip.bilinear_l2norm(x, scale, True))
    yn = y.detach().permute(0, 2, 3, 1).cpu()
    _, inv = _fused(lib, c["x"], scale, 1, ("slice_vec", "dense"))
    for k, v in rc.fused_figures(yn, inv, c["x"], scale).items():
        _figure(k, v, f"wrapper ({H},{W}) x{scale} C={C}", extra=rc.RSQRT_ULP)
    g = rc.ints((rc.FUSED_B, H * scale, W * scale, C), "wrapper g").bfloat16()
    y.backward(_nchw_slice(g, "slice_vec"))
    inv = inv.view(rc.FUSED_B, H * scale, W * scale)
    gup = rc.l2_bwd64(yn, g, inv, 1e-12)
    l2_scale = inv.double()[..., None] * (g.double().abs() + yn.double().abs() * (yn.double() * g.double()).abs().sum(-1, keepdim=True))
    ref = rc.resize_bwd64(gup, H, W, True)
    # the intermediate is stored in bf16 (half an ulp of each element, through the adjoint), each half within its own bound
    tol = rc.resize_bwd64(0.5 * rc.ulp_bf16(gup) + (rc.BOUND["l2_bwd"] + 2.0 ** -23) * l2_scale, H, W, True) + \
        rc.BOUND["resize_bwd_bf16"] * rc.resize_bwd64(gup.abs() * (1 + 2.0 ** -8), H, W, True) + 0.5 * rc.ulp_bf16(ref) * (1 + 2.0 ** -6)
    d = (xg.grad.permute(0, 2, 3, 1).double().cpu() - ref).abs()
    print(f"FIGURE wrapper_train_bwd {float((d / tol).max()):.3e} bound 1.000e+00 of the composed tolerance")
    assert bool((d <= tol).all())


def test_wrapper_upsampled_normalized_pool_on_a_slice(lib):
    """hip.UpsampledNormalizedFeature(x, scale).pool: the forward within bf16 storage of the normalised map, the backward against
    the composed float64 reference on the node's own saved operands (the fused entry's output on the same input; the counts)"""
    from openess_amd import hip
    H, W, scale, C, B, sps, S = 7, 7, 7, 64, rc.POOL_B, rc.POOL_SPS, rc.POOL_S
    Ho, Wo = H * scale, W * scale
    c = rc.exact_fused(H, W, scale, C)
    ids = rc.pool_ids(B, Ho, Wo, sps)
    x = _nchw_slice(c["x"], "slice_vec", grad=True)
    k = hip.UpsampledNormalizedFeature(x, scale).pool(ids.view(B, Ho, Wo).to(DEV), sps, S)
    y, inv = _fused(lib, c["x"], scale, 1, ("slice_vec", "dense"))
    gid = ids + torch.arange(B).repeat_interleave(Ho * Wo) * sps
    ok = (gid >= 0) & (gid < S)
    count = torch.zeros(S, dtype=F64).index_add(0, gid[ok], torch.ones(int(ok.sum()), dtype=F64))
    sums = torch.zeros(S, C, dtype=F64).index_add(0, gid[ok], y.view(-1, C).double()[ok])
    k64 = sums / (count.float() + torch.tensor(1e-6)).double()[:, None]
    # fp32 sums of at most 2 Ho Wo terms of magnitude <= 1 over the count: 2^-24 per addition is far below this
    assert float((k.detach().double().cpu() - k64).abs().max()) <= 1e-5
    gk = rc.ints((S, C), "wrapper gk").float()
    k.backward(gk.to(DEV))
    fig = rc.pool_figure(x.grad.permute(0, 2, 3, 1).cpu(), y, inv, ids, gk, count.float(), sps, H, W, 1e-12)
    print(f"FIGURE wrapper_pool_bwd {fig:.3e} bound {rc.pool_bound():.3e} (7,7) x7 C=64")
    assert fig <= rc.pool_bound()
