"""The bf16 normalisation kernels of norm_ops.hip on every route, against float64 and, where the answer can be known, to the bit
(tests/norm_cases.py holds the cases, the references, the bounds and their derivation; tests/test_norm_cases.py proves on the CPU
that a correct implementation passes and what the criteria catch).  The C entries are called directly with data_ptr()s, so a test
hands them its own mean / rstd / scale / shift / y_out / tile partials; every operand also runs as a channel slice of a wider
NaN-filled buffer, and every workspace starts as NaN.  hip.instance_norm and hip.batch_norm_train run on strided slices too.

Each bounded figure is printed (`FIGURE quantity value case`) before it is asserted."""
import math

import numpy as np
import pytest
import torch

from tests import norm_cases as nc

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = math.nan


def _id(case):
    return f"{case[0]}-{case[1]}x{case[2]}x{case[3]}"


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
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def _workspace(lib, G, ppg, C, backward):
    """the partials buffer, all NaN: a chunk row the statistics kernel does not write poisons the sums"""
    n = lib.oess_norm_partials_bytes(G, ppg, C, int(backward))
    assert n % 4 == 0 and n > 0
    return _nan(n // 4), n


def _figure(name, value, what, bound=None):
    bound = nc.BOUND[name] if bound is None else bound
    print(f"FIGURE {name} {value:.3e} bound {bound:.3e} {what}")
    assert value <= bound, (name, value, bound, what)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _other(layout):
    """a second layout with another pixel stride: the residual, dy and the outputs never share x's stride"""
    return {"dense": "slice24", "slice8": "slice24", "slice24": "slice8"}[layout]


# --------------------------------------------------------------------------------------------- entry helpers
def _stats(lib, xv, ps):
    G, P, C = xv.shape
    ws, n = _workspace(lib, G, P, C, False)
    s, q = _nan(G, C), _nan(G, C)
    _check(lib.oess_norm_stats_nhwc_bf16(_p(xv), ps, G, P, C, _p(s), _p(q), _p(ws), n, _st()), "stats")
    return s, q


def _finalize(lib, xv, ps, gamma, beta, running):
    G, P, C = xv.shape
    ws, n = _workspace(lib, G, P, C, False)
    o = _nan(4, G, C)
    rm = rv = None
    if running:
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    _check(lib.oess_norm_stats_finalize_nhwc_bf16(_p(xv), ps, G, P, C, nc.EPS, _p(gamma), _p(beta), _p(rm), _p(rv), nc.MOMENTUM, _p(o[0]),
                                                  _p(o[1]), _p(o[2]), _p(o[3]), _p(ws), n, _st()), "stats_finalize")
    return dict(mean=o[0], rstd=o[1], scale=o[2], shift=o[3], running_mean=rm, running_var=rv)


def _apply(lib, xv, ps, scale, shift, resv, rps, relu, outv, ops):
    G, P, C = xv.shape
    _check(lib.oess_norm_apply_nhwc_bf16(_p(xv), ps, _p(scale), _p(shift), _p(resv), rps, int(relu), G, P, C, _p(outv), ops, _st()), "apply")


def _check_finalize_exact(got, c, f64, gamma, beta, running):
    P = c["ppg"]
    assert torch.equal(got["mean"].cpu(), (c["S"].double() / P).float())                 # the float64 quotient rounded to fp32
    assert nc.ulps_fp32(got["rstd"], f64["rstd"]) <= nc.RSTD_ULPS
    bs, bh = nc.finalize_bounds(f64, gamma, beta)
    assert bool(((got["scale"].double().cpu() - f64["scale"]).abs() <= bs).all())
    assert bool(((got["shift"].double().cpu() - f64["shift"]).abs() <= bh).all())
    if running:
        rm, rv = nc.running64(f64["mean"], f64["var"], P, torch.zeros(c["C"]), torch.ones(c["C"]))
        np.testing.assert_allclose(got["running_mean"].cpu().numpy(), rm.numpy(), rtol=nc.RUNNING_MEAN_RTOL, atol=1e-9)
        np.testing.assert_allclose(got["running_var"].cpu().numpy(), rv.numpy(), rtol=nc.RUNNING_VAR_RTOL)


def _check_running(rm, rv, f64, P, C):
    """the running statistics of a fresh BatchNorm2d after one bounded (not exact) forward"""
    erm, erv = nc.running64(f64["mean"], f64["var"], P, torch.zeros(C), torch.ones(C))
    am, av = nc.running_tolerances(f64, P)
    np.testing.assert_allclose(rm.cpu().numpy(), erm.numpy(), rtol=nc.RUNNING_MEAN_RTOL, atol=am + 1e-9)
    np.testing.assert_allclose(rv.cpu().numpy(), erv.numpy(), rtol=nc.RUNNING_VAR_RTOL, atol=av)


# --------------------------------------------------------------------------------------------- exact forward
@pytest.mark.parametrize("case", nc.FWD_CASES, ids=_id)
def test_exact_forward(lib, case):
    _, G, P, C, layouts, _ = case
    c = nc.exact_forward(G, P, C)
    gamma, beta = c["gamma"].to(DEV), c["beta"].to(DEV)
    f64 = nc.forward64(c["x"], c["gamma"], c["beta"])
    scale, shift = c["scale"].to(DEV), c["shift"].to(DEV)
    for layout in layouts:
        xbuf, xv = nc.place(c["x"], layout, DEV)
        ps = nc.layout_stride(layout, C)
        s, q = _stats(lib, xv, ps)
        assert torch.equal(s.double().cpu(), c["S"].double()) and torch.equal(q.double().cpu(), c["Q"].double()), layout
        got = _finalize(lib, xv, ps, gamma, beta, running=G == 1)
        _check_finalize_exact(got, c, f64, c["gamma"], c["beta"], G == 1)
        rl = _other(layout)
        _, rv = nc.place(c["res"], rl, DEV)
        for ol in (layout, rl):
            for (relu, res), y in c["y"].items():
                obuf, ov = nc.place_out((G, P, C), torch.bfloat16, ol, DEV)
                _apply(lib, xv, ps, scale, shift, rv if res else None, nc.layout_stride(rl, C), relu, ov, nc.layout_stride(ol, C))
                assert torch.equal(_bits(ov), _bits(y)), (layout, ol, relu, res)
                assert nc.surroundings_untouched(obuf, ol, C)
        assert torch.equal(_bits(xv), _bits(c["x"])) and nc.surroundings_untouched(xbuf, layout, C)


def test_exact_apply_grid_cap(lib):
    """(1, 32769, 2048): rows = 1 and 8193 pixel chunks wanted, so the grid is capped at 8192 and the grid-stride loop runs twice for
    one workgroup.  Exact data made on the device, expectation from plain torch ops in float64 there."""
    _, G, P, C, _, _ = nc.CAP_CASE
    g = torch.Generator(device=DEV).manual_seed(nc.SEED)
    x = torch.randint(-8, 9, (G, P, C), generator=g, device=DEV).bfloat16()
    xd = x.double()
    assert float(xd.abs().sum(1).max()) < nc.LIMIT and float((xd * xd).sum(1).max()) < nc.LIMIT
    s, q = _stats(lib, x, C)
    assert torch.equal(s.double(), xd.sum(1)) and torch.equal(q.double(), (xd * xd).sum(1))
    scale = torch.tensor([0.25, 0.5, 1.0, 2.0, -0.25, -0.5, -1.0, -2.0], device=DEV)[torch.randint(0, 8, (G, C), generator=g, device=DEV)]
    shift = torch.randint(-4, 5, (G, C), generator=g, device=DEV).float()
    expect = (xd * scale.double()[:, None] + shift.double()[:, None]).clamp_min(0.0)
    del xd
    assert torch.equal(expect.bfloat16().double(), expect)
    out = torch.full((G, P, C), NAN, dtype=torch.bfloat16, device=DEV)
    _apply(lib, x, C, scale, shift, None, 0, True, out, C)
    assert torch.equal(out.double(), expect)


# --------------------------------------------------------------------------------------------- backward entries
def _bn_bwd(lib, xv, xps, dyv, dps, yv, yps, mean, rstd, gamma, relu, dxv, gps, drv, drps):
    _, P, C = xv.shape
    ws, n = _workspace(lib, 1, P, C, True)
    db, dg = _nan(C), _nan(C)
    _check(lib.oess_batchnorm_bwd_nhwc_bf16(_p(xv), xps, _p(dyv), dps, _p(yv), yps, _p(mean), _p(rstd), _p(gamma), int(relu), P, C, _p(db),
                                            _p(dg), _p(dxv), gps, _p(drv), drps, _p(ws), n, _st()), "batchnorm_bwd")
    return db[None], dg[None]


def _in_bwd(lib, xv, xps, dyv, dps, mean, rstd, relu, dxv, gps):
    G, P, C = xv.shape
    ws, n = _workspace(lib, G, P, C, True)
    s1, s2 = _nan(G, C), _nan(G, C)
    _check(lib.oess_instnorm_bwd_nhwc_bf16(_p(xv), xps, _p(dyv), dps, _p(mean), _p(rstd), int(relu), G, P, C, _p(s1), _p(s2), _p(dxv), gps,
                                           _p(ws), n, _st()), "instnorm_bwd")
    return s1, s2


def _run_backward(lib, kind, d, mean, rstd, gamma, yout, relu, layout):
    """either backward entry on `layout` (dy, y_out and the outputs on another stride): dict(s1, s2, dx, dres) and the buffers"""
    G, P, C = d["x"].shape
    ol = _other(layout)
    _, xv = nc.place(d["x"], layout, DEV)
    _, dyv = nc.place(d["dy"], ol, DEV)
    dxbuf, dxv = nc.place_out((G, P, C), torch.bfloat16, layout, DEV)
    xps, ops = nc.layout_stride(layout, C), nc.layout_stride(ol, C)
    mean, rstd = mean.to(DEV).contiguous(), rstd.to(DEV).contiguous()
    drbuf = drv = None
    if kind == "bn_bwd":
        yv = None if yout is None else nc.place(yout, ol, DEV)[1]
        if relu:
            drbuf, drv = nc.place_out((G, P, C), torch.bfloat16, ol, DEV)
        s1, s2 = _bn_bwd(lib, xv, xps, dyv, ops, yv, ops, mean, rstd, None if gamma is None else gamma.to(DEV), relu, dxv, xps, drv, ops)
    else:
        s1, s2 = _in_bwd(lib, xv, xps, dyv, ops, mean, rstd, relu, dxv, xps)
    assert nc.surroundings_untouched(dxbuf, layout, C) and (drbuf is None or nc.surroundings_untouched(drbuf, ol, C))
    return dict(s1=s1, s2=s2, dx=dxv, dres=drv)


@pytest.mark.parametrize("case", nc.BN_BWD_CASES + nc.IN_BWD_CASES, ids=_id)
def test_exact_backward(lib, case):
    """mean integer, rstd and gamma powers of two: d(beta) / s1 and d(gamma) / s2 are the integer sums, d(residual) is the masked dy
    bit for bit (the mask is y_out > 0 with +0, -0, negative and positive entries in y_out; without a stored output it is
    xhat > 0 with x equal to the mean at some pixels), dx sits within the float64 bound"""
    name, G, P, C, layouts, _ = case
    kind = nc.case_kind(name)
    c = nc.exact_backward(G, P, C, kind == "bn_bwd")
    gamma = c["gamma"] if kind == "bn_bwd" else None
    for layout in layouts:
        for relu in (False, True):
            got = _run_backward(lib, kind, c, c["mean"], c["rstd"], gamma, c["yout"] if relu else None, relu, layout)
            e = c[relu]
            assert torch.equal(got["s1"].double().cpu(), e["s1"]) and torch.equal(got["s2"].double().cpu(), e["s2"]), (layout, relu)
            if got["dres"] is not None:
                assert torch.equal(_bits(got["dres"]), _bits(e["dres"])), layout
            b64 = nc.backward64(c["x"], c["dy"], c["mean"], c["rstd"], gamma, relu, c["yout"])
            _figure("dx", nc.err_bf16(got["dx"], b64["dx"], b64["dx_scale"]), f"exact {_id(case)} {layout} relu={relu}")


@pytest.mark.parametrize("case", [c for c in nc.BN_BWD_CASES + nc.IN_BWD_CASES if c[2] <= nc.BOUNDED_MAX_PIXELS], ids=_id)
def test_bounded_backward(lib, case):
    """the four families through the backward entries, mean and rstd supplied (float64 statistics rounded to fp32) and taken by the
    reference as operands; with ReLU the BatchNorm mask comes from a stored output both sides read"""
    name, G, P, C, layouts, _ = case
    kind = nc.case_kind(name)
    for family in nc.FAMILIES:
        d = nc.family_inputs(family, G, P, C)
        mean, rstd = nc.fp32_stats_of(d["x"])
        gamma = d["gamma"] if kind == "bn_bwd" else None
        f64 = nc.forward64(d["x"], gamma, d["beta"] if kind == "bn_bwd" else None)
        for relu in (False, True):
            yout = nc.apply_model(d["x"], f64["scale"].float(), f64["shift"].float(), None, True) if (relu and kind == "bn_bwd") else None
            got = _run_backward(lib, kind, d, mean, rstd, gamma, yout, relu, layouts[1] if relu else layouts[0])
            b64 = nc.backward64(d["x"], d["dy"], mean, rstd, gamma, relu, yout)
            for k, v in nc.backward_figures(got, b64).items():
                _figure(k, v, f"{_id(case)} {family} relu={relu}")
            if got["dres"] is not None:
                assert torch.equal(_bits(got["dres"]), _bits(b64["dres"].bfloat16()))


# --------------------------------------------------------------------------------------------- bounded forward
@pytest.mark.parametrize("case", [c for c in nc.FWD_CASES if c[2] <= nc.BOUNDED_MAX_PIXELS], ids=_id)
def test_bounded_forward(lib, case):
    """statistics + finalize + apply through the entries, the apply taking the kernel's own scale and shift"""
    _, G, P, C, layouts, _ = case
    affine = G > 1 or C % 16 == 8
    for family in nc.FAMILIES:
        d = nc.family_inputs(family, G, P, C)
        ga, be = (d["gamma"], d["beta"]) if affine else (None, None)
        for layout, relu, res in ((layouts[0], False, None), (layouts[1], True, d["res"])):
            _, xv = nc.place(d["x"], layout, DEV)
            ol = _other(layout)
            rv = None if res is None else nc.place(res, ol, DEV)[1]
            ps = nc.layout_stride(layout, C)
            got = _finalize(lib, xv, ps, None if ga is None else ga.to(DEV), None if be is None else be.to(DEV), running=G == 1)
            obuf, ov = nc.place_out((G, P, C), torch.bfloat16, ol, DEV)
            _apply(lib, xv, ps, got["scale"], got["shift"], rv, nc.layout_stride(ol, C), relu, ov, nc.layout_stride(ol, C))
            assert nc.surroundings_untouched(obuf, ol, C)
            f64 = nc.forward64(d["x"], ga, be, res=res, relu=relu)
            got["y"] = ov
            for k, v in nc.forward_figures(got, f64).items():
                _figure(k, v, f"{_id(case)} {family} {layout}")
            if G == 1:
                _check_running(got["running_mean"], got["running_var"], f64, P, C)


# --------------------------------------------------------------------------------------------- the tile-stats route
def _tile(lib, part, tiles, C, P, gamma, beta, xv, xps, rv, rps, relu, ov, ops):
    o = _nan(2, C)
    rm, rvar = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    _check(lib.oess_norm_tile_stats_apply_nhwc_bf16(_p(part), tiles, C, float(P), nc.EPS, _p(gamma), _p(beta), _p(rm), _p(rvar), nc.MOMENTUM,
                                                    _p(o[0]), _p(o[1]), _p(xv), xps, _p(rv), rps, int(relu), P, _p(ov), ops, _st()),
           "tile_stats_apply")
    return dict(mean=o[0][None], rstd=o[1][None], running_mean=rm, running_var=rvar)


@pytest.mark.parametrize("case", nc.TILE_CASES, ids=lambda c: f"tile-{c[5]['tiles']}x{c[3]}")
def test_tile_stats_apply(lib, case):
    """oess_norm_tile_stats_apply_nhwc_bf16 on partials the test supplies: exact data first (mean to the bit, rstd within 2 ulps,
    running statistics, y within the bound; out of place and in place, with and without a residual, dense and as a slice), then
    the four families up to 33 000 pixels"""
    _, _, P, C, layouts, expect = case
    tiles = expect["tiles"]
    c = nc.exact_forward(1, P, C)
    datasets = [("exact", c)] + ([(f, nc.family_inputs(f, 1, P, C)) for f in nc.FAMILIES] if P <= nc.BOUNDED_MAX_PIXELS else [])
    for family, d in datasets:
        part = nc.tile_partials(d["x"], tiles)
        ga, be = d["gamma"].to(DEV), d["beta"].to(DEV)
        for layout, relu, res, in_place in ((layouts[0], True, d["res"], False), (layouts[1], False, None, True),
                                            (layouts[1], True, d["res"], True)):
            xbuf, xv = nc.place(d["x"], layout, DEV)
            ol = _other(layout)
            rv = None if res is None else nc.place(res, ol, DEV)[1]
            obuf, ov = (xbuf, xv) if in_place else nc.place_out((1, P, C), torch.bfloat16, ol, DEV)
            got = _tile(lib, part.to(DEV), tiles, C, P, ga, be, xv, nc.layout_stride(layout, C), rv, nc.layout_stride(ol, C), relu, ov,
                        nc.layout_stride(layout if in_place else ol, C))
            assert nc.surroundings_untouched(obuf, layout if in_place else ol, C)
            f64 = nc.forward64(d["x"], d["gamma"], d["beta"], res=res, relu=relu, partials=part)
            got["y"] = ov
            if family == "exact":
                _check_finalize_exact(dict(got, scale=f64["scale"], shift=f64["shift"]), c, f64, d["gamma"], d["beta"], True)
            for k, v in nc.forward_figures(got, f64).items():
                _figure(k, v, f"tile {tiles}x{C} {family} {layout} in_place={in_place}")


# --------------------------------------------------------------------------------------------- the wrappers on strided slices
def _nchw(view, B, H, W):
    """[G, P, C] view (G P = B H W) -> the logical [B, C, H, W] tensor over the same memory"""
    C = view.shape[2]
    return view.reshape(-1, C).view(B, H, W, C).permute(0, 3, 1, 2) if view.is_contiguous() else \
        view.as_strided((B, H, W, C), (H * W * view.stride(1), W * view.stride(1), view.stride(1), 1), view.storage_offset()).permute(0, 3, 1, 2)


@pytest.mark.parametrize("kind,B,H,W,C", nc.WRAPPER_CASES)
@pytest.mark.parametrize("layout", ["dense", "slice8"])
def test_wrappers_on_slices(kind, B, H, W, C, layout):
    """hip.instance_norm / hip.batch_norm_train forward and backward, x / residual / dy as channel slices: y, the running
    statistics, dx, d(gamma), d(beta) against the float64 chain (the ReLU mask of BatchNorm from the stored output the kernel
    reads; nothing multiplied into the gradient), d(residual) = masked dy bit for bit"""
    from openess_amd import hip
    G, P = (B, H * W) if kind == "in" else (1, B * H * W)
    for family in nc.FAMILIES:
        d = nc.family_inputs(family, G, P, C)
        for relu in (False, True):
            with_res = (kind == "bn") or not relu                      # InstanceNorm has no ReLU after a residual add
            if kind == "in" and not nc.chain_case_ok(family, relu, False):
                continue                                               # xhat = 0 +- rounding everywhere: the mask has no float64 answer
            x4 = _nchw(nc.place(d["x"], layout, DEV)[1], B, H, W).detach().requires_grad_(True)
            r4 = _nchw(nc.place(d["res"], _other(layout), DEV)[1], B, H, W).detach().requires_grad_(True) if with_res else None
            g4 = _nchw(nc.place(d["dy"], _other(layout), DEV)[1], B, H, W)
            what = f"{kind} {B}x{C}x{H}x{W} {family} {layout} relu={relu}"
            if kind == "in":
                y = hip.instance_norm(x4, relu=relu, residual=r4)
                ga = be = None
            else:
                bn = torch.nn.BatchNorm2d(C).to(DEV).train()
                with torch.no_grad():
                    bn.weight.copy_(d["gamma"]), bn.bias.copy_(d["beta"])
                y = hip.batch_norm_train(x4, bn, relu=relu, residual=r4)
                ga, be = d["gamma"], d["beta"]
            y.backward(g4)
            flat = lambda t: t.detach().permute(0, 2, 3, 1).reshape(G, P, C)               # noqa: E731
            f64 = nc.forward64(d["x"], ga, be, res=d["res"] if with_res else None, relu=relu)
            _figure("y", nc.err_bf16(flat(y), f64["y"], f64["y_scale"]), what)
            yout = flat(y).cpu() if (relu and kind == "bn") else None
            b64 = nc.backward64(d["x"], d["dy"], f64["mean"], f64["rstd"], ga, relu, yout)
            cond = nc.chain_condition(f64)
            got = dict(dx=flat(x4.grad), s1=b64["s1"], s2=b64["s2"])
            if kind == "bn":
                got["s1"], got["s2"] = bn.bias.grad[None], bn.weight.grad[None]
                _check_running(bn.running_mean, bn.running_var, f64, P, C)
                assert int(bn.num_batches_tracked) == 1
            for k, v in nc.backward_figures(got, b64, cond).items():
                _figure(k, v, what)
            if with_res:
                assert torch.equal(_bits(flat(r4.grad)), _bits(b64["dres"].bfloat16())), what


# --------------------------------------------------------------------------------------------- the three copies
def _place4(t, layout, fill=NAN):
    B, H, W, C = t.shape
    buf, view = nc.place(t.reshape(1, B * H * W, C), layout, DEV, fill)
    return buf, view, nc.layout_stride(layout, C)


@pytest.mark.parametrize("B,H,W,C", nc.COPY_CASES)
def test_copies_bit_for_bit(lib, B, H, W, C):
    t = nc.copy_values(B, H, W, C, "in")
    for il, ol in (("dense", "dense"), ("slice8", "dense"), ("dense", "slice24"), ("slice24", "slice8")):
        _, iv, ips = _place4(t, il)
        # nearest x2
        obuf, ov, ops = _place4(torch.full((B, 2 * H, 2 * W, C), NAN, dtype=torch.bfloat16), ol)
        _check(lib.oess_upsample_nearest2x_nhwc_bf16(_p(iv), ips, B, H, W, C, _p(ov), ops, _st()), "upsample")
        assert torch.equal(_bits(ov.reshape(B, 2 * H, 2 * W, C)), _bits(nc.upsample2x_ref(t))) and nc.surroundings_untouched(obuf, ol, C)
        # its adjoint: the 2x2 sum
        gout = nc.copy_values(B, 2 * H, 2 * W, C, "gout")
        _, gv, gps = _place4(gout, il)
        obuf, ov, ops = _place4(torch.full((B, H, W, C), NAN, dtype=torch.bfloat16), ol)
        _check(lib.oess_downsample_sum2x_nhwc_bf16(_p(gv), gps, B, H, W, C, _p(ov), ops, _st()), "downsample")
        assert torch.equal(_bits(ov.reshape(B, H, W, C)), _bits(nc.downsample_sum2x_ref(gout))) and nc.surroundings_untouched(obuf, ol, C)
        # zero insertion
        for s, eh, ew in nc.ZERO_INSERT:
            Hz, Wz = (H - 1) * s + 1 + eh, (W - 1) * s + 1 + ew
            obuf, ov, ops = _place4(torch.full((B, Hz, Wz, C), NAN, dtype=torch.bfloat16), ol)
            _check(lib.oess_zero_insert_nhwc_bf16(_p(iv), ips, B, H, W, C, s, Hz, Wz, _p(ov), ops, _st()), "zero_insert")
            assert torch.equal(_bits(ov.reshape(B, Hz, Wz, C)), _bits(nc.zero_insert_ref(t, s, Hz, Wz))), (il, ol, s, eh, ew)
            assert nc.surroundings_untouched(obuf, ol, C)
