"""CPU half of the bilinear resize / L2-normalise kernels' tests (tests/resize_cases.py holds the cases, tests/test_hip_resize_routes.py
runs them on the GPU): the restated routes put every case where it says and enter every branch, the float64 references agree with
torch's own float64 F.interpolate / F.normalize autograd (to 1e-12 where the index rule does not matter, to the measured fp32-lambda
difference elsewhere), the fp32 models of the kernels reproduce every exact expectation bit for bit in both associations, each
mutation of a model fails an exact case, and the bounds in use are four times the re-measured model figures.  No GPU."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import resize_cases as rc

F64 = torch.float64


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# --------------------------------------------------------------------------------------------- routes
def test_every_case_takes_its_route_and_every_branch_is_entered():
    for c in rc.resize_cases():
        r = rc.resize_route(c[1] == "bf16", *c[2:7], layouts=("dense", "slice_vec"))
        for k, v in c[8].items():
            assert r[k] == v, (c, k, r[k])
        for pair in rc.LAYOUT_PAIRS[2:]:
            assert rc.resize_route(c[1] == "bf16", *c[2:7], layouts=pair)["kernel"] == "scalar"
    assert rc.branches() == rc.REQUIRED_BRANCHES, (rc.REQUIRED_BRANCHES - rc.branches(), rc.branches() - rc.REQUIRED_BRANCHES)
    # the figures of the issue, restated
    assert rc.resize_route(True, 2, 65, 256, 4, 260)["lds_bytes"] == 66560 > rc.LDS_LIMIT
    assert rc.resize_route(True, 3, 5, 192, 12, 20)["idle_lanes"] == 16
    assert rc.l2norm_route(False, 4 * rc.GRID_CAP, 3)["capped"] is False and rc.l2norm_route(False, *rc.L2_CAP_CASE[1:])["capped"] is True
    assert rc.l2norm_route(False, rc.L2_CAP_CASE[1], 3)["grid"] == rc.GRID_CAP          # 2 blocks of pixels more: crossed once
    assert [rc.l2norm_route(True, 5, C)["lpp"] for C in (64, 128, 256, 512)] == [8, 16, 32, 64]
    assert [rc.l2norm_route(False, 5, C)["lpp"] for C in (32, 64, 128, 256)] == [8, 16, 32, 64]
    assert rc.fused_route(*rc.FUSED_CAP_CASE)["capped"] and not rc.fused_route(1, 64, 64, 192, 4)["capped"]
    assert rc.fused_route(*rc.FUSED_NT_CASE)["nt_out"] and not rc.fused_route(1, *rc.FUSED_NT_CASE[1:])["nt_out"]
    assert 5 * 256 * 256 * 512 * 2 == 335544320
    assert [rc.fused_route(2, 3, 3, C, 3)["kernel"] for C in (192, 320, 448)] == ["scalar"] * 3
    assert rc.pool_route(33, 64) == dict(lpp=8, G=32, iterations=2, carry_used=True) and not rc.pool_route(32, 64)["carry_used"]


def test_layouts():
    for dt, dtype in rc.DTYPES.items():
        bf = dt == "bf16"
        t = rc.ints((2, 3, 5, 8), "layout").to(dtype)
        for layout, (c0, extra) in rc.LAYOUTS.items():
            buf, view = rc.place(t, layout)
            assert torch.equal(view, t) and view.stride(2) == 8 + extra == rc.layout_stride(layout, 8)
            assert rc.surroundings_untouched(buf, layout, 8) and int(torch.isnan(buf).sum()) == 30 * extra
            aligned = view.data_ptr() % 16 == 0 and view.stride(2) % (8 if bf else 4) == 0
            assert aligned == rc.vec_ok(layout, 8, bf) == (layout != "slice_odd")
            if extra:
                assert bool(torch.isnan(rc.kernel_view(buf, view, "strided_as_dense")).any())
                obuf, _ = rc.place_out((2, 3, 5, 8), dtype, layout)
                obuf[0, 0] = 1.0
                assert not rc.surroundings_untouched(obuf, layout, 8)
    for pair in rc.LAYOUT_PAIRS:
        assert pair[0] != pair[1]
    for tr in rc.LAYOUT_TRIPLES:
        assert tr[0] != tr[1] and tr[1] != tr[2]


# --------------------------------------------------------------------------------------------- references against torch
def _nchw(t):
    return t.permute(0, 3, 1, 2)


# ATen's float64 path forms the source coordinate in double, the kernels (and the references) in fp32: two roundings on a coordinate
# below 16 move lambda by at most 16 x 2^-23 per axis, and a value by twice that times 2 max|x| over the two axes.  Measured: 8.3e-7.
LAMBDA_DIFF = 64 * 2.0 ** -23


def test_bilinear_references_agree_with_torch_float64():
    worst_exact, worst_other = 0.0, 0.0
    geoms = [(H, W, Ho, Wo, a, True) for (H, W, Ho, Wo, a) in rc.GEOMS] + \
            [(H, W, Ho, Wo, a, False) for (_, H, W, _, Ho, Wo, a) in rc.BOUNDED_GEOMS]
    for (H, W, Ho, Wo, align, dyadic) in geoms:
        x = torch.randn(2, H, W, 3, dtype=F64, generator=rc._gen("ref", H, W, Ho, Wo)).requires_grad_(True)
        ref = F.interpolate(_nchw(x), size=(Ho, Wo), mode="bilinear", align_corners=align)
        g = torch.randn(2, Ho, Wo, 3, dtype=F64, generator=rc._gen("refg", H, W, Ho, Wo))
        ref.backward(_nchw(g))
        d = max(float((rc.resize_fwd64(x.detach(), Ho, Wo, align) - ref.detach().permute(0, 2, 3, 1)).abs().max()),
                float((rc.resize_bwd64(g, H, W, align) - x.grad).abs().max()) / max(1.0, Ho * Wo / (H * W)))
        if dyadic:
            worst_exact = max(worst_exact, d)
        else:
            worst_other = max(worst_other, d / float(x.detach().abs().max()))
    print(f"references vs torch float64: dyadic {worst_exact:.3e}, fp32-lambda difference {worst_other:.3e}")
    assert worst_exact <= 1e-12
    assert worst_other <= LAMBDA_DIFF


def test_l2_references_agree_with_torch_float64():
    eps = rc.EPS_TEST
    x = torch.randn(9, 40, dtype=F64, generator=rc._gen("l2ref"))
    x[0] = 0.0
    x[1] *= 1e-5                                          # |x| below eps: y = x / eps
    x.requires_grad_(True)
    y = F.normalize(x, p=2, dim=-1, eps=eps)
    g = torch.randn(9, 40, dtype=F64, generator=rc._gen("l2refg"))
    y.backward(g)
    y64, inv = rc.l2_fwd64(x.detach(), eps)
    assert float((y64 - y.detach()).abs().max()) <= 1e-12 and float(inv[0]) == 1.0 / eps == float(inv[1])
    assert float(((rc.l2_bwd64(y64, g, inv, eps) - x.grad).abs() / inv[:, None]).max()) <= 1e-12
    assert torch.equal(rc.l2_bwd64(y64, g, inv, eps)[:2], g[:2] / eps)


def test_pooled_reference_agrees_with_torch_float64():
    """scatter_mean(normalize(upsample(x))) through autograd in float64, against the composed reference on the saved map"""
    B, H, W, C, s, sps = 2, 3, 3, 5, 3, rc.POOL_SPS          # ratio 2 / 8: the index rule does not matter
    Ho, Wo, S = H * s, W * s, rc.POOL_S
    x = torch.randn(B, H, W, C, dtype=F64, generator=rc._gen("poolref")).requires_grad_(True)
    up = F.interpolate(_nchw(x), scale_factor=s, mode="bilinear", align_corners=True)
    y = F.normalize(up, p=2, dim=1, eps=1e-12).permute(0, 2, 3, 1).reshape(-1, C)
    ids = rc.pool_ids(B, Ho, Wo, sps)
    gid = ids + torch.arange(B).repeat_interleave(Ho * Wo) * sps
    ok = (gid >= 0) & (gid < S)
    sums = torch.zeros(S, C, dtype=F64).index_add(0, gid[ok], y[ok])
    count = torch.zeros(S, dtype=F64).index_add(0, gid[ok], torch.ones(int(ok.sum()), dtype=F64))
    den = (count.float() + torch.tensor(1e-6)).double()
    gk = torch.randn(S, C, dtype=F64, generator=rc._gen("poolrefg"))
    ((sums / den[:, None]) * gk).sum().backward()
    inv = 1.0 / up.detach().permute(0, 2, 3, 1).norm(dim=-1).reshape(-1)
    got = rc.pool_bwd64(y.detach().view(B, Ho, Wo, C), inv, ids, gk, count, sps, H, W, 1e-12)
    assert float((got - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max()) * 10


# --------------------------------------------------------------------------------------------- the models on the exact cases
@pytest.mark.parametrize("geom", rc.GEOMS + tuple((H, W, Ho, Wo, False) for (_, H, W, _, Ho, Wo, _) in rc.UP_ROWS_LIMITS[:2]),
                         ids=lambda g: "x".join(map(str, g)))
def test_models_reproduce_the_exact_resize(geom):
    H, W, Ho, Wo, align = geom
    for dt, chans in rc.GENERIC_CHANNELS.items():
        for C in chans[:2] + chans[-1:]:
            c = rc.exact_resize(dt, H, W, C, Ho, Wo, align)
            for order in ("aten", "up_rows"):             # exact data: both associations give the reference's bits
                assert _same(rc.resize_fwd_model(c["x"], Ho, Wo, align, order), c["y"]), (dt, C, order)
            assert _same(rc.resize_bwd_model(c["g"], H, W, align), c["gin"]), (dt, C)
            if dt == "f32":                               # fp32 and float64 F.interpolate agree exactly on these geometries
                for cast_to in (torch.float32, F64):
                    x = c["x"].to(cast_to).clone().requires_grad_(True)
                    y = F.interpolate(_nchw(x), size=(Ho, Wo), mode="bilinear", align_corners=align)
                    y.backward(_nchw(c["g"].to(cast_to)))
                    assert torch.equal(y.detach().permute(0, 2, 3, 1).double(), c["y"].double())
                    assert torch.equal(x.grad.double(), c["gin64"])


@pytest.mark.parametrize("dt,P,C", rc.l2_cases(), ids=lambda v: str(v))
def test_models_reproduce_the_exact_l2(dt, P, C):
    c = rc.exact_l2(dt, P, C)
    y, inv = rc.l2_fwd_model(c["x"], rc.EPS_TEST)
    y64, inv64 = rc.l2_fwd64(c["x"], rc.EPS_TEST)
    # three correctly rounded operations (sqrt, divide, product) on an exact sum: 1.5 ulp of y before its own rounding
    assert float(((inv.double() - inv64).abs() / inv64).max()) <= 2.0 ** -23
    fig = rc.l2_fwd_figures(y, inv, c["x"], rc.EPS_TEST)
    assert fig["l2_fwd_y"] <= 3 * 2.0 ** -24 and fig["l2_fwd_inv"] <= 2.0 ** -23
    if P >= 5:
        assert float(inv[0]) == float(inv[1]) == float(inv[3]) == 1024.0 and float(inv[2]) < 1024.0 and bool((y[0] == 0).all())
        assert torch.equal(y[1].double(), c["x"][1].double() * 1024.0) and float(y[4].abs().max()) == 1.0
    assert _same(rc.l2_bwd_model(c["y"], c["g"], c["inv"], rc.EPS_TEST), c["gx"])
    assert bool((c["inv"] == 1024.0).any())               # inv == 1 / eps exactly: the clamped side


@pytest.mark.parametrize("H,W,scale", rc.FUSED_EXACT_GEOMS)
def test_models_reproduce_the_exact_fused(H, W, scale):
    for C in (64, 192):
        c = rc.exact_fused(H, W, scale, C)
        for kernel in ("vec", "scalar"):
            assert _same(rc.fused_model(c["x"], scale, False, kernel)[0], c["y"]), (C, kernel)


@pytest.mark.parametrize("geom", rc.POOL_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_models_reproduce_the_exact_pooled_backward(geom):
    H, W, Ho, Wo = geom
    for C in rc.POOL_CHANNELS if W > 3 else (64,):
        c = rc.exact_pool(H, W, Ho, Wo, C)
        got = rc.pool_bwd_model(c["feat"], c["inv"], c["ids"], c["gk"], c["count"], c["sps"], H, W, rc.EPS_TEST)
        assert _same(got, c["gin"]), C
        assert int((c["inv"] >= 1024.0).sum()) == 2


def test_the_issues_wide_pool_geometry_is_not_dyadic():
    """(2, 33) -> (8, 129) has the vertical ratio 1/7: its lambdas are no multiples of 2^-20, so it has no bit-exact answer"""
    lam = rc.axis_index(2, 8, True)[3].double()
    assert not bool((lam * 2.0 ** 20 == (lam * 2.0 ** 20).round()).all())
    lam = rc.axis_index(2, 9, True)[3].double()
    assert bool((lam * 8 == (lam * 8).round()).all())


def test_the_issues_wide_pool_geometry_runs_bounded():
    H, W, Ho, Wo = rc.POOL_ISSUE_WIDE
    for C in rc.POOL_CHANNELS:
        c = rc.wide_pool(C)
        got = rc.pool_bwd_model(c["feat"], c["inv"], c["ids"], c["gk"], c["count"], c["sps"], H, W, rc.EPS_TEST)
        assert rc.pool_figure(got, c["feat"], c["inv"], c["ids"], c["gk"], c["count"], c["sps"], H, W, rc.EPS_TEST) <= rc.BOUND["pool_bwd"]
        lost = rc.pool_bwd_model(c["feat"], c["inv"], c["ids"], c["gk"], c["count"], c["sps"], H, W, rc.EPS_TEST, "carry_lost")
        assert rc.pool_figure(lost, c["feat"], c["inv"], c["ids"], c["gk"], c["count"], c["sps"], H, W, rc.EPS_TEST) > 1e3 * rc.pool_bound()


# --------------------------------------------------------------------------------------------- bounds
@functools.lru_cache(maxsize=None)
def _measured():
    return rc.measure()


def test_bounds_are_four_times_the_models_figures():
    worst = _measured()
    assert set(worst) == set(rc.MODEL_FIGURE) == set(rc.BOUND)
    for k, const in rc.MODEL_FIGURE.items():
        assert abs(worst[k][0] - const) <= 5e-3 * const, (k, worst[k], const)      # the constant is the figure to three digits
        assert rc.BOUND[k] == 4.0 * const


# --------------------------------------------------------------------------------------------- mutations
def _failed_exact_cases(mutate):
    """names of the exact criteria the mutated models fail"""
    failed = []
    for (H, W, Ho, Wo, align) in ((3, 5, 12, 20, False), (5, 3, 17, 9, True), (40, 24, 5, 3, False), (5, 7, 5, 7, True)):
        for dt, C in (("bf16", 8), ("f32", 4)):
            c = rc.exact_resize(dt, H, W, C, Ho, Wo, align)
            xbuf, xv = rc.place(c["x"], "slice_vec")
            gbuf, gv = rc.place(c["g"], "slice_vec")
            for order in rc.model_orders(dt, H, W, C, Ho, Wo):
                if not _same(rc.resize_fwd_model(rc.kernel_view(xbuf, xv, mutate), Ho, Wo, align, order, mutate), c["y"]):
                    failed.append(f"resize forward {order}")
            if not _same(rc.resize_bwd_model(rc.kernel_view(gbuf, gv, mutate), H, W, align, mutate), c["gin"]):
                failed.append("resize backward")
    c = rc.exact_l2("f32", 37, 64)
    xbuf, xv = rc.place(c["x"], "slice_vec")
    y0, inv0 = rc.l2_fwd_model(c["x"], rc.EPS_TEST)
    y, inv = rc.l2_fwd_model(rc.kernel_view(xbuf, xv, mutate), rc.EPS_TEST, mutate)
    if not (_same(y, y0) and _same(inv, inv0)):
        failed.append("l2 forward")
    xs = rc.ints((37, 64), "l2 x for y")                  # the mutation that projects with x reads something that is not y
    if not _same(rc.l2_bwd_model(c["y"], c["g"], c["inv"], rc.EPS_TEST, mutate, x=xs.float()), c["gx"]):
        failed.append("l2 backward")
    for (H, W, Ho, Wo) in rc.POOL_GEOMS[1:]:
        p = rc.exact_pool(H, W, Ho, Wo, 64)
        got = rc.pool_bwd_model(p["feat"], p["inv"], p["ids"], p["gk"], p["count"], p["sps"], H, W, rc.EPS_TEST, mutate)
        if not _same(got, p["gin"]):
            failed.append(f"pooled backward W={W}")
    return failed


# mutation -> an exact criterion it must fail
MUTATION_TABLE = {
    "other_align_mode": "resize forward aten",
    "no_edge_clamp": "resize forward aten",
    "no_max0": "resize forward up_rows",
    "short_candidates": "resize backward",
    "swap_x_weights": "resize forward aten",
    "tmp_bf16": "pooled backward W=7",        # integer gradients of magnitude <= 3 leave a bf16-exact resize intermediate: see below
    "strided_as_dense": "resize forward aten",
    "l2_no_clamp": "l2 forward",
    "l2_proj_x": "l2 backward",
    "carry_lost": "pooled backward W=33",
}


def test_the_unmutated_models_pass():
    assert _failed_exact_cases(None) == []


@pytest.mark.parametrize("mutate", rc.MUTATIONS)
def test_each_mutation_fails_an_exact_case(mutate, capsys):
    failed = sorted(set(_failed_exact_cases(mutate)))
    with capsys.disabled():
        print(f"\n  mutation {mutate}: fails {failed}")
    assert MUTATION_TABLE[mutate] in failed, failed


def test_a_bf16_intermediate_fails_the_resize_backward_bound():
    """the plain resize backward's fp32 intermediate holds multiples of 1/8 below 24 on the exact data, which bf16 carries; there
    the bounded criterion is the one that sees it rounded"""
    dt, H, W, C, Ho, Wo, align = rc.BOUNDED_GEOMS[0]
    _, g = rc.resize_family_inputs("randn", dt, H, W, C, Ho, Wo)
    assert rc.resize_bwd_figure(rc.resize_bwd_model(g, H, W, align), g, H, W, align) <= rc.BOUND["resize_bwd_bf16"]
    assert rc.resize_bwd_figure(rc.resize_bwd_model(g, H, W, align, "tmp_bf16"), g, H, W, align) > 100 * rc.BOUND["resize_bwd_bf16"]


def test_mutation_table_names_every_mutation():
    assert tuple(MUTATION_TABLE) == rc.MUTATIONS
