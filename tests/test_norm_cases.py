"""CPU half of the bf16 normalisation kernels' tests (tests/norm_cases.py holds the cases, tests/test_hip_norm_routes.py runs them
on the GPU): the fp32 models of norm_ops.hip reproduce every exact expectation bit for bit (a correct implementation passes),
norm_route puts every case on the route it names and every branch of the dispatch is entered by some case, the bounds are four
times the models' figures against float64, and each of seven one-line mutations of the model fails a new criterion while the old
one (randn, dense, 2e-2 on the bf16 output) lets three of them through.  No GPU."""
import functools

import numpy as np
import pytest
import torch

from tests import norm_cases as nc

CPU_EXACT_MAX = 40000             # the larger exact cases run through the model once, in test_large_exact_cases


def _small(cases):
    return [c for c in cases if c[1] * c[2] * c[3] <= CPU_EXACT_MAX * 72]


# --------------------------------------------------------------------------------------------- routes
@pytest.mark.parametrize("case", nc.all_cases(), ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}")
def test_case_takes_its_route(case):
    r = nc.route_of_case(case)
    for k, v in case[5].items():
        assert r[k] == v, (k, r[k], v)
    assert all(layout in nc.LAYOUTS for layout in case[4]) and case[4][0] == "dense"
    if case is not nc.CAP_CASE:
        assert any(layout != "dense" for layout in case[4])                # each runs at least once as a strided slice


def test_every_branch_is_entered_by_some_case():
    seen = set()
    for case in nc.all_cases():
        seen |= nc.branches(case)
    assert seen == nc.REQUIRED_BRANCHES, (nc.REQUIRED_BRANCHES - seen, seen - nc.REQUIRED_BRANCHES)
    # the figures of the issue's table, restated
    assert nc.norm_route("fwd", 8, 3000, 72)["unrolled_trips"] == 1 and nc.norm_route("fwd", 8, 2999 - 27 * 32, 72)["unrolled"] is False
    assert nc.norm_route("fwd", 1, 16384, 8)["empty_chunks"] == 0 and nc.norm_route("fwd", 1, 16385, 8)["empty_chunks"] == 3
    assert [nc.norm_route("bn_bwd", 1, P, 64)["chunks"] for P in nc.BN_FUSED_PIXELS] == list(nc.BN_FUSED_PIXELS.values())
    assert nc.norm_route("fwd", 1, 32768, 2048)["apply_capped"] is False and nc.norm_route("fwd", 1, 32769, 2048)["apply_capped"] is True
    assert nc.norm_route("tile", 1, 91, 64, tiles=1) == dict(groups=1, pixel_chunks=1, ppc=96, last_pixel_chunk=91, tiles=1, tile_trips=1)
    r = nc.norm_route("bn_bwd", 1, 33000, 256)
    assert (r["pixel_chunks"], r["ppc"], r["last_pixel_chunk"]) == (258, 128, 104)


def test_layouts_surround_the_slice_with_nan():
    t = nc.exact_forward(1, 63, 24)["x"]
    for layout, (c0, extra) in nc.LAYOUTS.items():
        buf, view = nc.place(t, layout)
        assert torch.equal(view, t) and view.stride(1) == 24 + extra == nc.layout_stride(layout, 24) and view.data_ptr() % 16 == 0
        assert buf.shape == (63, 24 + extra) and nc.surroundings_untouched(buf, layout, 24)
        assert int(torch.isnan(buf).sum()) == 63 * extra
        obuf, oview = nc.place_out((1, 63, 24), torch.bfloat16, layout)
        assert bool(torch.isnan(obuf).all()) and oview.shape == t.shape
        if extra:
            assert bool(torch.isnan(nc.kernel_view(buf, view, "strided_as_dense")).any())
            obuf[0, 0] = 1.0
            assert not nc.surroundings_untouched(obuf, layout, 24)


# --------------------------------------------------------------------------------------------- the model on the exact cases
def _check_exact_forward(G, ppg, C):
    c = nc.exact_forward(G, ppg, C)
    x = c["x"]
    assert x.dtype == torch.bfloat16 and int(c["Q"].max()) < nc.LIMIT
    S, Q = nc.stats_model(x)
    assert torch.equal(S, c["S"].double()) and torch.equal(Q, c["Q"].double())
    rm0, rv0 = torch.zeros(C), torch.ones(C)               # a fresh nn.BatchNorm2d: a relative tolerance needs an update without cancellation
    f = nc.finalize_model(S, Q, ppg, nc.EPS, c["gamma"], c["beta"], (rm0, rv0) if G == 1 else None)
    f64 = nc.forward64(x, c["gamma"], c["beta"])
    assert torch.equal(f["mean"], (c["S"].double() / ppg).float())                  # the float64 quotient rounded once
    assert nc.ulps_fp32(f["rstd"], f64["rstd"]) <= nc.RSTD_ULPS
    bs, bh = nc.finalize_bounds(f64, c["gamma"], c["beta"])
    assert bool(((f["scale"].double() - f64["scale"]).abs() <= bs).all()) and bool(((f["shift"].double() - f64["shift"]).abs() <= bh).all())
    if G == 1:
        rm, rv = nc.running64(f64["mean"], f64["var"], ppg, rm0, rv0)
        np.testing.assert_allclose(f["running_mean"].numpy(), rm.numpy(), rtol=nc.RUNNING_MEAN_RTOL, atol=1e-9)
        np.testing.assert_allclose(f["running_var"].numpy(), rv.numpy(), rtol=nc.RUNNING_VAR_RTOL)
    for (relu, res), y in c["y"].items():
        assert torch.equal(nc.apply_model(x, c["scale"], c["shift"], c["res"] if res else None, relu), y)
        ref = x.double() * c["scale"].double()[:, None] + c["shift"].double()[:, None] + (c["res"].double() if res else 0.0)
        assert torch.equal(ref.clamp_min(0.0) if relu else ref, y.double())


def _check_exact_backward(G, ppg, C, with_yout):
    c = nc.exact_backward(G, ppg, C, with_yout)
    gamma = c["gamma"] if with_yout else None
    for relu in (False, True):
        m = nc.backward_model(c["x"], c["dy"], c["mean"], c["rstd"], relu, gamma, c["yout"])
        e = c[relu]
        assert torch.equal(m["s1"].double(), e["s1"]) and torch.equal(m["s2"].double(), e["s2"])
        assert torch.equal(m["dres"].view(torch.int16), e["dres"].view(torch.int16))
        b64 = nc.backward64(c["x"], c["dy"], c["mean"], c["rstd"], gamma, relu, c["yout"])
        assert torch.equal(b64["s1"], e["s1"]) and torch.equal(b64["s2"], e["s2"]) and torch.equal(b64["dres"], e["dres"].double())
        assert nc.err_bf16(m["dx"], b64["dx"], b64["dx_scale"]) <= nc.BOUND["dx"]


@pytest.mark.parametrize("case", _small(nc.FWD_CASES), ids=lambda c: c[0])
def test_model_reproduces_the_exact_forward(case):
    _check_exact_forward(*case[1:4])


@pytest.mark.parametrize("case", _small(nc.BN_BWD_CASES + nc.IN_BWD_CASES), ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}")
def test_model_reproduces_the_exact_backward(case):
    _check_exact_backward(case[1], case[2], case[3], with_yout=nc.case_kind(case[0]) == "bn_bwd")


def test_large_exact_cases():
    """the sums of the largest shapes stay below 2^24 and the model adds them exactly: rows = 256 with the x4 loop, and the
    512-row backward"""
    c = nc.exact_forward(1, 262149, 8)
    S, Q = nc.stats_model(c["x"])
    assert torch.equal(S, c["S"].double()) and torch.equal(Q, c["Q"].double()) and int(c["Q"].max()) > nc.LIMIT // 4
    _check_exact_backward(1, 33000, 64, True)


@pytest.mark.parametrize("C,tiles", [(64, 1), (64, 17), (256, 70)])
def test_model_reproduces_the_exact_tile_route(C, tiles):
    P = 128 * tiles - 37
    c = nc.exact_forward(1, P, C)
    part = nc.tile_partials(c["x"], tiles)
    assert torch.equal(part[:, 0].double().sum(0), c["S"][0].double()) and torch.equal(part[:, 1].double().sum(0), c["Q"][0].double())
    f = nc.forward_model(c["x"], c["gamma"], c["beta"], partials=part)
    assert torch.equal(f["mean"], (c["S"].double() / P).float())
    assert nc.ulps_fp32(f["rstd"], nc.forward64(c["x"], c["gamma"], c["beta"], partials=part)["rstd"]) <= nc.RSTD_ULPS


def test_copy_references():
    t = nc.copy_values(2, 3, 5, 8, "t")
    up = nc.upsample2x_ref(t)
    assert up.shape == (2, 6, 10, 8) and all(torch.equal(up[:, dy::2, dx::2], t) for dy in (0, 1) for dx in (0, 1))
    z = nc.zero_insert_ref(t, 3, 9, 14)
    assert torch.equal(z[:, 0:7:3, 0:13:3], t) and int((z != 0).sum()) == t.numel()
    d = nc.downsample_sum2x_ref(up)
    assert torch.equal(d, (4.0 * t.double()).bfloat16())
    g = nc.copy_values(2, 6, 10, 8, "g")
    s = g.float()
    fp32 = (s[:, 0::2, 0::2] + s[:, 0::2, 1::2]) + (s[:, 1::2, 0::2] + s[:, 1::2, 1::2])       # exact in any order
    assert torch.equal(nc.downsample_sum2x_ref(g), fp32.bfloat16())


# --------------------------------------------------------------------------------------------- bounds
@functools.lru_cache(maxsize=None)
def _measured():
    return nc.measure()


def test_bounds_are_four_times_the_models_figures():
    worst = _measured()
    assert set(worst) == set(nc.MODEL_FIGURE) == set(nc.BOUND)
    for k, const in nc.MODEL_FIGURE.items():
        assert abs(worst[k][0] - const) <= 5e-3 * const, (k, worst[k], const)      # the constant is the figure to three digits
        assert nc.BOUND[k] == 4.0 * const


def test_bounded_cases_cover_the_families_and_the_routes():
    cases = nc.bounded_cases()
    assert {c[0] for c in cases} == {"fwd", "in_bwd", "bn_bwd", "tile"} and all(c[3] <= nc.BOUNDED_MAX_PIXELS for c in cases)
    assert len(cases) == len(nc.all_cases()) - 1 - 1 - 2                   # all but the cap case, 262149 pixels and the 512-tile pair
    d = nc.family_inputs("constant", 2, 63, 24)
    assert bool((nc.forward64(d["x"])["var"] == 0).all())
    d = nc.family_inputs("single", 2, 63, 24)
    assert bool(((d["x"] != 0).sum(1) == 1).all())
    d = nc.family_inputs("large_mean", 1, 1050, 64)
    f = nc.forward64(d["x"])
    assert float((f["ex2"] / f["var"]).min()) > 3000.0


# --------------------------------------------------------------------------------------------- mutations
def _new_criteria(mutate):
    """names of the new criteria the mutated model fails"""
    failed = []
    # exact sums, strided, three groups
    c = nc.exact_forward(3, 130, 72)
    buf, view = nc.place(c["x"], "slice8")
    S, Q = nc.stats_model(nc.kernel_view(buf, view, mutate), mutate=mutate)
    if not (torch.equal(S, c["S"].double()) and torch.equal(Q, c["Q"].double())):
        failed.append("exact sums")
    f = nc.finalize_model(S, Q, 130, nc.EPS, c["gamma"], c["beta"], mutate=mutate)
    f64 = nc.forward64(c["x"], c["gamma"], c["beta"])
    bs, bh = nc.finalize_bounds(f64, c["gamma"], c["beta"])
    if not (bool(((f["scale"].double() - f64["scale"]).abs() <= bs).all()) and bool(((f["shift"].double() - f64["shift"]).abs() <= bh).all())):
        failed.append("scale / shift within the derived bound")
    # running statistics
    c = nc.exact_forward(1, 63, 24)
    rm0, rv0 = torch.zeros(24), torch.ones(24)
    S, Q = nc.stats_model(c["x"])
    f = nc.finalize_model(S, Q, 63, running=(rm0, rv0), mutate=mutate)
    f64 = nc.forward64(c["x"])
    rv = nc.running64(f64["mean"], f64["var"], 63, rm0, rv0)[1]
    if not np.allclose(f["running_var"].numpy(), rv.numpy(), rtol=nc.RUNNING_VAR_RTOL, atol=0):
        failed.append("running variance at 1e-6")
    # bounded forward
    d = nc.family_inputs("randn", 1, 1050, 64)
    figs = nc.forward_figures(nc.forward_model(d["x"], mutate=mutate), nc.forward64(d["x"]))
    failed += [f"{k} within its bound" for k, v in figs.items() if not v <= nc.BOUND[k]]
    # exact backward with a stored output
    c = nc.exact_backward(1, 1050, 72, True)
    m = nc.backward_model(c["x"], c["dy"], c["mean"], c["rstd"], True, c["gamma"], c["yout"], mutate=mutate)
    if not (torch.equal(m["s1"].double(), c[True]["s1"]) and torch.equal(m["s2"].double(), c[True]["s2"])):
        failed.append("exact d(beta) / d(gamma)")
    if not torch.equal(m["dres"].view(torch.int16), c[True]["dres"].view(torch.int16)):
        failed.append("d(residual) bit for bit")
    # bounded backward
    mean, rstd = nc.fp32_stats_of(d["x"])
    got = nc.backward_model(d["x"], d["dy"], mean, rstd, False, d["gamma"], None, mutate=mutate)
    figs = nc.backward_figures(got, nc.backward64(d["x"], d["dy"], mean, rstd, d["gamma"]))
    failed += [f"{k} within its bound" for k, v in figs.items() if not v <= nc.BOUND[k]]
    return failed


def _old_criterion_passes(mutate):
    """what tests/test_hip_norms.py asserts, on the model: randn, dense, torch-fp32-class reference, rtol = atol = 2e-2 on the bf16
    output (3e-2 on dx, 2e-2 / 5e-2 on d(gamma) and d(beta), 1e-2 on d(residual)), the running statistics at 1e-4 / 1e-5, the
    upstream gradient multiplied by both ReLU masks; at its first InstanceNorm shape (2, 32, 20, 28) with ReLU and at the
    shape of test_batch_norm_train_fwd_bwd (4, 64, 9, 13) with every combination of ReLU and residual"""
    g = torch.Generator().manual_seed(0)

    def close(a, b, tol):
        return bool(np.allclose(a.double().numpy(), b.double().numpy(), rtol=tol, atol=tol))

    ok = True
    x = (torch.randn(2, 560, 32, generator=g) * 2 + 0.5).bfloat16()
    dy = torch.randn(2, 560, 32, generator=g).bfloat16()
    buf, view = nc.place(x, "dense")
    xk = nc.kernel_view(buf, view, mutate)
    f64 = nc.forward64(x, relu=True)
    S, Q = nc.stats_model(xk, mutate=mutate)
    f = nc.finalize_model(S, Q, 560, mutate=mutate)
    ok &= close(nc.apply_model(x, f["scale"], f["shift"], None, True), f64["y"], 2e-2)
    m = nc.backward_model(x, dy, f["mean"], f["rstd"], True, mutate=mutate)
    ok &= close(m["dx"], nc.backward64(x, dy, f64["mean"], f64["rstd"], None, True)["dx"], 3e-2)
    # test_batch_norm_train_fwd_bwd: (4, 64, 9, 13) with an affine, every combination of ReLU and residual
    x = (torch.randn(1, 468, 64, generator=g) * 2 + 0.5).bfloat16()
    res0, dy = torch.randn(1, 468, 64, generator=g).bfloat16(), torch.randn(1, 468, 64, generator=g).bfloat16()
    gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2
    rm0, rv0 = torch.zeros(64), torch.ones(64)
    for relu, with_res in ((True, True), (True, False), (False, False), (False, True)):
        res = res0 if with_res else None
        f64 = nc.forward64(x, gamma, beta, res=res, relu=relu)
        f = nc.forward_model(x, gamma, beta, res=res, relu=relu, running=(rm0, rv0), mutate=mutate)
        ok &= close(f["y"], f64["y"], 2e-2)
        rm, rv = nc.running64(f64["mean"], f64["var"], 468, rm0, rv0)
        ok &= bool(np.allclose(f["running_mean"].numpy(), rm.numpy(), rtol=1e-4, atol=1e-5))
        ok &= bool(np.allclose(f["running_var"].numpy(), rv.numpy(), rtol=1e-4, atol=1e-5))
        dyk = (dy.double() * (f["y"].double() > 0) * (f64["y"] > 0)).bfloat16() if relu else dy      # both masks multiplied in
        m = nc.backward_model(x, dyk, f["mean"], f["rstd"], relu, gamma, f["y"] if relu else None, mutate=mutate)
        b64 = nc.backward64(x, dyk, f64["mean"], f64["rstd"], gamma, relu, f64["y"] if relu else None)
        ok &= close(m["dx"], b64["dx"], 3e-2)
        ok &= bool(np.allclose(m["s1"].numpy(), b64["s1"].numpy(), rtol=2e-2, atol=5e-2))
        ok &= bool(np.allclose(m["s2"].numpy(), b64["s2"].numpy(), rtol=2e-2, atol=5e-2))
        if with_res and relu:
            ok &= bool(np.allclose(m["dres"].double().numpy(), b64["dres"].numpy(), rtol=1e-2, atol=1e-2))
    return ok


# mutation -> (a new criterion it must fail, whether the old criterion lets it through); DESIGN.md carries the table
MUTATION_TABLE = {
    "drop_last_pixel": ("exact sums", False),      # 63-pixel chunks at the old shapes: 1.6 % of the pixels, seen through flipped ReLU masks
    "strided_as_dense": ("exact sums", True),      # the old tensors are dense
    "no_group_offset": ("exact sums", False),
    "gamma_i": ("scale / shift within the derived bound", True),       # never reached: no affine with G > 1
    "biased_running_var": ("running variance at 1e-6", False),         # 468 pixels: 2e-3 of the variance against 1e-4
    "mask_from_xhat": ("exact d(beta) / d(gamma)", False),             # caught with a residual only; both masks hide the rest
    "ppg_plus_1": ("dx within its bound", True),
}


def test_the_unmutated_model_passes_both_criteria():
    assert _new_criteria(None) == [] and _old_criterion_passes(None)


@pytest.mark.parametrize("mutate", nc.MUTATIONS)
def test_each_mutation_fails_a_new_criterion(mutate, capsys):
    failed = _new_criteria(mutate)
    old = _old_criterion_passes(mutate)
    with capsys.disabled():
        print(f"\n  mutation {mutate}: fails {failed}; old criterion {'passes' if old else 'fails'}")
    assert MUTATION_TABLE[mutate][0] in failed, failed
    assert old == MUTATION_TABLE[mutate][1]


def test_mutation_table_names_every_mutation():
    assert tuple(MUTATION_TABLE) == nc.MUTATIONS
