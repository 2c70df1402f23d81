"""CPU half of the fp32 ViT token kernels' tests (tests/vit_f32_cases.py holds the cases, tests/test_hip_vit_f32.py runs them on the
GPU): the fp32 model of the attention kernel reproduces every exact expectation bit for bit (a correct kernel passes), each of
three one-line mutations of the kernel is caught by an exact case, the figures in the module are what the model or torch fp32
shows against float64 (the bounds are four times them), every LayerNorm case takes the route it names, a one-pass variance falls
outside the bound on the large-mean families, and the integer GEMM cases are exact by construction.  No GPU."""
import math

import pytest
import torch

from tests import vit_f32_cases as fc

EXACT = [(f, B, L, h) for f in ("selection", "constant_v") for (B, L, h) in fc.exact_shapes()]


def _holds(measured, figure):
    """the constant in the module is the figure measured here, to a quarter either way (another CPU's vector width moves the last
    digits of an fp32 sum); the factor of four of the bound is applied to the constant"""
    return measured <= 1.25 * figure and figure <= 1.25 * measured


@pytest.mark.parametrize("family,B,L,heads", EXACT)
def test_model_reproduces_the_exact_expectation(family, B, L, heads):
    c = fc.exact_case(family, B, L, heads)
    assert c["qkv"].dtype == c["expect"].dtype == torch.float32
    assert c["qkv"].shape == (B * L, 3 * heads * 64) and c["expect"].shape == (B * L, heads * 64)
    assert bool((c["qkv"][:, 2 * heads * 64:] != 0).all())  # V is never zero: an output of 0 is always an error
    assert torch.equal(fc.attention_model_f32(c["qkv"], B, L, heads), c["expect"])
    assert float((fc.attention64(c["qkv"], B, L, heads) - c["expect"].double()).abs().max()) < 1e-9


@pytest.mark.parametrize("B,heads", fc.ATT_BH)
def test_each_kernel_mutation_breaks_an_exact_case(B, heads):
    """mask `key > L`: the zero-filled row at key L scores 0 against <= -64 and takes the softmax of the constant-V case (any L that
    is no multiple of 64).  V rows read in natural order: the weight of the selected key lands on another V row (selection, every
    L >= 7 here).  Rows past L left as loaded: 0 * NaN behind the last batch, or the next batch's rows scored (both cases, any L
    that is no multiple of 64)."""
    for L in fc.ATT_L:
        sel, con = fc.exact_case("selection", B, L, heads), fc.exact_case("constant_v", B, L, heads)
        ragged = L % fc.AK != 0
        got = fc.attention_model_f32(con["qkv"], B, L, heads, mutate="mask_gt")
        assert torch.equal(got, con["expect"]) == (not ragged), L
        if L >= 7:
            assert not torch.equal(fc.attention_model_f32(sel["qkv"], B, L, heads, mutate="natural_v_rows"), sel["expect"]), L
        for c in (sel, con):
            got = fc.attention_model_f32(c["qkv"], B, L, heads, mutate="no_zero_fill")
            assert torch.equal(got, c["expect"]) == (not ragged), L


def test_score_register_map_pairs_keys_four_apart():
    """the C/D map of a 32 x 32 MFMA: register e of lane half hi is key 8 (e >> 2) + 4 hi + (e & 3), so the k-step of register e
    multiplies keys k and k + 4; every key of a block appears exactly once, and the natural-order mutation is a real permutation"""
    keys = sorted(8 * (e >> 2) + 4 * hi + (e & 3) for e in range(16) for hi in (0, 1))
    assert keys == list(range(32))
    assert sorted(fc._KEY_OF_ROW.tolist()) == list(range(fc.AK)) and fc._KEY_OF_ROW.tolist() != list(range(fc.AK))


@pytest.mark.parametrize("family", fc.ATT_BOUNDED_FAMILIES)
@pytest.mark.parametrize("L", fc.ATT_BOUNDED_L)
def test_attention_figure_is_the_models(family, L):
    c = fc.bounded_case(family, L)
    assert c["qkv"].dtype == torch.float32 and not torch.equal(c["qkv"].bfloat16().float(), c["qkv"])      # not bf16-exact
    e = fc.attention_err(fc.attention_model_f32(c["qkv"], c["B"], L, c["heads"]), c["qkv"], c["B"], L, c["heads"])
    assert _holds(e, fc.ATT_FIGURES[family, L]), (e, fc.ATT_FIGURES[family, L])
    assert fc.ATT_BOUNDS[family, L] == 4.0 * fc.ATT_FIGURES[family, L]


@pytest.mark.parametrize("C,layout,route", fc.LN_CASES)
def test_layernorm_case_takes_its_route_and_the_model_is_inside_the_bound(C, layout, route):
    for rows in fc.LN_ROWS:
        for family in fc.LN_FAMILIES:
            x, g, b = fc.layernorm_inputs(C, rows, family)
            xv, gv, bv, yv, ybuf = fc.place_layernorm(x, g, b, layout)
            assert torch.equal(xv, x) and bool((ybuf == fc.SENTINEL).all())
            assert fc.route_of(xv, gv, bv, yv) == ("vec" if rows == 1 and "stride" in layout else route)
            e = fc.layernorm_err(fc.layer_norm_model_f32(x, g, b, route=route), x, g, b)
            assert e <= fc.LN_BOUNDS[family], (family, rows, e)


@pytest.mark.parametrize("family", fc.LN_FAMILIES)
def test_layernorm_figure_is_torch_fp32s(family):
    worst = 0.0
    for C, layout, route in fc.LN_CASES:
        for rows in fc.LN_ROWS:
            x, g, b = fc.layernorm_inputs(C, rows, family)
            worst = max(worst, fc.layernorm_err(fc.layernorm_torch_f32(x, g, b), x, g, b))
    assert _holds(worst, fc.LN_FIGURES[family]), (worst, fc.LN_FIGURES[family])
    assert fc.LN_BOUNDS[family] == 4.0 * fc.LN_FIGURES[family]


@pytest.mark.parametrize("family", ("large_mean", "large_mean_sparse"))
def test_a_one_pass_variance_is_outside_the_bound(family):
    for C, route in ((768, "vec"), (2047, "scalar")):
        x, g, b = fc.layernorm_inputs(C, 77, family)
        e = fc.layernorm_err(fc.layer_norm_model_f32(x, g, b, route=route, one_pass=True), x, g, b)
        assert e > 100.0 * fc.LN_BOUNDS[family], (C, e)
        assert fc.layernorm_err(fc.layer_norm_model_f32(x, g, b, route=route), x, g, b) <= fc.LN_BOUNDS[family]


def test_route_predicate_restates_the_dispatch():
    a = 1 << 20
    assert fc.layernorm_route(768, 768, 768, a, a, a, a) == "vec"
    assert fc.layernorm_route(4, 8, 12, a, a + 16, a, a) == "vec"
    for bad in ((770, 772, 772, a, a, a, a), (768, 769, 768, a, a, a, a), (768, 768, 770, a, a, a, a), (768, 768, 768, a + 4, a, a, a),
                (768, 768, 768, a, a + 8, a, a), (768, 768, 768, a, a, a + 4, a), (768, 768, 768, a, a, a, a + 12)):
        assert fc.layernorm_route(*bad) == "scalar", bad


def test_gelu_figure_is_the_k_ordered_chains():
    worst = 0.0
    for rows, Cin, Cout in fc.linear_shapes():
        c = fc.linear_gelu_case(rows, Cin, Cout)
        for with_br in (False, True):
            worst = max(worst, fc.linear_gelu_err(fc.linear_chain_f32(c, with_br), c, with_br))
    assert _holds(worst, fc.GELU_FIGURE), (worst, fc.GELU_FIGURE)
    assert fc.GELU_BOUND == 4.0 * fc.GELU_FIGURE


@pytest.mark.parametrize("rows,Cin,Cout", [(1, 16, 11), (129, 24, 40), (300, 768, 96)])
def test_integer_gemm_cases_are_exact_in_fp32(rows, Cin, Cout):
    c = fc.linear_int_case(rows, Cin, Cout)
    x, w = c["x"].long(), c["w"].long()
    assert torch.equal((x @ w.T).float(), c["y"]) and torch.equal((x @ w.T + c["b"].long() + c["r"].long()).float(), c["y_br"])
    assert int((x.abs() @ w.abs().T).max()) + 100 < (1 << 24)                # every partial sum in any order is an exact fp32 integer
    assert torch.equal(c["x"] @ c["w"].T, c["y"])


def test_tower_bounds_are_four_times_the_figures():
    assert fc.TOWER_LOGIT_BOUNDS == tuple(4.0 * f for f in fc.TOWER_LOGIT_FIGURES)
    assert fc.TOWER_VMAP_BOUNDS == tuple(4.0 * f for f in fc.TOWER_VMAP_FIGURES)
    assert max(fc.TOWER_LOGIT_BOUNDS) == pytest.approx(3.4e-6, rel=0.01)
    assert math.isclose(fc.TOWER_MARGIN, 1e-4) and fc.TOWER_LEFT_OUT_CAP == 0.01


@pytest.mark.parametrize("case", range(len(fc.TOWER_CASES)))
def test_tower_figures_are_torch_fp32s(case):
    """torch fp32 of the restatement against its float64 copy: the figures, the argmax at the margin, the pixels left out"""
    o, img, ref, v64 = fc.tower_reference(case)
    with torch.no_grad():
        out = o(img)
        _, v = o.encoder(img)
    assert _holds(fc.rel_max(out, ref), fc.TOWER_LOGIT_FIGURES[case]) and _holds(fc.rel_max(v, v64), fc.TOWER_VMAP_FIGURES[case])
    bad, left = fc.argmax_check(out, ref)
    assert bad == 0 and left <= fc.TOWER_LEFT_OUT_CAP
