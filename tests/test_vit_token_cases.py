"""CPU half of the ViT token kernels' tests (tests/vit_token_cases.py holds the cases, tests/test_hip_vit_tokens.py runs them on
the GPU): the fp32 model of the attention kernel reproduces every exact expectation bit for bit (a correct implementation
passes), each of three one-line mutations of the kernel is caught by an exact case while the old randn comparison lets the mask
mutation through, the bounds are four times the models' figures against float64, every LayerNorm case takes the route it names,
and the two C entries and their wrappers refuse bad arguments before anything is launched.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import vit_token_cases as vc

EINVAL = -22
EXACT = [(f, B, L, h) for f in vc.EXACT_CASES for (B, L, h) in vc.exact_shapes()]


@pytest.mark.parametrize("family,B,L,heads", EXACT)
def test_model_reproduces_the_exact_expectation(family, B, L, heads):
    c = vc.EXACT_CASES[family](B, L, heads)
    assert c["qkv"].dtype == c["expect"].dtype == torch.bfloat16
    assert c["qkv"].shape == (B * L, 3 * heads * 64) and c["expect"].shape == (B * L, heads * 64)
    if family == "selection" and L > 1:
        assert c["gap"] >= vc.MIN_GAP                       # from the builder's int64 dot products
    assert bool((c["qkv"][:, 2 * heads * 64:] != 0).all())  # V is never zero: an output of 0 is always an error
    assert torch.equal(vc.attention_model(c["qkv"], B, L, heads), c["expect"])
    # float64 agrees to far below one bf16 step: the expectation is the operation's result, not the model's habit
    assert float((vc.attention64(c["qkv"], B, L, heads) - c["expect"].double()).abs().max()) < 1e-9


@pytest.mark.parametrize("B,heads", vc.ATT_BH)
def test_each_kernel_mutation_breaks_an_exact_case(B, heads):
    """mask `key > L`: the zero pad row at key L scores 0 against <= -64 and takes the softmax of the constant-V case (any L that
    is no multiple of 64; the selection case, whose winner scores +256, cannot see it).  Unpermuted K rows: the weight lands on
    the V row with key bits 2 and 3 swapped (selection, any L > 4).  V rows of masked keys left unfilled: 0 * NaN (both cases,
    any L that is no multiple of 64)."""
    for L in vc.ATT_L:
        sel, con = vc.selection_case(B, L, heads), vc.constant_v_case(B, L, heads)

        def broken(c, mutate):
            return not torch.equal(vc.attention_model(c["qkv"], B, L, heads, mutate=mutate), c["expect"])

        ragged = L % vc.AK != 0
        assert broken(con, "mask_gt") == ragged, L
        if ragged:
            o = vc.attention_model(con["qkv"], B, L, heads, mutate="mask_gt")
            assert float(o.float().abs().max()) < 1e-20     # w e^-64 at the most against |w| >= 0.5: total, not 0.1 %
        assert not broken(sel, "mask_gt")
        assert broken(sel, "identity_perm") == (L > 4), L
        assert broken(sel, "no_v_zero") == ragged and broken(con, "no_v_zero") == ragged, L


def test_the_randn_comparison_lets_the_mask_mutation_through():
    """what tests/test_hip_maskclip.py::test_layernorm_and_attention_kernels asserts (randn 1.5, rtol = atol = 2e-2 against
    fp32 torch) holds for the model with the off-by-one mask at every L of that test: the gap this module closes"""
    torch.manual_seed(1)
    heads = 12
    C = heads * 64
    for B, L in ((2, 77), (1, 32), (3, 130)):
        qkv = (torch.randn(B * L, 3 * C) * 1.5).bfloat16()
        ref = vc.attention64(qkv, B, L, heads).float().numpy()
        o = vc.attention_model(qkv, B, L, heads, mutate="mask_gt")
        np.testing.assert_allclose(o.float().numpy(), ref, rtol=2e-2, atol=2e-2)


def test_a_leaked_next_batch_key_takes_the_constant_v_softmax():
    """the keys of batch b + 1 appended to batch b's: the output turns into w_{b+1}"""
    B, L, heads = 2, 9, 2
    c = vc.constant_v_case(B, L, heads)
    leak = torch.cat([c["qkv"][:L], c["qkv"][L:L + 1]])     # batch 0 plus the first key of batch 1
    o = vc.attention_model(leak, 1, L + 1, heads)[:L]
    assert torch.equal(o, c["expect"][L:2 * L]) and not torch.equal(o, c["expect"][:L])


def test_attention_bound_is_four_times_the_models_figure():
    worst = 0.0
    for family in vc.ATT_BOUNDED_FAMILIES:
        for L in vc.ATT_BOUNDED_L:
            c = vc.bounded_case(family, L)
            assert c["qkv"].shape == (c["B"] * c["L"], 3 * c["heads"] * 64) and c["L"] == L
            worst = max(worst, vc.attention_err(vc.attention_model(c["qkv"], c["B"], L, c["heads"]), c["qkv"], c["B"], L, c["heads"]))
    assert 0.8 * vc.ATT_MODEL_FIGURE <= worst <= 1.05 * vc.ATT_MODEL_FIGURE, worst
    assert vc.ATT_BOUND == 4.0 * vc.ATT_MODEL_FIGURE
    # the measure sees what the exact cases see: the mutations sit far outside the bound on a random case
    c = vc.bounded_case("randn4", 65)
    for mutate in ("identity_perm", "no_v_zero"):
        e = vc.attention_err(vc.attention_model(c["qkv"], c["B"], 65, c["heads"], mutate=mutate), c["qkv"], c["B"], 65, c["heads"])
        assert not e <= vc.ATT_BOUND, (mutate, e)


def test_ordered_cases_rescale_in_every_tile_or_in_none():
    """restated from the model's own recurrence: the running maximum of every query moves in each tile of the ascending case and
    in none after the first of the descending one"""
    for family, moves in (("ascending", True), ("descending", False)):
        c = vc.bounded_case(family, 257)
        q, k, _ = vc.split_heads(c["qkv"].float(), c["B"], 257, c["heads"])
        s = q @ k.transpose(-1, -2)
        m = s[..., :vc.AK].max(dim=-1).values
        for k0 in range(vc.AK, 257, vc.AK):
            t = s[..., k0:k0 + vc.AK].max(dim=-1).values
            assert bool((t > m).all()) if moves else bool((t < m).all())
            m = torch.maximum(m, t)


def _layernorm_case_on_the_cpu(C, layout, route, rows_list, families):
    worst = 0.0
    for rows in rows_list:
        for family in families:
            x, g, b = vc.layernorm_inputs(C, rows, family)
            assert x.dtype == torch.bfloat16 and x.shape == (rows, C) and g.dtype == b.dtype == torch.float32
            xv, gv, bv, yv, ybuf = vc.place_layernorm(x, g, b, layout)
            assert vc.route_of(xv, gv, bv, yv) == route
            assert torch.equal(xv, x) and torch.equal(gv, g) and torch.equal(bv, b) and yv.shape == x.shape
            assert bool((ybuf == vc.SENTINEL).all())
            if xv.stride(0) > C:
                assert bool(torch.isnan(xv.as_strided((rows, xv.stride(0) - C), (xv.stride(0), 1), xv.storage_offset() + C)).all())
            worst = max(worst, vc.layernorm_err(vc.layer_norm_model(x, g, b, vc.LN_EPS, route), x, g, b))
    assert worst <= 1.05 * vc.LN_MODEL_FIGURE, worst
    return worst


@pytest.mark.parametrize("C,layout,route", vc.LN_CASES)
def test_layernorm_case_takes_its_route_and_the_model_holds_the_figure(C, layout, route):
    _layernorm_case_on_the_cpu(C, layout, route, vc.LN_ROWS, vc.LN_FAMILIES)


def test_layernorm_bound_is_four_times_the_models_figure():
    """the largest figure comes from the grid-stride cases (most elements); the rest is held under it case by case above"""
    worst = max(_layernorm_case_on_the_cpu(C, layout, route, (vc.LN_GRID_ROWS,), ("randn",)) for C, layout, route in vc.LN_GRID_CASES)
    assert worst >= 0.8 * vc.LN_MODEL_FIGURE, worst
    assert vc.LN_BOUND == 4.0 * vc.LN_MODEL_FIGURE and vc.LN_GRID_ROWS > 4 * 65536


def test_route_predicate_restates_the_dispatch():
    a = 1 << 20
    assert vc.layernorm_route(768, 768, 768, a, a, a, a) == "vec"
    assert vc.layernorm_route(8, 8, 16, a, a + 16, a, a) == "vec"
    for C, xs, ys, ptrs in ((772, 772, 772, (a, a, a, a)), (768, 772, 768, (a, a, a, a)), (768, 768, 772, (a, a, a, a)),
                            (768, 768, 768, (a + 8, a, a, a)), (768, 768, 768, (a, a + 2, a, a)), (768, 768, 768, (a, a, a + 4, a)),
                            (768, 768, 768, (a, a, a, a + 4)), (1, 1, 1, (a, a, a, a))):
        assert vc.layernorm_route(C, xs, ys, *ptrs) == "scalar"


def test_layernorm_measure_sees_a_one_pass_variance():
    """E[x^2] - mean^2 from the same fp32 lane sums.  On the large-mean family (mean 100, spread 0.25) it reaches 4.3 at C = 768,
    77 rows: outside what correct arithmetic gives (1.6) but inside the x4 bound, so that family alone would let it through; on
    the sparse one (sigma ~ 0.125) it is at 14, outside the bound on both routes.  The two-pass model stays at its figure."""
    for route in ("vec", "scalar"):
        x, g, b = vc.layernorm_inputs(768, 77, "large_mean_sparse")
        assert not vc.layernorm_err(vc.layer_norm_model(x, g, b, vc.LN_EPS, route, one_pass=True), x, g, b) <= vc.LN_BOUND
        assert vc.layernorm_err(vc.layer_norm_model(x, g, b, vc.LN_EPS, route), x, g, b) <= vc.LN_MODEL_FIGURE
        x, g, b = vc.layernorm_inputs(768, 77, "large_mean")
        one, two = (vc.layernorm_err(vc.layer_norm_model(x, g, b, vc.LN_EPS, route, one_pass=p), x, g, b) for p in (True, False))
        assert one > 2.0 * two and two <= vc.LN_MODEL_FIGURE
    # a constant row gives beta (rounded), whatever eps
    x, g, b = vc.layernorm_inputs(64, 5, "constant")
    assert torch.equal(vc.layer_norm_model(x, g, b, vc.LN_EPS, "vec"), b.bfloat16().expand(5, 64))


def test_strided_attention_operands():
    c = vc.selection_case(2, 33, 2)
    buf, view = vc.embed(c["qkv"], vc.NAN_TAIL_ROWS, 8, math.nan)
    assert view.stride(0) == 3 * 128 + 8 and view.stride(0) % 8 == 0 and view.data_ptr() % 16 == 0 and torch.equal(view, c["qkv"])
    assert bool(torch.isnan(buf[66:]).all()) and bool(torch.isnan(buf[:, 3 * 128:]).all())


# --------------------------------------------------------------------------------------------- argument contract, no launch
def _aligned():
    buf = ctypes.create_string_buffer(1 << 16)
    addr = ctypes.addressof(buf)
    return buf, addr + (-addr) % 16


def test_layernorm_entry_validates_arguments_before_any_launch():
    from openess_amd import _lib
    ln = _lib.load().oess_layernorm_bf16
    buf, a = _aligned()

    def call(x=a, xs=768, rows=4, C=768, gamma=a, beta=a, eps=1e-6, y=a, ys=768):
        return ln(x, xs, rows, C, gamma, beta, eps, y, ys, None)

    for bad in (dict(C=0, xs=8, ys=8), dict(C=-8), dict(C=2049, xs=2056, ys=2056), dict(eps=0.0), dict(eps=-1e-6), dict(xs=767),
                dict(ys=767), dict(xs=0), dict(rows=0), dict(rows=-1), dict(x=None), dict(y=None), dict(gamma=None),
                dict(beta=None)):
        assert call(**bad) == EINVAL, bad
    del buf


def test_attention_entry_validates_arguments_before_any_launch():
    from openess_amd import _lib
    att = _lib.load().oess_attention_d64_bf16
    buf, a = _aligned()

    def call(qkv=a, qs=3 * 128, B=2, L=9, heads=2, out=a, os_=128):
        return att(qkv, qs, B, L, heads, 0.125, out, os_, None)

    for bad in (dict(L=0), dict(L=-1), dict(heads=0), dict(B=0), dict(qs=3 * 128 - 8), dict(qs=3 * 128 + 4), dict(qs=3 * 128 + 1),
                dict(os_=120), dict(os_=132), dict(qkv=a + 8), dict(qkv=a + 2), dict(out=a + 8), dict(qkv=None), dict(out=None)):
        assert call(**bad) == EINVAL, bad
    del buf


def test_wrappers_refuse_a_bad_out_or_affine_before_anything_runs():
    """every refusal is a ValueError raised before the device check, so CPU tensors reach it; a fully valid CPU call then stops at
    the device check (no CPU fallback)"""
    from openess_amd import hip
    rows, C = 5, 64
    x = torch.zeros(rows, C, dtype=torch.bfloat16)
    g, b = torch.ones(C), torch.zeros(C)
    out = torch.empty(rows, C, dtype=torch.bfloat16)
    wide = torch.empty(rows, 2 * C, dtype=torch.bfloat16)
    bad_outs = (out.float(), out.to("meta"), torch.empty(rows + 1, C, dtype=torch.bfloat16), torch.empty(rows, C - 8, dtype=torch.bfloat16),
                out[0], wide[:, ::2], torch.empty(C, rows, dtype=torch.bfloat16).T)
    for o in bad_outs:
        with pytest.raises(ValueError, match="out must be bf16"):
            hip.layer_norm_tokens(x, g, b, out=o)
    bad_affine = (g.double(), g.bfloat16(), torch.ones(2 * C)[::2], torch.ones(C + 1), torch.ones(C - 1), torch.ones(1, C), g.to("meta"),
                  None)
    for p in bad_affine:
        with pytest.raises(ValueError, match="gamma must be contiguous fp32"):
            hip.layer_norm_tokens(x, p, b)
        with pytest.raises(ValueError, match="beta must be contiguous fp32"):
            hip.layer_norm_tokens(x, g, p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.layer_norm_tokens(x, g, b, out=wide[:, :C])

    B, L, heads = 1, rows, 1
    qkv = torch.zeros(B * L, 3 * C, dtype=torch.bfloat16)
    for o in bad_outs:
        with pytest.raises(ValueError, match="out must be bf16"):
            hip.attention_d64(qkv, B, L, heads, out=o)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.attention_d64(qkv, B, L, heads, out=wide[:, :C])
