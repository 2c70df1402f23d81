"""GPU tests of the ViT token kernels (openess_amd/csrc/vit_ops.hip) on the cases of tests/vit_token_cases.py:

  * attention, exact: the selection and the constant-V cases must come out bit for bit (tests/test_vit_token_cases.py proves on
    the CPU that a correct implementation does), with the qkv rows followed by NaN rows, at every L of ATT_L x ATT_BH, at the
    full token count, and with a row-strided qkv and an out that is a column slice of a sentinel-filled buffer;
  * attention, bounded: randn 1.5 / randn 4 / ascending / descending keys against float64 within ATT_BOUND;
  * LayerNorm on both routes (asserted per case from the actual strides and addresses), every family, strided views with NaN
    gaps and sentinel-filled outputs, and the two grid-stride cases, against float64 within LN_BOUND.

The bounds are four times what the fp32 CPU models of the kernels give against float64 (tools/exp_vit_token_bounds.py); nothing
the kernels produce went into them."""
import math

import pytest
import torch

from tests import vit_token_cases as vc

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXACT = [(f, B, L, h) for f in vc.EXACT_CASES for (B, L, h) in vc.exact_shapes()]


def _exact(family, B, L, heads, extra_cols=0, out_cols=0):
    from openess_amd import hip
    c = vc.EXACT_CASES[family](B, L, heads)
    C = heads * 64
    buf, qkv = vc.embed(c["qkv"], vc.NAN_TAIL_ROWS, extra_cols, math.nan, DEV)
    assert qkv.stride(0) == 3 * C + extra_cols and qkv.data_ptr() % 16 == 0
    obuf = torch.full((B * L, C + out_cols), vc.SENTINEL, dtype=torch.bfloat16, device=DEV)
    o = hip.attention_d64(qkv, B, L, heads, out=obuf[:, :C])
    assert o.data_ptr() == obuf.data_ptr() and o.stride(0) == C + out_cols
    got = o.cpu()
    assert not bool(torch.isnan(got.float()).any()), "NaN: a masked key's V row or a row past B L reached the output"
    wrong = (got != c["expect"]).any(dim=1).nonzero().flatten().tolist()
    assert torch.equal(got, c["expect"]), f"{family} B={B} L={L} heads={heads}: {len(wrong)} rows differ, first {wrong[:8]}"
    assert bool((obuf[:, C:] == vc.SENTINEL).all())
    assert bool(torch.isnan(buf[B * L:]).all())                            # the input is not written either


@pytest.mark.parametrize("family,B,L,heads", EXACT)
def test_attention_exact(family, B, L, heads):
    _exact(family, B, L, heads)


@pytest.mark.parametrize("family", list(vc.EXACT_CASES))
@pytest.mark.parametrize("L", vc.ATT_STRIDE_L)
def test_attention_exact_with_row_strides(family, L):
    B, heads = vc.ATT_STRIDE_BH
    _exact(family, B, L, heads, extra_cols=8, out_cols=64)


@pytest.mark.parametrize("family", vc.ATT_BOUNDED_FAMILIES)
@pytest.mark.parametrize("L", vc.ATT_BOUNDED_L)
def test_attention_within_the_float64_bound(family, L):
    from openess_amd import hip
    c = vc.bounded_case(family, L)
    o = hip.attention_d64(c["qkv"].to(DEV), c["B"], L, c["heads"])
    err = vc.attention_err(o, c["qkv"], c["B"], L, c["heads"])
    print(f"attention {family} L={L}: err {err:.3e} (model figure {vc.ATT_MODEL_FIGURE:.3e}, bound {vc.ATT_BOUND:.3e})")
    assert err <= vc.ATT_BOUND


def _layernorm(C, layout, route, rows_list, families):
    from openess_amd import hip
    worst = 0.0
    for rows in rows_list:
        for family in families:
            x, g, b = vc.layernorm_inputs(C, rows, family)
            xv, gv, bv, yv, ybuf = vc.place_layernorm(x, g, b, layout, DEV)
            assert vc.route_of(xv, gv, bv, yv) == route
            y = hip.layer_norm_tokens(xv, gv, bv, vc.LN_EPS, out=yv)
            assert y.data_ptr() == ybuf.data_ptr()
            err = vc.layernorm_err(y, x, g, b)
            assert err <= vc.LN_BOUND, f"C={C} {layout} rows={rows} {family}: err {err:.3f} > {vc.LN_BOUND}"
            assert bool((ybuf[:, C:] == vc.SENTINEL).all())
            if family == "constant":                                       # variance 0: beta, whatever eps
                assert torch.equal(y.cpu(), b.bfloat16().expand(rows, C))
            worst = max(worst, err)
    print(f"layernorm C={C} {layout} ({route}): largest err {worst:.3f} (model figure {vc.LN_MODEL_FIGURE}, bound {vc.LN_BOUND})")


@pytest.mark.parametrize("C,layout,route", vc.LN_CASES)
def test_layernorm_within_the_float64_bound(C, layout, route):
    _layernorm(C, layout, route, vc.LN_ROWS, vc.LN_FAMILIES)


@pytest.mark.parametrize("C,layout,route", vc.LN_GRID_CASES)
def test_layernorm_grid_stride_loop(C, layout, route):
    assert vc.LN_GRID_ROWS > 4 * 65536
    _layernorm(C, layout, route, (vc.LN_GRID_ROWS,), ("randn",))


def test_layernorm_without_out_allocates_a_dense_result():
    from openess_amd import hip
    x, g, b = vc.layernorm_inputs(768, 5, "randn")
    y = hip.layer_norm_tokens(x.to(DEV), g.to(DEV), b.to(DEV), vc.LN_EPS)
    assert y.shape == (5, 768) and y.is_contiguous() and y.dtype == torch.bfloat16
    assert vc.layernorm_err(y, x, g, b) <= vc.LN_BOUND


def test_wrappers_refuse_operands_on_another_device():
    from openess_amd import hip
    x, g, b = (t.to(DEV) for t in vc.layernorm_inputs(64, 5, "randn"))
    with pytest.raises(ValueError, match="out must be bf16"):
        hip.layer_norm_tokens(x, g, b, out=torch.empty(5, 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="gamma must be contiguous fp32"):
        hip.layer_norm_tokens(x, g.cpu(), b)
    with pytest.raises(ValueError, match="beta must be contiguous fp32"):
        hip.layer_norm_tokens(x, g, b.cpu())
    with pytest.raises(ValueError, match="out must be bf16"):
        hip.layer_norm_tokens(x, g, b, out=torch.empty(5, 64, dtype=torch.float16, device=DEV))
    qkv = vc.constant_v_case(1, 7, 1)["qkv"].to(DEV)
    with pytest.raises(ValueError, match="out must be bf16"):
        hip.attention_d64(qkv, 1, 7, 1, out=torch.empty(7, 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="out must be bf16"):
        hip.attention_d64(qkv, 1, 7, 1, out=torch.empty(8, 64, dtype=torch.bfloat16, device=DEV))
