"""GPU tests of the fp32 ViT token kernels (openess_amd/csrc/vit_f32.hip, oess_linear_tokens_f32 of conv_f32.hip) on the cases of
tests/vit_f32_cases.py:

  * attention, exact: the selection and the constant-V cases in fp32 must come out bit for bit (tests/test_vit_f32_cases.py
    proves on the CPU that a correct implementation does), with the qkv rows followed by NaN rows, at every L of ATT_L x ATT_BH,
    at the full token count, and with a row-strided qkv and an out that is a column slice of a sentinel-filled buffer;
  * attention, bounded: fp32 operands that are not bf16-exact against float64, per family; two runs give equal bits;
  * LayerNorm on both routes (asserted per case from the actual strides and addresses), every family, strided views with NaN gaps
    and sentinel-filled outputs, against float64 per family;
  * the token GEMM: small-integer operands equal an int64 reference and hip.conv2d_f32 at 1 x 1 bit for bit, with and without
    bias and residual, dense and row-strided; the GELU epilogue against a float64 erf GELU.

Every bound is four times what fp32 on the CPU gives against float64 (tools/exp_maskclip_fp32_bounds.py); nothing the kernels
produce went into one."""
import math

import pytest
import torch

from tests import vit_f32_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXACT = [(f, B, L, h) for f in ("selection", "constant_v") for (B, L, h) in fc.exact_shapes()]


def _exact(family, B, L, heads, extra_cols=0, out_cols=0):
    from openess_amd import hip
    c = fc.exact_case(family, B, L, heads)
    C = heads * 64
    buf, qkv = fc.embed(c["qkv"], fc.NAN_TAIL_ROWS, extra_cols, math.nan, DEV)
    assert qkv.data_ptr() % 16 == 0 and (B * L == 1 or qkv.stride(0) == 3 * C + extra_cols)
    obuf = torch.full((B * L, C + out_cols), fc.SENTINEL, dtype=torch.float32, device=DEV)
    o = hip.attention_d64_f32(qkv, B, L, heads, out=obuf[:, :C])
    assert o.data_ptr() == obuf.data_ptr() and o.dtype == torch.float32
    got = o.cpu()
    assert not bool(torch.isnan(got).any()), "NaN: a masked key's V row or a row past B L reached the output"
    wrong = (got != c["expect"]).any(dim=1).nonzero().flatten().tolist()
    assert torch.equal(got, c["expect"]), f"{family} B={B} L={L} heads={heads}: {len(wrong)} rows differ, first {wrong[:8]}"
    assert bool((obuf[:, C:] == fc.SENTINEL).all())
    assert bool(torch.isnan(buf[B * L:]).all()) and bool(torch.isnan(buf[:, 3 * C:]).all())     # the input is not written either


@pytest.mark.parametrize("family,B,L,heads", EXACT)
def test_attention_exact(family, B, L, heads):
    _exact(family, B, L, heads)


@pytest.mark.parametrize("family", ("selection", "constant_v"))
@pytest.mark.parametrize("L", fc.ATT_STRIDE_L)
def test_attention_exact_with_row_strides(family, L):
    B, heads = fc.ATT_STRIDE_BH
    _exact(family, B, L, heads, extra_cols=fc.ATT_STRIDE_EXTRA, out_cols=fc.ATT_OUT_COLS)


@pytest.mark.parametrize("family", fc.ATT_BOUNDED_FAMILIES)
@pytest.mark.parametrize("L", fc.ATT_BOUNDED_L)
def test_attention_within_the_float64_bound(family, L):
    from openess_amd import hip
    c = fc.bounded_case(family, L)
    qkv = c["qkv"].to(DEV)
    o = hip.attention_d64_f32(qkv, c["B"], L, c["heads"])
    err = fc.attention_err(o, c["qkv"], c["B"], L, c["heads"])
    print(f"attention f32 {family} L={L}: err {err:.3e} (figure {fc.ATT_FIGURES[family, L]:.3e}, bound {fc.ATT_BOUNDS[family, L]:.3e})")
    assert err <= fc.ATT_BOUNDS[family, L]
    assert torch.equal(hip.attention_d64_f32(qkv, c["B"], L, c["heads"]), o), "two runs differ"


@pytest.mark.parametrize("family", fc.LN_FAMILIES)
@pytest.mark.parametrize("C,layout,route", fc.LN_CASES)
def test_layernorm_within_the_float64_bound(C, layout, route, family):
    from openess_amd import hip
    for rows in fc.LN_ROWS:
        x, g, b = fc.layernorm_inputs(C, rows, family)
        xv, gv, bv, yv, ybuf = fc.place_layernorm(x, g, b, layout, DEV)
        # a single row has no stride to be off: the two padded-stride layouts that force the 4-byte route need rows > 1
        assert fc.route_of(xv, gv, bv, yv) == ("vec" if rows == 1 and "stride" in layout else route)
        y = hip.layer_norm_tokens_f32(xv, gv, bv, fc.LN_EPS, out=yv)
        assert y.data_ptr() == ybuf.data_ptr()
        err = fc.layernorm_err(y, x, g, b)
        print(f"layernorm f32 C={C} {layout} rows={rows} {family}: err {err:.3e} (figure {fc.LN_FIGURES[family]:.3e}, "
              f"bound {fc.LN_BOUNDS[family]:.3e})")
        assert err <= fc.LN_BOUNDS[family]
        assert bool((ybuf[:, C:] == fc.SENTINEL).all())
        again = torch.as_strided(torch.full_like(ybuf, fc.SENTINEL), tuple(yv.shape), yv.stride())     # same layout: same route
        assert torch.equal(hip.layer_norm_tokens_f32(xv, gv, bv, fc.LN_EPS, out=again), y), "two runs differ"


def _strided(t, extra, fill):
    """t as the leading columns of a wider buffer filled with `fill`: (buffer, view with t's shape and row stride width + extra)"""
    buf = torch.full((t.shape[0], t.shape[1] + extra), fill, dtype=torch.float32, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf, torch.as_strided(buf, tuple(t.shape), (t.shape[1] + extra, 1))


def _as_map(t):
    """[rows, C] token view -> the logical [1, C, 1, rows] map hip.conv2d_f32 takes, same memory"""
    return torch.as_strided(t, (1, t.shape[1], 1, t.shape[0]), (0, 1, 0, t.stride(0) if t.shape[0] > 1 else t.shape[1]), t.storage_offset())


@pytest.mark.parametrize("rows,Cin,Cout", fc.linear_shapes())
def test_linear_tokens_integers_are_exact_and_equal_the_1x1_conv(rows, Cin, Cout):
    from openess_amd import hip
    c = fc.linear_int_case(rows, Cin, Cout)
    packed = hip.pack_conv_weight_f32(c["w"][:, :, None, None].to(DEV))
    b = c["b"].to(DEV)
    # dense, no bias, no residual
    x = c["x"].to(DEV)
    y = hip.linear_tokens_f32(x, packed, None, Cout)
    assert y.dtype == torch.float32 and y.shape == (rows, Cout)
    assert torch.equal(y.cpu(), c["y"])
    ref = hip.conv2d_f32(_as_map(x), packed, None, Cout, 1, 1)
    assert torch.equal(ref.permute(0, 2, 3, 1).reshape(rows, Cout), y)
    # bias and residual; x, residual and out row-strided (an x stride that is no multiple of 4 floats: the 4-byte operand route)
    for ex in (4, 3):
        xbuf, xv = _strided(c["x"], ex, math.nan)
        rbuf, rv = _strided(c["r"], 5, math.nan)
        obuf = torch.full((rows, Cout + 7), fc.SENTINEL, dtype=torch.float32, device=DEV)
        ov = torch.as_strided(obuf, (rows, Cout), (Cout + 7, 1))
        y = hip.linear_tokens_f32(xv, packed, b, Cout, residual=rv, out=ov)
        assert y.data_ptr() == obuf.data_ptr()
        assert torch.equal(y.cpu(), c["y_br"])
        assert bool((obuf[:, Cout:] == fc.SENTINEL).all())
        ref = torch.empty((1, rows, 1, Cout), dtype=torch.float32, device=DEV).permute(0, 3, 2, 1)          # [1, Cout, 1, rows]
        hip.conv2d_f32(_as_map(xv), packed, b, Cout, 1, 1, residual=_as_map(rv), out=ref)
        assert torch.equal(ref.permute(0, 3, 2, 1).reshape(rows, Cout), y)


@pytest.mark.parametrize("rows,Cin,Cout", fc.linear_shapes())
def test_linear_tokens_gelu_within_the_float64_bound(rows, Cin, Cout):
    from openess_amd import hip
    c = fc.linear_gelu_case(rows, Cin, Cout)
    packed = hip.pack_conv_weight_f32(c["w"][:, :, None, None].to(DEV))
    x = c["x"].to(DEV)
    for with_br in (False, True):
        y = hip.linear_tokens_f32(x, packed, c["b"].to(DEV) if with_br else None, Cout, act='gelu',
                                  residual=c["r"].to(DEV) if with_br else None)
        err = fc.linear_gelu_err(y, c, with_br)
        print(f"gelu gemm rows={rows} Cin={Cin} Cout={Cout} bias+residual={with_br}: err {err:.3e} (figure {fc.GELU_FIGURE:.3e}, "
              f"bound {fc.GELU_BOUND:.3e})")
        assert err <= fc.GELU_BOUND
