"""Exact-arithmetic GPU parity of every convolution dispatch route (rows of tests/conv_route_cases.py).

Operands make the fp32 accumulation order irrelevant: activations are integers in [-2, 2] at density d = min(0.5, 750 / K),
weights integers in {-1, 0, 1}, bias and residual integers in [-2, 2].  Every product and partial sum is an integer far below
2^24, so MFMA order, split-K slices, ring depth and tile shape cannot change a bit.  The reference is F.conv2d in float64 on
the CPU (+ bias, + residual, ReLU) from the same tensors, and the tolerance is ZERO: torch.equal on the fp32 output and on the
bf16 output.  For the bf16 comparison the reference must itself be bf16-representable (integers of magnitude <= 256, then no
rounding happens anywhere); that, and a floor of 0.5 on the non-zero share of the pre-activation reference (a ReLU alone zeroes
half of a symmetric result), are asserted on the reference before the kernel result is looked at, never skipped or masked.

Each call first asserts its route with hip.conv2d_route on the real tensors.  The ConvLSTM gate epilogue and GELU are not exact
functions: their routes are pinned in tests/test_conv_routes.py, parity stays with their own tests in test_hip_conv.py."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_route_cases as rc

pytestmark = pytest.mark.gpu

ROUTES = rc.header_routes()


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _operands(geom, seed):
    B, H, W, Cin, Cout, R, stride, pad, dil = geom
    g = torch.Generator().manual_seed(seed)
    d = min(0.5, 750.0 / (R * R * Cin))
    x = _ints(g, (B, H, W, Cin), -2, 2) * (torch.rand((B, H, W, Cin), generator=g) < d)
    w = _ints(g, (Cout, Cin, R, R), -1, 1)
    conv = F.conv2d(x.permute(0, 3, 1, 2), w, stride=stride, padding=pad, dilation=dil).permute(0, 2, 3, 1).contiguous()
    bias = _ints(g, (Cout,), -2, 2)
    res = _ints(g, tuple(conv.shape), -2, 2)
    return x, w, conv, bias, res


def _check_reference(ref_pre, ref, what):
    """conditions on the inputs, asserted on the reference alone"""
    assert torch.equal(ref.float().bfloat16().double(), ref), f"{what}: reference is not bf16-representable (max |ref| {float(ref.abs().max())})"
    share = float((ref_pre != 0).double().mean())
    assert share >= 0.5, f"{what}: only {share:.3f} of the reference is non-zero"
    # what is compared: a ReLU zeroes the negative half of a symmetric result (P(ref > 0) = (1 - P(0)) / 2 >= 0.25 from the
    # floor above, less sampling noise), so the compared reference must keep a quarter non-zero
    shared = float((ref != 0).double().mean())
    assert shared >= (0.5 if ref is ref_pre else 0.25), f"{what}: only {shared:.3f} of the compared reference is non-zero"


def _ref_stats(conv, rows):
    M, C = conv.shape[0] * conv.shape[1] * conv.shape[2], conv.shape[3]
    tiles = (M + rows - 1) // rows
    flat = torch.zeros(tiles * rows, C, dtype=torch.float64)
    flat[:M] = conv.reshape(M, C)
    flat = flat.reshape(tiles, rows, C)
    return flat.sum(1), (flat * flat).sum(1)


@pytest.mark.parametrize("name,geom,routes,_why", rc.ROUTE_CASES, ids=[r[0] for r in rc.ROUTE_CASES])
def test_conv_route_is_exact(name, geom, routes, _why):
    from openess_amd import hip
    B, H, W, Cin, Cout, R, stride, pad, dil = geom
    x, w, conv, bias, res = _operands(geom, 1000 + sum(geom))
    Ho, Wo = conv.shape[1], conv.shape[2]
    M = B * Ho * Wo
    packed = hip.pack_conv_weight(w.cuda())
    bias_d = bias.float().cuda()
    for variant, want in routes.items():
        a = rc.VARIANTS[variant]
        what = f"{name}/{variant}"
        ref_pre = conv + (bias if a.get("bias") else 0) + (res if a.get("residual") else 0)
        ref = ref_pre.clamp_min(0) if a.get("relu") else ref_pre
        _check_reference(ref_pre, ref, what)
        ps_in, ps_out, ps_res = rc.strides(geom, variant)
        # operands as the variant's views; neighbours of a slice hold values that would show up in the result if read
        xin = x.bfloat16().cuda()
        if "in_extra" in a:
            wide = torch.full((B, H, W, ps_in), 7.0, dtype=torch.bfloat16, device="cuda")
            wide[..., 8:8 + Cin] = xin
            xin = wide[..., 8:8 + Cin]
        out, obuf = None, None
        if "out_extra" in a:
            obuf = torch.full((B, Ho, Wo, ps_out), -3.0, dtype=torch.bfloat16, device="cuda")
            out = obuf[..., 8:8 + Cout]
        rv = None
        if a.get("residual"):
            rwide = torch.full((B, Ho, Wo, ps_res), 5.0, dtype=torch.bfloat16, device="cuda")
            rwide[..., :Cout] = res.bfloat16().cuda()
            rv = rwide[..., :Cout]
        part = torch.full(((M + 127) // 128, 2, Cout), float("nan"), device="cuda") if a.get("tile_stats") else None
        kw = dict(relu=bool(a.get("relu")), residual=rv, out=out, out_f32=bool(a.get("out_f32")), tile_stats=part)
        b_ = bias_d if a.get("bias") else None
        got = hip.conv2d_route(xin, packed, b_, Cout, R, R, stride, pad, dil, **kw)
        assert got == rc.route_value(ROUTES, want), f"{what}: meant for {want}, dispatch says {hip.conv2d_route_name(got)} ({got})"
        y = hip.conv2d_nhwc(xin, packed, b_, Cout, R, R, stride, pad, dil, **kw)
        torch.cuda.synchronize()
        assert tuple(y.shape) == tuple(ref.shape), what
        if a.get("out_f32"):
            assert y.dtype == torch.float32 and torch.equal(y.cpu(), ref.float()), \
                f"{what}: {int((y.cpu() != ref.float()).sum())} of {ref.numel()} fp32 outputs differ"
        else:
            assert y.dtype == torch.bfloat16 and torch.equal(y.cpu(), ref.float().bfloat16()), \
                f"{what}: {int((y.cpu() != ref.float().bfloat16()).sum())} of {ref.numel()} bf16 outputs differ"
        if obuf is not None:
            assert bool((obuf[..., :8] == -3.0).all()) and bool((obuf[..., 8 + Cout:] == -3.0).all()), f"{what}: neighbours of the output slice were written"
        if part is not None:
            # per-128-row column sums and sums of squares, exact (sums <= 128 x 256, squares <= 2^23).  The 256 x 256-tile kernel
            # documents another layout (include/oess.h): row 2t = the sums of its 256 rows, row 2t + 1 = 0
            p = part.double().cpu()
            assert bool(torch.isfinite(p).all()), f"{what}: statistics rows left unwritten"
            s1, s2 = _ref_stats(conv, 128)
            if want == "TILE256":
                z = torch.zeros(1, Cout, dtype=torch.float64)
                for s_ in (s1, s2):
                    even = s_[0::2] + torch.cat([s_[1::2], z])[:s_[0::2].shape[0]]
                    s_[0::2], s_[1::2] = even, 0.0
            assert torch.equal(p[:, 0], s1), f"{what}: tile column sums differ"
            assert torch.equal(p[:, 1], s2), f"{what}: tile column sums of squares differ"


def test_conv_dgrad_operator_is_exact():
    """pack_conv_weight(flip=1): dX = conv(dY, flipped operator) against torch.autograd.grad of the float64 convolution, with
    the same integer operands (K = 9 x 72 of the gradient's reduction), fp32 and bf16 outputs both exact."""
    from openess_amd import hip
    B, H, W, Cin, Cout, R, pad, dil = 2, 9, 10, 64, 72, 3, 2, 2
    g = torch.Generator().manual_seed(77)
    xz = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
    w = _ints(g, (Cout, Cin, R, R), -1, 1)
    y = F.conv2d(xz, w, padding=pad, dilation=dil)
    gy = _ints(g, tuple(y.shape), -2, 2) * (torch.rand(tuple(y.shape), generator=g) < 0.5)
    ref = torch.autograd.grad(y, xz, gy)[0].permute(0, 2, 3, 1).contiguous()
    _check_reference(ref, ref, "dgrad")
    gy_nhwc = gy.permute(0, 2, 3, 1).contiguous().bfloat16().cuda()
    packed = hip.pack_conv_weight(w.cuda(), flip=True)
    args = (gy_nhwc, packed, None, Cin, R, R, 1, dil * (R - 1) - pad, dil)
    assert hip.conv2d_route(*args, out_f32=True) == hip.conv2d_route(*args) == ROUTES["DMA64_SLOWK"]
    assert torch.equal(hip.conv2d_nhwc(*args, out_f32=True).cpu(), ref.float())
    assert torch.equal(hip.conv2d_nhwc(*args).cpu(), ref.float().bfloat16())
