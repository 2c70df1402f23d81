"""CPU test of hip.pack_conv_weight_f32_dgrad (K18): the operand with which the fp32 forward kernel computes the data gradient of
a stride-1 convolution.  Unpacked from pack_conv_weight_f32's layout ([ceil16(R S Cout)][ceil32(Cin)], row (r S + s) Cout + co,
column ci) it is W'[ci][co][r][s] = W[co][ci][R - 1 - r][S - 1 - s], and conv(dY, W', pad' = R - 1 - pad) in float64 equals
torch.autograd.grad of F.conv2d.  Needs neither a GPU nor the library."""
import pytest
import torch
import torch.nn.functional as F


@pytest.mark.parametrize("Cout,Cin,R", [(33, 16, 3), (11, 32, 1), (128, 256, 3)])
def test_dgrad_pack_is_the_rotated_transposed_weight(Cout, Cin, R):
    from openess_amd import hip
    g = torch.Generator().manual_seed(Cout * 7 + Cin + R)
    pad = (R - 1) // 2
    w = torch.randn(Cout, Cin, R, R, generator=g)
    packed = hip.pack_conv_weight_f32_dgrad(w)
    Kp, Cp = (R * R * Cout + 15) // 16 * 16, (Cin + 31) // 32 * 32
    assert packed.shape == (Kp, Cp) and packed.dtype == torch.float32
    # the padding is zero: the forward kernel multiplies it
    assert not packed[R * R * Cout:].any() and not packed[:, Cin:].any()
    wd = packed[:R * R * Cout, :Cin].reshape(R, R, Cout, Cin).permute(3, 2, 0, 1)         # [Cin, Cout, R, R]
    assert torch.equal(wd, w.flip(2, 3).permute(1, 0, 2, 3))
    x = torch.randn(2, Cin, 6, 5, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(2, Cout, 6, 5, generator=g, dtype=torch.float64)
    want, = torch.autograd.grad(F.conv2d(x, w.double(), padding=pad), x, dy)
    got = F.conv2d(dy, wd.double(), padding=R - 1 - pad)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
