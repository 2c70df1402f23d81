"""CPU test of hip.pack_conv_weight_f32_dgrad_s2 (K21): the packed operand of oess_conv2d_dgrad_s2_f32 is replayed phase by phase
in torch float64, following the layout documented in include/oess.h alone (four blocks by tap parity class; phase (py, px)
reads class ((py + pad) & 1, (px + pad) & 1) at dy[q + (py + pad - r) / 2]), and must reproduce torch.autograd.grad of
F.conv2d(stride=2) to 1e-12.  Needs neither the library nor a GPU."""
import pytest
import torch
import torch.nn.functional as F

from openess_amd import hip


def replay(dy, packed, Cout, Cin, H, W, R, pad):
    """dx [B, Cin, H, W] (float64) from dy [B, Cout, Ho, Wo] and the packed operand; every element assigned exactly once"""
    B, _, Ho, Wo = dy.shape
    Cp = (Cin + 31) // 32 * 32
    n_of = lambda par: (R - par + 1) // 2                                        # noqa: E731
    rows = [(n_of(c >> 1) * n_of(c & 1) * Cout + 15) // 16 * 16 for c in range(4)]
    offs = [sum(rows[:c]) * Cp for c in range(4)]
    assert packed.numel() == sum(rows) * Cp
    dx = torch.full((B, Cin, H, W), float('nan'), dtype=torch.float64)
    written = torch.zeros((H, W), dtype=torch.int64)
    for py in range(2):
        for px in range(2):
            ry, rx = (py + pad) & 1, (px + pad) & 1
            ny, nx = n_of(ry), n_of(rx)
            c = 2 * ry + rx
            blk = packed[offs[c]:offs[c] + rows[c] * Cp].reshape(rows[c], Cp)
            assert float(blk[ny * nx * Cout:].abs().sum()) == 0 and float(blk[:, Cin:].abs().sum()) == 0      # zero padding
            wt = blk[:ny * nx * Cout, :Cin].reshape(ny, nx, Cout, Cin)
            Hq, Wq = len(range(py, H, 2)), len(range(px, W, 2))
            out = torch.zeros((B, Cin, Hq, Wq), dtype=torch.float64)
            for ty in range(ny):
                for tx in range(nx):
                    for qy in range(Hq):
                        oy = qy + (py + pad - ry) // 2 - ty
                        if not 0 <= oy < Ho:
                            continue
                        for qx in range(Wq):
                            ox = qx + (px + pad - rx) // 2 - tx
                            if 0 <= ox < Wo:
                                out[:, :, qy, qx] += dy[:, :, oy, ox] @ wt[ty, tx]
            dx[:, :, py::2, px::2] = out
            written[py::2, px::2] += 1
    assert int(written.min()) == int(written.max()) == 1
    return dx


@pytest.mark.parametrize("H,W", [(7, 9), (8, 10), (7, 10)])
@pytest.mark.parametrize("R,pad", [(1, 0), (3, 0), (3, 1)])
def test_dgrad_s2_pack_replays_to_autograd(R, pad, H, W):
    B, Cin, Cout = 2, 5, 3
    g = torch.Generator().manual_seed(17 * R + 3 * pad + H + W)
    w = torch.randn(Cout, Cin, R, R, generator=g)
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w.double(), stride=2, padding=pad)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    want, = torch.autograd.grad(y, [x], dy)
    packed = hip.pack_conv_weight_f32_dgrad_s2(w)
    assert packed.dtype == torch.float32 and packed.ndim == 1 and packed.is_contiguous()
    got = replay(dy, packed.double(), Cout, Cin, H, W, R, pad)
    assert not torch.isnan(got).any()
    assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)
    if R == 1:                                                   # a 1 x 1 stride-2 conv never reads the odd rows and columns
        assert float(got[:, :, 1::2].abs().max()) == 0 and float(got[:, :, :, 1::2].abs().max()) == 0


def test_dgrad_s2_pack_refuses_other_kernels():
    for shape in ((4, 4, 5, 5), (4, 4, 7, 7), (4, 4, 3, 1)):
        with pytest.raises(ValueError):
            hip.pack_conv_weight_f32_dgrad_s2(torch.zeros(shape))
