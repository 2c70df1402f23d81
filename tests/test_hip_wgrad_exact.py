"""Exact-arithmetic GPU parity of every bf16 weight-gradient kernel (rows of tests/wgrad_route_cases.py).

Operands make the fp32 accumulation order irrelevant: x and dy are integers in [-2, 2] at density 0.5 (exact in bf16), so every
product and every partial sum is an integer of magnitude <= 4 * B * Ho * Wo < 2^24: MFMA order, K-step raggedness, slice count
and the association of either reduce kernel cannot change a bit.  The reference is torch.nn.grad.conv2d_weight in float64 on the
CPU from the same tensors and the tolerance is ZERO (torch.equal): one dropped or doubled pixel anywhere changes an integer.
The bound and a floor of 0.5 on the non-zero share of the reference are asserted on the reference alone, before the kernel
result is looked at.

The operands are what the engine passes: x is the channel slice [8 : 8 + Cin_x] of a wider buffer filled with 7.0, whose channels
Cin .. Cin_x - 1 are 7.0 as well (contractually ignored), dy a slice of a buffer filled with 5.0, so a read outside the operands
changes integers.  The rows of the 2 GiB rule place their 90 pixels 24 MB apart in one flat uninitialised buffer.  dW and the
caller-owned workspace start as NaN: an element the reduce kernel leaves unwritten, or a stale partial it reads, is a NaN in the
result, and the 4 KiB behind the workspace on offer must stay as they were.  Each call first asserts its kernel and slice
count with hip.conv2d_wgrad_route on the real tensors."""
import functools

import pytest
import torch

from tests import wgrad_route_cases as wc

pytestmark = pytest.mark.gpu

KERNELS = wc.header_kernels()
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _operands(geom):
    """(x [B,H,W,Cin], dy [B,Ho,Wo,Cout], ref [Cout,Cin,R,S]) in float64 on the CPU, one set per geometry (rows that differ in the
    workspace alone share it); nobody writes to them"""
    B, H, W, Cin_x, Cin, Cout, R, S, stride, pad, dil = geom
    Ho, Wo = wc.out_size(geom)
    g = torch.Generator().manual_seed(2000 + sum(geom))
    x = torch.randint(-2, 3, (B, H, W, Cin), generator=g).double() * (torch.rand((B, H, W, Cin), generator=g) < 0.5)
    dy = torch.randint(-2, 3, (B, Ho, Wo, Cout), generator=g).double() * (torch.rand((B, Ho, Wo, Cout), generator=g) < 0.5)
    ref = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), (Cout, Cin, R, S), dy.permute(0, 3, 1, 2), stride=stride, padding=pad,
                                      dilation=dil)
    # conditions on the inputs, asserted on the reference alone
    assert 4 * B * Ho * Wo < 2 ** 24 and float(ref.abs().max()) <= 4 * B * Ho * Wo
    assert torch.equal(ref, ref.round())
    share = float((ref != 0).double().mean())
    assert share >= 0.5, f"only {share:.3f} of the reference is non-zero"
    return x, dy, ref


def _view(vals, C_view, ps, fill):
    """vals [B,h,w,C] (CPU float64) as a bf16 CUDA view [B,h,w,C_view] with pixel stride ps.  SLICE: channels [8 : 8 + C_view] of a
    buffer 16 channels wider filled with `fill` (C .. C_view - 1 keep it); a number: pixels ps elements apart in one flat
    uninitialised buffer, of which only the pixels are written.  Returns (view, its buffer)."""
    B, h, w, C = vals.shape
    v = vals.bfloat16().cuda()
    if ps == wc.SLICE:
        buf = torch.full((B, h, w, C_view + 16), fill, dtype=torch.bfloat16, device="cuda")
        buf[..., 8:8 + C] = v
        return buf[..., 8:8 + C_view], buf
    assert C == C_view
    buf = torch.empty(8 + (B * h * w - 1) * ps + C, dtype=torch.bfloat16, device="cuda")
    view = buf.as_strided((B, h, w, C), (h * w * ps, w * ps, ps, 1), 8)
    view.copy_(v)
    return view, buf


def _nan_workspace(nbytes):
    """(the nbytes on offer, the 4 KiB and more behind them), one NaN-filled allocation"""
    words = (nbytes + 4096 + 3) // 4 + 1
    raw = torch.full((words,), NAN, dtype=torch.float32, device="cuda").view(torch.uint8)
    return raw[:nbytes], raw[nbytes:]


@pytest.mark.parametrize("name,geom,x_ps,dy_ps,ws_bytes,want_kernel,want_slices,_why", wc.WGRAD_CASES, ids=[r[0] for r in wc.WGRAD_CASES])
def test_wgrad_row_is_exact(name, geom, x_ps, dy_ps, ws_bytes, want_kernel, want_slices, _why):
    from openess_amd import hip
    B, H, W, Cin_x, Cin, Cout, R, S, stride, pad, dil = geom
    x, dy, ref = _operands(geom)
    xv, xbuf = _view(x, Cin_x, x_ps, 7.0)
    dv, dbuf = _view(dy, Cout, dy_ps, 5.0)
    assert (xv.stride(2), dv.stride(2)) == wc.strides(geom, x_ps, dy_ps) and xv.data_ptr() % 16 == 0 and dv.data_ptr() % 16 == 0
    ws, tail = _nan_workspace(ws_bytes)
    assert ws.numel() == ws_bytes and tail.numel() >= 4096
    tail_before = tail.clone()
    dw = torch.full((Cout, Cin, R, S), NAN, dtype=torch.float32, device="cuda")
    args = (xv, dv, Cout, Cin, R, S, stride, pad, dil)
    try:
        if want_kernel in wc.ERRORS:
            code = str(wc.ERRORS[want_kernel])
            with pytest.raises(RuntimeError, match=code):
                hip.conv2d_wgrad_route(*args, workspace=ws)
            with pytest.raises(RuntimeError, match=code):
                hip.conv2d_wgrad(*args, workspace=ws, out=dw)
            torch.cuda.synchronize()
            assert bool(torch.isnan(dw).all()), f"{name}: a refused call wrote to dW"
            assert bool(torch.isnan(ws[:ws_bytes // 4 * 4].view(torch.float32)).all()), f"{name}: a refused call wrote to the workspace"
        else:
            got = hip.conv2d_wgrad_route(*args, workspace=ws)
            assert got == (KERNELS[want_kernel] | want_slices << 8), \
                f"{name}: meant for {want_kernel} x {want_slices}, dispatch says kernel {got & 0xff} x {got >> 8}"
            out = hip.conv2d_wgrad(*args, workspace=ws, out=dw)
            torch.cuda.synchronize()
            assert out is dw and tuple(dw.shape) == (Cout, Cin, R, S) and dw.dtype == torch.float32
            res = dw.cpu().double()
            assert torch.equal(res, ref), f"{name}: {int((res != ref).sum())} of {ref.numel()} elements differ ({int(torch.isnan(res).sum())} NaN)"
        assert torch.equal(tail, tail_before), f"{name}: bytes behind the {ws_bytes} on offer were written"
    finally:
        del xv, dv, xbuf, dbuf, ws, tail, tail_before
        if wc.HUGE_PS in (x_ps, dy_ps) or wc.BELOW_PS in (x_ps, dy_ps):
            torch.cuda.empty_cache()       # hand the 2 GiB buffer back before the next row


def test_default_workspace_and_fresh_output_are_unchanged_behaviour():
    """Without workspace= and out= the call is the one the engine makes: the cached 256 MiB buffer, whatever it last held (here:
    NaN throughout), and a new dW.  A workspace or an output of the wrong type or shape is refused before the library is called."""
    from openess_amd import hip
    name, geom = wc.WGRAD_CASES[0][:2]
    B, H, W, Cin_x, Cin, Cout, R, S, stride, pad, dil = geom
    x, dy, ref = _operands(geom)
    xv, _ = _view(x, Cin_x, wc.SLICE, 7.0)
    dv, _ = _view(dy, Cout, wc.SLICE, 5.0)
    cached = hip._workspace(wc.DEFAULT_WS, xv.device, tag="wgrad")
    assert cached.numel() == wc.DEFAULT_WS
    cached.view(torch.float32).fill_(NAN)
    dw = hip.conv2d_wgrad(xv, dv, Cout, Cin, R, S, stride, pad, dil)
    assert tuple(dw.shape) == (Cout, Cin, R, S) and torch.equal(dw.cpu().double(), ref)
    with pytest.raises(ValueError):
        hip.conv2d_wgrad(xv, dv, Cout, Cin, R, S, stride, pad, dil, workspace=torch.zeros(1 << 20, device="cuda"))     # not uint8
    with pytest.raises(ValueError):
        hip.conv2d_wgrad(xv, dv, Cout, Cin, R, S, stride, pad, dil, out=torch.zeros(Cout, Cin_x, R, S, device="cuda"))
