"""Route coverage of the bf16 weight-gradient dispatch (no GPU): oess_conv2d_wgrad_route returns the kernel and slice count of the
plan the launch itself executes (wgrad_plan), so these assertions pin which gradient kernel and which reduce kernel every row of
tests/wgrad_route_cases.py runs on, and that the rows together reach all eight gradient kernels, both reduce kernels and the
error returns.  A threshold edit that moves a parity case to another kernel fails here on any machine."""
import pytest

from tests import wgrad_route_cases as wc

KERNELS = wc.header_kernels()
_NAMES = {v: k for k, v in KERNELS.items()}


def _query(geom, x_ps, dy_ps, workspace_bytes):
    from openess_amd import _lib
    B, H, W, Cin_x, Cin, Cout, R, S, stride, pad, dil = geom
    xps, dps = wc.strides(geom, x_ps, dy_ps)
    return _lib.load().oess_conv2d_wgrad_route(B, H, W, Cin_x, Cout, Cin, R, S, stride, pad, dil, xps, dps, workspace_bytes)


def _say(r):
    return f"{_NAMES.get(r & 0xff, '?')} x {r >> 8}" if r > 0 else str(r)


@pytest.mark.parametrize("name,geom,x_ps,dy_ps,ws,want_kernel,want_slices,_why", wc.WGRAD_CASES, ids=[r[0] for r in wc.WGRAD_CASES])
def test_row_reaches_its_kernel(name, geom, x_ps, dy_ps, ws, want_kernel, want_slices, _why):
    got = _query(geom, x_ps, dy_ps, ws)
    if want_kernel in wc.ERRORS:
        assert got == wc.ERRORS[want_kernel], f"{name}: meant to return {want_kernel}, dispatch says {_say(got)}"
    else:
        assert got == (KERNELS[want_kernel] | want_slices << 8), f"{name}: meant for {want_kernel} x {want_slices}, dispatch says {_say(got)}"


def test_wrapper_query_agrees_with_the_library():
    """hip.conv2d_wgrad_route on a shape: the same numbers, errors raised like the call's."""
    from openess_amd import hip
    for name, geom, x_ps, dy_ps, ws, want_kernel, want_slices, _ in wc.WGRAD_CASES:
        B, H, W, Cin_x, Cin, Cout, R, S, stride, pad, dil = geom
        xps, dps = wc.strides(geom, x_ps, dy_ps)
        args = ((B, H, W, Cin_x), None, Cout, Cin, R, S, stride, pad, dil)
        kw = dict(workspace=ws, x_pix_stride=xps, dy_pix_stride=dps)
        if want_kernel in wc.ERRORS:
            with pytest.raises(RuntimeError, match=str(wc.ERRORS[want_kernel])):
                hip.conv2d_wgrad_route(*args, **kw)
        else:
            assert hip.conv2d_wgrad_route(*args, **kw) == _query(geom, x_ps, dy_ps, ws), name
            if ws == wc.DEFAULT_WS:                 # the wrapper's default offer is the 256 MiB buffer of hip.conv2d_wgrad
                del kw["workspace"]
                assert hip.conv2d_wgrad_route(*args, **kw) == _query(geom, x_ps, dy_ps, ws), name


def test_table_covers_every_kernel_both_reducers_and_the_errors():
    assert sorted(KERNELS) == sorted(["REG_32", "REG_64", "REG_128", "DMA_32", "DMA_64", "DMA_128", "STRIP_32", "STRIP_64"])
    launched = [r for r in wc.WGRAD_CASES if r[5] not in wc.ERRORS]
    pinned = {r[5] for r in launched}
    assert pinned == set(KERNELS), f"no row reaches {sorted(set(KERNELS) - pinned)}"
    slices = {r[6] for r in launched}
    # narrow reduce: a tail without a round (1..3), rounds without a tail (4), rounds and a tail (15); wide reduce from 16 on,
    # at its threshold, with and without a tail on every lane, and at the strip kernels' hundreds of slices
    assert {1, 2, 3, 4, 15} <= slices and min(s for s in slices if s >= 16) == 16 and max(slices) >= 256, sorted(slices)
    assert {r[5] for r in wc.WGRAD_CASES if r[5] in wc.ERRORS} == {"ENOMEM"}
    # both tensors take the 2 GiB route, and the row just under the limit does not
    assert any(r[2] == wc.HUGE_PS for r in launched) and any(r[3] == wc.HUGE_PS for r in launched)
    assert any(r[2] == wc.BELOW_PS and r[5].startswith("DMA") for r in launched)
    # Cin_x > Cin, R != S and a workspace-limited plan are present
    assert any(r[1][3] > r[1][4] for r in launched) and any(r[1][6] != r[1][7] for r in launched)
    assert sum(r[4] != wc.DEFAULT_WS for r in launched) >= 5
    assert all(len(r[7]) > 10 for r in wc.WGRAD_CASES), "every row says what it is for"
    assert len({r[0] for r in wc.WGRAD_CASES}) == len(wc.WGRAD_CASES)


def test_extent_limit_is_where_the_table_says():
    """0x7ffffff0 bytes: the byte span of the strided rows sits on either side of it, for x and for dy."""
    lim = 0x7ffffff0
    assert (89 * wc.HUGE_PS + 16) * 2 == 2147484592 >= lim > (89 * wc.BELOW_PS + 16) * 2 == 2147483168
    assert (89 * wc.HUGE_PS + 40) * 2 >= lim and wc.HUGE_PS - wc.BELOW_PS == 8
    g = (2, 5, 9, 16, 16, 40, 3, 3, 1, 1, 1)
    assert _query(g, 32, wc.BELOW_PS, wc.DEFAULT_WS) == (KERNELS["DMA_64"] | 10 << 8)
    assert _query(g, 32, wc.HUGE_PS, wc.DEFAULT_WS) == (KERNELS["REG_64"] | 10 << 8)


def test_workspace_moves_a_call_between_plans():
    """the strip kernels need their units' partials to fit; the tiled kernels shrink their slice count down to one"""
    name, geom = "strip32", wc._STRIP32
    per = 81920
    assert _query(geom, wc.SLICE, wc.SLICE, 441 * per) == (KERNELS["STRIP_32"] | 441 << 8)
    assert _query(geom, wc.SLICE, wc.SLICE, 441 * per - 1) == (KERNELS["DMA_32"] | 84 << 8)
    assert _query(geom, wc.SLICE, wc.SLICE, 5 * per - 1) == (KERNELS["DMA_32"] | 4 << 8)
    assert _query(geom, wc.SLICE, wc.SLICE, per) == (KERNELS["DMA_32"] | 1 << 8)
    assert _query(geom, wc.SLICE, wc.SLICE, per - 1) == wc.ERRORS["ENOMEM"]
    assert _query(geom, wc.SLICE, wc.SLICE, 0) == wc.ERRORS["ENOMEM"]


_OK = (2, 5, 9, 16, 16, 24, 3, 3, 1, 1, 1)


def _launch(geom, xps, dps, x=4096, dy=8192, dw=12288, ws=16384, ws_bytes=wc.DEFAULT_WS):
    """oess_conv2d_wgrad_bf16 itself, with pointers that are never dereferenced: only for calls that the query (the same plan)
    has just refused, which therefore return before any launch"""
    from openess_amd import _lib
    lib = _lib.load()
    B, H, W, Cin_x, Cin, Cout, R, S, stride, pad, dil = geom
    if x and dy and dw and ws:
        assert lib.oess_conv2d_wgrad_route(B, H, W, Cin_x, Cout, Cin, R, S, stride, pad, dil, xps, dps, ws_bytes) < 0
    return lib.oess_conv2d_wgrad_bf16(x, xps, B, H, W, Cin_x, dy, dps, Cout, Cin, R, S, stride, pad, dil, dw, ws, ws_bytes, None)


@pytest.mark.parametrize("which", ["x", "dy", "dw", "ws"])
def test_launch_refuses_null_pointers(which):
    assert _query(_OK, 16, 24, wc.DEFAULT_WS) == (KERNELS["DMA_32"] | 10 << 8)       # the numbers themselves are fine
    assert _launch(_OK, 16, 24, **{which: None}) == wc.ERRORS["EINVAL"]


@pytest.mark.parametrize("name,geom,xps,dps", wc.EINVAL_CASES, ids=[r[0] for r in wc.EINVAL_CASES])
def test_launch_refuses_bad_numbers(name, geom, xps, dps):
    assert _query(geom, xps, dps, wc.DEFAULT_WS) == wc.ERRORS["EINVAL"], name
    assert _launch(geom, xps, dps) == wc.ERRORS["EINVAL"], name


def test_launch_refuses_a_short_workspace():
    assert _launch(wc._S2, 88, 56, ws_bytes=196608 - 1) == wc.ERRORS["ENOMEM"]
