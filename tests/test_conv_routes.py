"""Route coverage of the convolution dispatch (no GPU): oess_conv2d_fwd_route is the route of the plan the launch itself
executes (conv_plan), so these assertions pin which kernel every row of tests/conv_route_cases.py runs on, and that
the rows together reach every kernel the library declares.  A new kernel without a row, or a threshold change that moves a
parity case to another kernel, fails here on any machine."""
import pytest

from tests import conv_route_cases as rc

ROUTES = rc.header_routes()
_ROWS = [(name, geom, variant, want) for name, geom, routes, _ in rc.ROUTE_CASES for variant, want in routes.items()]


@pytest.fixture(autouse=True)
def _no_dispatch_knobs(monkeypatch):
    """the A/B environment knobs of the w128 rules would move rows between kernels"""
    for k in ("OESS_W128_CONV3", "OESS_W128_GEMM", "OESS_W128_MIN_TILES", "OESS_W128_NT", "OESS_W128_WHY"):
        monkeypatch.delenv(k, raising=False)


def _route(geom, variant):
    from openess_amd import hip
    B, H, W, Cin, Cout, R, stride, pad, dil = geom
    a = rc.VARIANTS[variant]
    ps_in, ps_out, ps_res = rc.strides(geom, variant)
    return hip.conv2d_route((B, H, W, Cin), None, a.get("bias", False), Cout, R, R, stride, pad, dil, relu=a.get("relu", False),
                            residual=a.get("residual", False), out_f32=a.get("out_f32", False), tile_stats=a.get("tile_stats", False),
                            in_pix_stride=ps_in, out_pix_stride=ps_out, res_pix_stride=ps_res)


@pytest.mark.parametrize("name,geom,variant,want", _ROWS, ids=[f"{r[0]}-{r[2]}" for r in _ROWS])
def test_row_reaches_its_kernel(name, geom, variant, want):
    from openess_amd import hip
    got = _route(geom, variant)
    assert got == rc.route_value(ROUTES, want), f"{name}/{variant}: meant for {want}, dispatch says {hip.conv2d_route_name(got)} ({got})"


@pytest.mark.parametrize("name,call,want,_why", rc.LSTM_ROUTE_CASES, ids=[r[0] for r in rc.LSTM_ROUTE_CASES])
def test_convlstm_row_reaches_its_kernel(name, call, want, _why):
    from openess_amd import hip
    got = hip.convlstm_route(*call)
    assert got == ROUTES[want], f"{name}: meant for {want}, dispatch says {hip.conv2d_route_name(got)} ({got})"


def test_table_covers_every_declared_route():
    from openess_amd import _lib
    lib = _lib.load()
    declared = set(range(1, lib.oess_conv2d_route_count() + 1))
    assert declared == set(ROUTES.values()), "include/oess.h and the library disagree about the routes"
    pinned = {rc.route_value(ROUTES, w) & 0xff for _, _, routes, _ in rc.ROUTE_CASES for w in routes.values()}
    pinned |= {ROUTES[w] for _, _, w, _ in rc.LSTM_ROUTE_CASES}
    names = {v: k for k, v in ROUTES.items()}
    assert pinned == declared, f"no row of ROUTE_CASES reaches {sorted(names[v] for v in declared - pinned)}"
    for v in declared:
        assert lib.oess_conv2d_route_name(v) not in (b"?", b""), names[v]
    # every row says what it is for
    assert all(len(why) > 10 for *_, why in rc.ROUTE_CASES + rc.LSTM_ROUTE_CASES)


def test_split_k_rows_resolve_to_several_slice_counts():
    ks = {}
    for _, _, routes, _ in rc.ROUTE_CASES:
        for w in routes.values():
            if isinstance(w, tuple):
                ks.setdefault(w[0], set()).add(w[1])
    assert len(ks["SPLITK_FASTK"]) >= 2 and len(ks["SPLITK_SLOWK"]) >= 2, ks


def test_route_follows_the_call_not_only_the_geometry():
    """The arguments beyond the geometry move a call between kernels: the workspace on offer (split-K), the output pointer's
    alignment (the w128 and stride-2 kernels), and a 2 GiB input extent (register-staged fallback)."""
    from openess_amd import hip
    sk = (1, 15, 17, 256), 132
    assert hip.conv2d_route(sk[0], None, True, sk[1], 3, 3, 1, 1, 1) & 0xff == ROUTES["SPLITK_FASTK"]
    assert hip.conv2d_route(sk[0], None, True, sk[1], 3, 3, 1, 1, 1, allow_splitk=False) == ROUTES["TILE64_FASTK"]
    s2 = (1, 9, 35, 32), 64
    assert hip.conv2d_route(s2[0], None, True, s2[1], 5, 5, 2, 2, 1) == ROUTES["S2_HALO"]
    assert hip.conv2d_route(s2[0], None, True, s2[1], 5, 5, 2, 2, 1, out_aligned16=False) == ROUTES["DMA64_SLOWK"]
    big = (2, 257, 256, 256), 256
    assert hip.conv2d_route(big[0], None, False, big[1], 1, 1) == ROUTES["CONV1X1_W128"]
    assert hip.conv2d_route(big[0], None, False, big[1], 1, 1, out_aligned16=False) == ROUTES["TILE256"]
    # the same 1x1 layer read from a buffer whose pixel stride puts the last pixel past 2 GiB
    assert hip.conv2d_route((1, 9, 20, 320), None, True, 72, 1, 1) == ROUTES["DMA128_FASTK"]
    assert hip.conv2d_route((1, 9, 20, 320), None, True, 72, 1, 1, in_pix_stride=1 << 23) == ROUTES["FALLBACK_128"]
    with pytest.raises(RuntimeError, match="invalid argument"):
        hip.conv2d_route((1, 9, 20, 12), None, True, 72, 1, 1)          # Cin % 8 != 0
    with pytest.raises(RuntimeError, match="invalid argument"):
        hip.convlstm_route((1, 9, 20, 128), 24, 3, 1)                   # C_hidden % 32 != 0
