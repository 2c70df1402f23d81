"""K38: the bf16 ConvLSTM kernels -- the single launch on its three routes (conv3x3_halo.h, conv_general.h), the 256-row grouped
launch, the persistent w128 kernel (conv_lstm_w128.h) and the unfused gate kernel (pointwise.hip) -- against expectations
computed on the host.

References: tests/convlstm_cases.py (operands, the exact cases and their integer expectations) and tests/convlstm_reference.py
(float64 restatement of one step, CPU); tests/test_convlstm_host.py proves both without a GPU.
  Exact cases: one-hot gate rows of magnitude 256 over every tap and both halves of cat(x, h), +-128 biases, +-1 operands, the
    previous cell in {0, +-40}: every pre-activation is an integer of magnitude >= 128, the sigmoids are exactly 0 or 1 and
    tanh(gc) exactly +-1 in fp32 (rcp(1 + __expf(-x)) with __expf -> 0 or inf), so the fp32 cell is an integer and the bf16
    hidden state one of {0, +-1, +-bf16(tanh(1)) = +-0.76171875} (after a second step also +-bf16(tanh(2)) = +-0.96484375): every
    output is compared with torch.equal.  Every output buffer is NaN on entry; in the zero-state form the cell buffer too.
  float64 bounds on seeded random operands, one launch per comparison, the reference on the launch's own operands (bf16-rounded
    x, h, weight; fp32 bias and cell).  Measured max |cell - float64| on the MI355X (MEASURED_CELL_DEV): single launch 1.064e-6
    over its ten cases (largest at (3, 8, 8, 96, 32), 5 x 5, LSTM_FASTK; row-halo 8.67e-7, slow K 6.30e-7), w128 7.99e-7, unfused
    gate kernel 1.98e-7 -> CELL_BOUND = 4 x 1.064e-6 = 4.26e-6 absolute (cells are O(1); the margin is for other seeds and the
    data-dependent error of __expf, as K28).  The hidden state is held to half a bf16 ulp of the float64 value plus
    CELL_BOUND, elementwise; measured beyond the half ulp: at most 8.9e-8."""
import ctypes
import functools

import pytest
import torch

from tests import conv_route_cases as rc
from tests import convlstm_cases as cases
from tests import convlstm_reference as ref

pytestmark = pytest.mark.gpu
ROUTES = rc.header_routes()
EINVAL = -22
NAN = float('nan')
# max |cell - float64| printed by the tests below on one MI355X (pytest -s), by launch
MEASURED_CELL_DEV = {'single launch, 10 cases': 1.0636856950796414e-06, 'w128': 7.986044865404551e-07, 'unfused gate kernel': 1.9789753302745794e-07}
CELL_BOUND = 4.26e-6                    # four times the largest measured deviation (module docstring)
LAYOUTS = ('dense', 'cat', 'cat+2')     # the hidden output: a tensor of its own; the h window of a cat(x, h) buffer; the same with a
                                        # pixel stride that is even but no multiple of 8 (the epilogue's 4-byte stores)


def nhwc(t):
    """fp32 [B, C, H, W] on the CPU -> fp32 [B, H, W, C] on the GPU."""
    return t.float().permute(0, 2, 3, 1).contiguous().cuda()


def nchw(t):
    """[B, H, W, C] device tensor -> fp32 [B, C, H, W] on the CPU."""
    return t.float().permute(0, 3, 1, 2).contiguous().cpu()


@functools.lru_cache(maxsize=None)
def exact(geom, k):
    """(case, {zero-state form?: (cell int64, hidden fp32)}) of an exact case, computed once."""
    c = cases.exact_case(*geom, k)
    return c, {f: cases.exact_expected(c, f)[1:] for f in (False, True)}


def problem(case, k, fresh, layout='cat', cell=None):
    """One problem tuple of hip.convlstm_fused / _group from a case: (problem, the buffer the hidden output lies in).  Outputs are
    NaN on entry: the hidden buffer, in the zero-state form the cell and the unread h window of the input as well."""
    from openess_amd import hip
    B, Cx, H, W = case['x'].shape
    C = case['h'].shape[1]
    xh = torch.full((B, H, W, Cx + C), NAN, device='cuda', dtype=torch.bfloat16)
    xh[..., :Cx] = nhwc(case['x']).bfloat16()
    if not fresh:
        xh[..., Cx:] = nhwc(case['h']).bfloat16()
    w = case['w'].cuda()
    packed = hip.pack_conv_weight(w[:, :Cx] if fresh else w, flip=2)
    if cell is None:
        cell = torch.full((B, H, W, C), NAN, device='cuda') if fresh else nhwc(case['c'])
    out = torch.full((B, H, W, {'dense': C, 'cat': Cx + C, 'cat+2': Cx + C + 2}[layout]), NAN, device='cuda', dtype=torch.bfloat16)
    hidden = out if layout == 'dense' else out[..., Cx:Cx + C]
    return (xh[..., :Cx] if fresh else xh, packed, case['b'].cuda(), cell, hidden, k, k // 2, fresh), out


def assert_route(p, want):
    from openess_amd import hip
    got = hip.convlstm_route(p[0], p[4].shape[3], p[5], p[6], hidden_pix_stride=p[4].stride(2))
    assert got == ROUTES[want], f"meant for {want}, dispatch says {hip.conv2d_route_name(got)}"


def assert_exact(p, out, want, cell=None):
    """Cell and hidden state equal the host's integers bit for bit; everything around the hidden window is still NaN."""
    cell_want, hidden_want = want
    cell = p[3] if cell is None else cell
    C, Cx = p[4].shape[3], p[4].storage_offset() - out.storage_offset()           # the window is out[..., Cx:Cx + C]
    assert torch.equal(nchw(cell), cell_want.float()), float((nchw(cell) - cell_want.float()).abs().max())
    assert torch.equal(nchw(p[4]), hidden_want), float((nchw(p[4]) - hidden_want).abs().max())
    assert bool(torch.isnan(out[..., :Cx].float()).all()) and bool(torch.isnan(out[..., Cx + C:].float()).all())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fresh", [False, True], ids=["prev", "zero"])
@pytest.mark.parametrize("geom,k,routes", cases.EXACT_SINGLE + [cases.EXACT_LARGE], ids=lambda v: str(v).replace(' ', '') if isinstance(v, tuple) else None)
def test_single_launch_exact(geom, k, routes, fresh, layout):
    """hip.convlstm_fused on every route, from a previous cell and in the zero-state form, the hidden output dense or a window
    of a wider buffer: cell and hidden state bit for bit.  Pins every tap, both halves of cat(x, h), the four gates' rows of the
    gate-interleaved packing, the bias of every row whose tap meets the padding, every 32-block of hidden channels, ragged tiles,
    the batch border and the second round of workgroups."""
    from openess_amd import hip
    c, want = exact(geom, k)
    p, out = problem(c, k, fresh, layout)
    assert_route(p, routes[fresh])
    hip.convlstm_fused(*p)
    torch.cuda.synchronize()
    assert_exact(p, out, want[fresh])


@pytest.mark.parametrize("fresh", [(False, True, False), (True, False, True)], ids=["zero-in-the-middle", "zero-outside"])
def test_grouped_launch_exact(fresh):
    """hip.convlstm_fused_group (three row-halo problems in one launch of 256-row tiles), zero-state and given cells mixed: each
    problem gives its OWN expectation, which test_convlstm_fused_group_equals_separate_launches (group == single) cannot see."""
    from openess_amd import hip
    probs, outs, wants = [], [], []
    for (B, H, W, C), f in zip(cases.GROUP, fresh):
        c, want = exact((B, H, W, C, C), 3)
        p, out = problem(c, 3, f)
        assert_route(p, 'HALO3X3_LSTM')
        probs.append(p), outs.append(out), wants.append(want[f])
    assert len(hip.convlstm_fused_group(probs)) == 3
    torch.cuda.synchronize()
    for p, out, want in zip(probs, outs, wants):
        assert_exact(p, out, want)


def w128_cell(c, B, H, W, C, fresh):
    """The w128-tiled cell buffer of a case: NaN in the zero-state form, else the case's cell through the relayout."""
    from openess_amd import hip
    px = B * H * W
    if fresh:
        return torch.full((hip.convlstm_w128_cell_elems(px, C),), NAN, device='cuda')
    return hip.convlstm_w128_cell_relayout(nhwc(c['c']).reshape(px, C), px, C, True)


def w128_cell_nhwc(cell, B, H, W, C):
    from openess_amd import hip
    return hip.convlstm_w128_cell_relayout(cell, B * H * W, C, False).reshape(B, H, W, C)


@pytest.mark.parametrize("geoms,fresh", [(cases.W128[:1], (False,)), (cases.W128[:1], (True,)), (cases.W128[1:], (False,)),
                                         (cases.W128[1:], (True,)), (cases.W128, (False, True)), (cases.W128, (True, False))],
                         ids=["64-prev", "64-zero", "128-prev", "128-zero", "both-prev-zero", "both-zero-prev"])
def test_w128_launch_exact_two_steps(geoms, fresh):
    """hip.convlstm_w128_group: two recurrent steps, the cell passed through convlstm_w128_cell_relayout both ways and kept in the
    kernel's tiled layout in between, so the second step reads what the first one wrote.  Second step: a new exact x and h, the
    cell kept; its values are then in cases.possible_cells(2)."""
    from openess_amd import hip
    from openess_amd.e2vid.model.submodules import ConvLSTM
    st = []
    for (B, H, W, C), f in zip(geoms, fresh):
        assert ConvLSTM(C, C, 3).w128_ok(B, H, W)
        c, want = exact((B, H, W, C, C), 3)
        cell = w128_cell(c, B, H, W, C, f)
        p, out = problem(c, 3, f, cell=cell)
        assert_route(p, 'HALO3X3_LSTM')
        st.append(dict(g=(B, H, W, C), p=p, out=out, want=want[f], cell=cell))
    assert hip.convlstm_w128_group([s['p'] for s in st]) is True
    torch.cuda.synchronize()
    for s in st:
        assert_exact(s['p'], s['out'], s['want'], cell=w128_cell_nhwc(s['cell'], *s['g']))
    for s in st:
        B, H, W, C = s['g']
        c2 = cases.exact_case(B, H, W, C, C, 3, seed=4)
        c2['c'] = s['want'][0].float()
        s['want'] = cases.exact_expected(c2)[1:]
        assert set(s['want'][0].unique().tolist()) <= set(cases.possible_cells(2))
        s['p'], s['out'] = problem(c2, 3, False, cell=s['cell'])
    assert hip.convlstm_w128_group([s['p'] for s in st]) is True
    torch.cuda.synchronize()
    for s in st:
        assert_exact(s['p'], s['out'], s['want'], cell=w128_cell_nhwc(s['cell'], *s['g']))


def gates_problem(g, fresh):
    """Buffers of hip.convlstm_gates: the gates in a buffer whose pixel stride is wider than 4C, the hidden output a window of a
    wider buffer, everything else NaN."""
    B, C4, H, W = g['gates'].shape
    C = C4 // 4
    gbuf = torch.full((B, H, W, C4 + 8), NAN, device='cuda', dtype=torch.bfloat16)
    gbuf[..., :C4] = nhwc(g['gates']).bfloat16()
    cell = torch.full((B, H, W, C), NAN, device='cuda') if fresh else nhwc(g['c'])
    out = torch.full((B, H, W, C + 24), NAN, device='cuda', dtype=torch.bfloat16)
    return gbuf[..., :C4], cell, out[..., 16:16 + C], out


@pytest.mark.parametrize("fresh", [False, True], ids=["prev", "zero"])
def test_unfused_gate_kernel_exact(fresh):
    """oess_convlstm_gates_bf16 (hip.convlstm_gates, the path of C % 32 != 0) on bf16 gates of +-128 and a previous cell in
    {0, +-40}: the same integers."""
    from openess_amd import hip
    g = cases.exact_gates(*cases.GATES_GEOM)
    C = cases.GATES_GEOM[3]
    c0 = torch.zeros_like(g['c']) if fresh else g['c']
    cell_want, hidden_want = cases.cell_update(g['gates'].to(torch.int64), c0.to(torch.int64))
    gates, cell, hidden, out = gates_problem(g, fresh)
    hip.convlstm_gates(gates, cell, hidden, prev_cell_is_zero=fresh)
    torch.cuda.synchronize()
    assert torch.equal(nchw(cell), cell_want.float()) and torch.equal(nchw(hidden), hidden_want)
    assert bool(torch.isnan(out[..., :16].float()).all()) and bool(torch.isnan(out[..., 16 + C:].float()).all())
    assert set(cell_want.unique().tolist()) == ({-1, 0, 1} if fresh else set(cases.possible_cells(1)))     # every kind of value occurs


def half_ulp_bf16(v):
    """Half a bf16 ulp (8 significand bits) of |v|, elementwise, float64."""
    return 2.0 ** (torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 8)


def assert_within_bound(tag, cell, hidden, cell64, hidden64):
    """cell: max |cell - cell64| <= CELL_BOUND; hidden: |h - h64| <= half a bf16 ulp of |h64| + CELL_BOUND, elementwise.  Prints
    the deviations first."""
    dev = float((cell.double() - cell64).abs().max())
    over = float(((hidden.double() - hidden64).abs() - half_ulp_bf16(hidden64)).max())
    print("convlstm bf16 deviation from float64", tag, "cell", dev, "hidden beyond half a bf16 ulp", over, "bound", CELL_BOUND)
    assert dev <= CELL_BOUND, (tag, dev)
    assert over <= CELL_BOUND, (tag, over)


@pytest.mark.parametrize("geom,k,fresh,route", cases.BOUND_CASES, ids=[f"{g}-{k}-{'zero' if f else 'prev'}".replace(' ', '') for g, k, f, _ in cases.BOUND_CASES])
def test_single_launch_within_float64_bound(geom, k, fresh, route):
    from openess_amd import hip
    c = cases.random_case(*geom, k)
    p, out = problem(c, k, fresh)
    assert_route(p, route)
    hip.convlstm_fused(*p)
    torch.cuda.synchronize()
    cell64, hidden64 = ref.step(c['x'], None if fresh else c['h'], None if fresh else c['c'], c['w'], c['b'])
    assert_within_bound((geom, k, fresh, route), nchw(p[3]), nchw(p[4]), cell64, hidden64)
    assert bool(torch.isnan(out[..., :geom[3]].float()).all())


@pytest.mark.parametrize("fresh", [False, True], ids=["prev", "zero"])
def test_w128_launch_within_float64_bound(fresh):
    from openess_amd import hip
    B, H, W, C = cases.W128_BOUND_GEOM
    c = cases.random_case(B, H, W, C, C, 3)
    p, out = problem(c, 3, fresh, cell=w128_cell(c, B, H, W, C, fresh))
    assert_route(p, 'HALO3X3_LSTM')
    assert hip.convlstm_w128_group([p]) is True
    torch.cuda.synchronize()
    cell64, hidden64 = ref.step(c['x'], None if fresh else c['h'], None if fresh else c['c'], c['w'], c['b'])
    assert_within_bound(('w128', cases.W128_BOUND_GEOM, fresh), nchw(w128_cell_nhwc(p[3], B, H, W, C)), nchw(p[4]), cell64, hidden64)


@pytest.mark.parametrize("fresh", [False, True], ids=["prev", "zero"])
def test_unfused_gate_kernel_within_float64_bound(fresh):
    from openess_amd import hip
    g = cases.random_gates(*cases.GATES_GEOM)
    gates, cell, hidden, out = gates_problem(g, fresh)
    hip.convlstm_gates(gates, cell, hidden, prev_cell_is_zero=fresh)
    torch.cuda.synchronize()
    cell64, hidden64 = ref.gates_kernel(g['gates'], None if fresh else g['c'])
    assert_within_bound(('gates', cases.GATES_GEOM, fresh), nchw(cell), nchw(hidden), cell64, hidden64)


def test_rejections_leave_outputs_untouched():
    """C % 32 != 0, an odd hidden pixel stride and a group of four problems raise; no output element is written."""
    from openess_amd import _lib, hip
    lib = _lib.load()
    touched = []
    # C % 32 != 0 (C = 48, Cin = 96)
    c = cases.random_case(1, 8, 8, 48, 48, 3)
    p, out = problem(c, 3, True)
    touched += [p[3], out]
    with pytest.raises(RuntimeError, match="invalid argument"):
        hip.convlstm_route(p[0], 48, 3, 1, hidden_pix_stride=p[4].stride(2))
    with pytest.raises(RuntimeError, match="oess_convlstm_fused_bf16"):
        hip.convlstm_fused(*p)
    with pytest.raises(RuntimeError, match="oess_convlstm_fused_group_bf16"):
        hip.convlstm_fused_group([p])
    # an odd hidden pixel stride
    c = cases.random_case(1, 8, 8, 32, 32, 3)
    p, _ = problem(c, 3, True)
    odd = torch.full((1, 8, 8, 33), NAN, device='cuda', dtype=torch.bfloat16)
    p = p[:4] + (odd[..., :32],) + p[5:]
    touched += [p[3], odd]
    with pytest.raises(RuntimeError, match="invalid argument"):
        hip.convlstm_route(p[0], 32, 3, 1, hidden_pix_stride=33)
    with pytest.raises(RuntimeError, match="oess_convlstm_fused_bf16"):
        hip.convlstm_fused(*p)
    # four problems: the wrappers and both entry points
    B, H, W, C = cases.W128[0]
    c = cases.random_case(B, H, W, C, C, 3)
    four = []
    for _ in range(4):
        p, out = problem(c, 3, True, cell=w128_cell(c, B, H, W, C, True))
        four.append(p)
        touched += [p[3], out]
    with pytest.raises(ValueError, match="1..3 problems"):
        hip.convlstm_fused_group(four)
    with pytest.raises(ValueError, match="1..3 problems"):
        hip.convlstm_w128_group(four)
    descs = (_lib.ConvLstmDesc * 4)()
    keep = [hip._convlstm_descs([p], "test", lambda px, C_: p[3].numel())[0] for p in four]
    for i, d in enumerate(keep):
        ctypes.memmove(ctypes.addressof(descs[i]), ctypes.addressof(d[0]), ctypes.sizeof(_lib.ConvLstmDesc))
    assert lib.oess_convlstm_w128_group_bf16(ctypes.addressof(descs), 4, None) == EINVAL
    assert lib.oess_convlstm_fused_group_bf16(ctypes.addressof(descs), 4, None) == EINVAL
    torch.cuda.synchronize()
    for t in touched:
        assert bool(torch.isnan(t.float()).all())
    assert hip.convlstm_w128_group(four[:3]) is True                                   # the same problems are taken three at a time
