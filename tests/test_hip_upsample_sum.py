"""GPU tests of K30's kernel and layer: oess_upsample_bilinear2x_sum_nhwc_bf16 (hip.upsample2x_sum_nhwc) against the float64
restatement of tests/upsample_sum_reference.py on the cases of tests/upsample_sum_cases.py -- bit for bit on the exact family,
within the derived bound on the others, dense and as channel slices of wider poisoned buffers --, every refusal of the entry
and of the wrapper, and UpsampleConvLayer.forward against torch on the same bf16 operands."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import upsample_sum_cases as uc
from tests import upsample_sum_reference as ur

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = [(s, k, l) for s in uc.SHAPES for k in (False, True) for l in uc.LAYOUTS]


def _f64(t):
    return None if t is None else t.double().numpy()


@pytest.mark.parametrize("shape,with_skip,layout", CASES, ids=[uc.case_id(*c) for c in CASES])
def test_kernel_against_float64(shape, with_skip, layout):
    from openess_amd import hip
    B, C, H, W = shape
    for family in uc.FAMILIES:
        x, skip = uc.operands(shape, family, with_skip)
        ref = ur.upsample2x_sum(_f64(x), _f64(skip))
        xv, _ = uc.place(x, layout, DEV)
        sv = uc.place(skip, layout, DEV)[0] if with_skip else None
        if layout == "dense":
            out, big = None, None
        else:
            out, big = uc.out_view(shape, layout, DEV)
        y = hip.upsample2x_sum_nhwc(xv, sv, out=out)
        assert y.shape == (B, 2 * H, 2 * W, C) and y.dtype == torch.bfloat16
        if out is not None:
            assert y.data_ptr() == out.data_ptr() and uc.neighbours_untouched(big, layout, C), family
        got = y.cpu().double().numpy()
        if family == "exact":
            bad = int((got != ref).sum())
            assert bad == 0, f"{family}: {bad} of {ref.size} outputs differ"
        else:
            A = ur.tap_magnitude(_f64(x), _f64(skip))
            excess = np.abs(got - ref) - uc.bound(ref, A)
            print(f"{uc.case_id(shape, with_skip, layout)} {family}: max |out - ref| = {np.abs(got - ref).max():.3e}, "
                  f"largest share of the bound used = {(np.abs(got - ref) / np.maximum(uc.bound(ref, A), 1e-300)).max():.3f}")
            assert np.isfinite(got).all() and excess.max() <= 0, f"{family}: over the bound by {excess.max():.3e}"


def test_default_output_is_dense_and_the_inputs_are_left_alone():
    from openess_amd import hip
    x, skip = uc.operands((2, 40, 5, 7), "randn", True)
    xv, sv = x.to(DEV), skip.to(DEV)
    y = hip.upsample2x_sum_nhwc(xv, sv)
    assert y.is_contiguous() and y.shape == (2, 10, 14, 40)
    assert torch.equal(xv.cpu(), x) and torch.equal(sv.cpu(), skip)
    # a logical-NCHW channels_last tensor and a channel slice of a state buffer, as the decoder passes them (engine.nhwc)
    from openess_amd import engine
    xc = xv.permute(0, 3, 1, 2)
    wide = torch.zeros(2, 5, 7, 80, dtype=torch.bfloat16, device=DEV)
    wide[..., 40:] = sv
    y2 = hip.upsample2x_sum_nhwc(engine.nhwc(xc), engine.nhwc(engine.from_nhwc(wide)[:, 40:]))
    assert torch.equal(y2, y)


def _entry_args(B=1, H=3, W=5, C=16):
    """Device buffers large enough for every variation below, plus the argument list of a valid call."""
    from openess_amd import hip
    x = torch.ones(B, H, W, 2 * C, dtype=torch.bfloat16, device=DEV)
    skip = torch.ones(B, H, W, 2 * C, dtype=torch.bfloat16, device=DEV)
    out = torch.full((B, 2 * H, 2 * W, 2 * C), uc.POISON_OUT, dtype=torch.bfloat16, device=DEV)
    st = hip._stream()
    return x, skip, out, dict(x=x.data_ptr(), xps=2 * C, skip=skip.data_ptr(), sps=2 * C, B=B, H=H, W=W, C=C, out=out.data_ptr(),
                              ops=2 * C, stream=st)


def _call(a):
    from openess_amd import _lib
    return _lib.load().oess_upsample_bilinear2x_sum_nhwc_bf16(a['x'], a['xps'], a['skip'], a['sps'], a['B'], a['H'], a['W'], a['C'],
                                                              a['out'], a['ops'], a['stream'])


ENTRY_REFUSALS = {
    "c_not_multiple_of_8": dict(C=12),
    "c_zero": dict(C=0),
    "b_zero": dict(B=0),
    "h_negative": dict(H=-1),
    "w_zero": dict(W=0),
    "x_stride_below_c": dict(xps=8),
    "x_stride_no_whole_vectors": dict(xps=20),
    "skip_stride_below_c": dict(sps=8),
    "out_stride_below_c": dict(ops=8),
    "null_x": dict(x=None),
    "null_out": dict(out=None),
    "out_is_x": "alias_x",
    "out_is_skip": "alias_skip",
    "out_inside_x_range": "alias_x_offset",
}


@pytest.mark.parametrize("name", sorted(ENTRY_REFUSALS))
def test_entry_refuses_before_any_launch(name):
    x, skip, out, a = _entry_args()
    assert _call(a) == 0                                     # the unmodified call is valid (and fills its half of `out`)
    torch.cuda.synchronize()
    assert bool((out[..., :16] != uc.POISON_OUT).all()) and bool((out[..., 16:] == uc.POISON_OUT).all())
    out.fill_(uc.POISON_OUT)
    change = ENTRY_REFUSALS[name]
    if change == "alias_x":
        change = dict(out=a['x'])
    elif change == "alias_skip":
        change = dict(out=a['skip'])
    elif change == "alias_x_offset":
        change = dict(out=a['x'] + 32)                       # the other channel half of x's buffer: inside x's byte range
    keep = (x.clone(), skip.clone())
    assert _call(dict(a, **change)) == -22
    torch.cuda.synchronize()
    assert bool((out == uc.POISON_OUT).all()) and torch.equal(x, keep[0]) and torch.equal(skip, keep[1])


def test_null_skip_is_no_refusal():
    x, _, out, a = _entry_args()
    assert _call(dict(a, skip=None, sps=0)) == 0
    torch.cuda.synchronize()
    assert bool((out[..., :16] == 1.0).all()) and bool((out[..., 16:] == uc.POISON_OUT).all())


def test_wrapper_refuses_before_any_launch():
    from openess_amd import hip
    x = torch.ones(1, 3, 5, 16, dtype=torch.bfloat16, device=DEV)
    out = torch.full((1, 6, 10, 16), uc.POISON_OUT, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.upsample2x_sum_nhwc(x.cpu(), out=out)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.upsample2x_sum_nhwc(x, x.cpu(), out=out)
    with pytest.raises(ValueError, match="bf16"):
        hip.upsample2x_sum_nhwc(x.float(), out=out)
    with pytest.raises(ValueError, match="bf16"):
        hip.upsample2x_sum_nhwc(x, x.half(), out=out)
    with pytest.raises(ValueError, match="skip has shape"):
        hip.upsample2x_sum_nhwc(x, x[:, :, :4], out=out)
    with pytest.raises(ValueError, match="multiple of 8"):
        hip.upsample2x_sum_nhwc(x[..., :12], out=out[..., :12])
    with pytest.raises(ValueError, match="out must be"):
        hip.upsample2x_sum_nhwc(x, out=out[:, :5])
    with pytest.raises(ValueError, match="out must be"):
        hip.upsample2x_sum_nhwc(x, out=torch.zeros(1, 6, 10, 16, device=DEV))
    torch.cuda.synchronize()
    assert bool((out == uc.POISON_OUT).all())
    # the entry's own refusal reaches the caller: an `out` of the right shape and dtype laid over x's memory
    big = torch.full((1, 6, 10, 16), 3.0, dtype=torch.bfloat16, device=DEV)
    xa = big.view(-1)[:3 * 5 * 16].view(1, 3, 5, 16)
    with pytest.raises(RuntimeError, match="invalid argument"):
        hip.upsample2x_sum_nhwc(xa, out=big)
    with pytest.raises(RuntimeError, match="invalid argument"):
        hip.upsample2x_sum_nhwc(x, xa, out=big)
    torch.cuda.synchronize()
    assert bool((big == 3.0).all())


# ------------------------------------------------------------------------------------------------------------------- the layer
def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


@pytest.mark.parametrize("cin,cout,norm", [(256, 128, 'BN'), (64, 32, None)])
def test_layer_matches_torch_on_the_same_bf16_operands(cin, cout, norm):
    from openess_amd.e2vid.model.submodules import UpsampleConvLayer
    from tests.synth import fill_by_name
    layer = UpsampleConvLayer(cin, cout, 5, padding=2, norm=norm).eval()
    fill_by_name(layer, 30 + cin)
    layer.cuda()
    g = torch.Generator().manual_seed(cin)
    x, skip = (torch.randn(2, cin, 7, 9, generator=g).cuda().bfloat16().contiguous(memory_format=torch.channels_last) for _ in range(2))
    with torch.no_grad():
        y = layer(x, skip=skip)
        c, bn = layer.conv2d, layer.bn
        up = F.interpolate(x.float() + skip.float(), scale_factor=2, mode='bilinear', align_corners=False)
        want = F.conv2d(up, c.weight.bfloat16().float(), c.bias, 1, 2)
        if bn is not None:
            want = F.batch_norm(want, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
        want = torch.relu(want)
        y1 = layer(x)                                         # no skip: the layer as the reference calls it
        want1 = F.conv2d(F.interpolate(x.float(), scale_factor=2, mode='bilinear', align_corners=False), c.weight.bfloat16().float(),
                         c.bias, 1, 2)
        if bn is not None:
            want1 = F.batch_norm(want1, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
        want1 = torch.relu(want1)
    assert y.shape == want.shape == (2, cout, 14, 18) and y.dtype == torch.bfloat16
    e, e1 = relerr(y.float().cpu().numpy(), want.cpu().numpy()), relerr(y1.float().cpu().numpy(), want1.cpu().numpy())
    print(f"UpsampleConvLayer({cin}, {cout}, norm={norm}): relerr {e:.3e} with skip, {e1:.3e} without")
    assert e < 2e-2 and e1 < 2e-2


def test_layer_refuses_what_check_runs_refuses():
    from openess_amd.e2vid.model.submodules import UpsampleConvLayer
    x = torch.zeros(1, 64, 3, 4, dtype=torch.bfloat16, device=DEV).contiguous(memory_format=torch.channels_last)
    train_bn = UpsampleConvLayer(64, 32, 5, padding=2, norm='BN').cuda().train()
    with pytest.raises(RuntimeError, match="eval mode"):
        train_bn(x, skip=x)
    sig = UpsampleConvLayer(64, 32, 5, padding=2, activation='sigmoid').cuda().eval()
    with pytest.raises(NotImplementedError, match="relu / None"):
        sig(x, skip=x)
    inorm = UpsampleConvLayer(64, 32, 5, padding=2, norm='IN').cuda().eval()
    with pytest.raises(NotImplementedError, match="norm='IN'"):
        inorm(x)
