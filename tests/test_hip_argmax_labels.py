"""GPU tests of K31's kernel: oess_argmax_labels (hip.argmax_labels) against the float32 restatement of
tests/argmax_labels_reference.py -- exact, the kernel uses no FMA --, in fp32 and bf16, dense and as a channel slice of a wider
NaN-filled buffer, with and without out=; the raw-value rule at the input size, the exact tie family, the sibling check against
hip.bilinear_resize(...).argmax(1) (bit-equal labels, the LDS and the global-memory path), and every refusal of the entry and
of the wrapper."""
import numpy as np
import pytest
import torch

from tests import argmax_labels_reference as ar

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = -7
ALL_SHAPES = ar.SHAPES + [ar.GLOBAL_PATH_SHAPE]
VARIANTS = [(d, l, o) for d in ("fp32", "bf16") for l in ("dense", "slice") for o in (False, True)]


def _place(x, dtype, layout):
    """logical [B, K, h, w] device tensor of `x`: dense NCHW, or channels 8 ... 8 + K of a NaN-filled NHWC buffer of K + 24 channels"""
    x = x.to(torch.bfloat16 if dtype == "bf16" else torch.float32)
    if layout == "dense":
        return x.to(DEV)
    B, K, h, w = x.shape
    big = torch.full((B, h, w, K + 24), float('nan'), dtype=x.dtype, device=DEV)
    big[..., 8:8 + K] = x.to(DEV).permute(0, 2, 3, 1)
    return big[..., 8:8 + K].permute(0, 3, 1, 2)


def _out_size(shape, size):
    return tuple(shape[2:]) if size is None else tuple(size)


@pytest.mark.parametrize("dtype,layout,with_out", VARIANTS, ids=["-".join((d, l, "out" if o else "new")) for d, l, o in VARIANTS])
@pytest.mark.parametrize("shape,size,align", ar.SHAPES, ids=[ar.case_id(*c) for c in ar.SHAPES])
def test_kernel_equals_the_float32_restatement(shape, size, align, dtype, layout, with_out):
    from openess_amd import hip
    x = ar.randn_logits(shape, seed=sum(shape))
    xv = _place(x, dtype, layout)
    want = ar.argmax_labels(xv.float().cpu().numpy(), size, align)
    H, W = _out_size(shape, size)
    out = torch.full((shape[0], H, W), POISON, dtype=torch.int64, device=DEV) if with_out else None
    y = hip.argmax_labels(xv, size=size, align_corners=align, out=out)
    assert y.shape == (shape[0], H, W) and y.dtype == torch.int64 and y.is_contiguous()
    if with_out:
        assert y.data_ptr() == out.data_ptr()
    bad = int((y.cpu().numpy() != want).sum())
    assert bad == 0, f"{bad} of {want.size} labels differ"


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_input_size_compares_the_raw_values(dtype):
    """+-inf, NaN and ties at the input size: no blend, so no 0 * inf; torch.argmax's rule"""
    from openess_amd import hip
    x, planted = ar.special_logits()
    xv = _place(x, dtype, "slice")
    want = ar.argmax_labels(xv.float().cpu().numpy())
    for size in (None, (4, 6)):
        y = hip.argmax_labels(xv, size=size)
        assert np.array_equal(y.cpu().numpy(), want) and torch.equal(y, xv.argmax(1))
        assert all(int(y[p]) == k for p, k in planted.items())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape,scale", ar.EXACT_CASES, ids=[f"{'x'.join(map(str, s))}-x{k}" for s, k in ar.EXACT_CASES])
def test_exact_tie_family(shape, scale, dtype):
    """integer logits at power-of-two upsampling: the float64 labels, everywhere, 7 % of the pixels being exact ties"""
    from openess_amd import hip
    x = ar.exact_logits(shape)
    size = (shape[2] * scale, shape[3] * scale)
    v64 = ar.float64_upsampled(x.numpy(), size, False)
    y = hip.argmax_labels(_place(x, dtype, "dense"), size=size).cpu().numpy()
    assert np.array_equal(y, np.argmax(v64, axis=1)) and np.array_equal(y, ar.argmax_labels(x.numpy(), size))


def test_all_equal_logits_give_label_zero():
    from openess_amd import hip
    for value in (0.0, -3.5, float('inf'), float('nan')):
        x = torch.full((2, 19, 5, 7), value, device=DEV)
        assert not hip.argmax_labels(x).any()
        if np.isfinite(value):                               # (inf - inf in a blend is NaN: still all equal, still 0)
            assert not hip.argmax_labels(x, size=(20, 21)).any()
    assert not hip.argmax_labels(torch.full((1, 4, 3, 3), float('inf'), device=DEV), size=(9, 9)).any()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape,size,align", ALL_SHAPES, ids=[ar.case_id(*c) for c in ALL_SHAPES])
def test_labels_equal_the_composed_path_bit_for_bit(shape, size, align, dtype):
    """the sibling: resize_fwd_kernel's values, argmax-ed by torch.  The last shape reads its taps from global memory (two source
    rows of 25 x 256 fp32 exceed the kernel's 48 KB of LDS)."""
    from openess_amd import hip
    x = _place(ar.randn_logits(shape, seed=1 + sum(shape)), dtype, "dense")
    size = _out_size(shape, size)
    got = hip.argmax_labels(x, size, align)
    full = hip.bilinear_resize(x.float(), size=size, align_corners=align)
    assert torch.equal(got, full.argmax(1))
    assert np.array_equal(got.cpu().numpy(), ar.argmax_labels(x.float().cpu().numpy(), size, align))


def test_non_finite_taps_blend_as_the_composed_path_blends_them():
    from openess_amd import hip
    x = ar.randn_logits((2, 11, 3, 4), seed=5)
    x[0, 2, 1, 1], x[1, 7, 0, 3], x[1, 4, 2, 0] = float('nan'), float('inf'), float('-inf')
    x = x.to(DEV)
    got = hip.argmax_labels(x, (12, 16))
    assert torch.equal(got, hip.bilinear_resize(x, size=(12, 16)).argmax(1))
    assert np.array_equal(got.cpu().numpy(), ar.argmax_labels(x.cpu().numpy(), (12, 16)))


# ------------------------------------------------------------------------------------------------------------------- refusals
def _entry_args(B=2, K=5, h=3, w=4, H=6, W=8):
    from openess_amd import hip
    x = torch.randn(B, h, w, K + 3, device=DEV)
    out = torch.full((B, H, W), POISON, dtype=torch.int64, device=DEV)
    return x, out, dict(logits=x.data_ptr(), is_bf16=0, ps=K + 3, B=B, K=K, h=h, w=w, H=H, W=W, ac=0, out=out.data_ptr(),
                        stream=hip._stream())


def _call(a):
    from openess_amd import _lib
    return _lib.load().oess_argmax_labels(a['logits'], a['is_bf16'], a['ps'], a['B'], a['K'], a['h'], a['w'], a['H'], a['W'], a['ac'],
                                          a['out'], a['stream'])


ENTRY_REFUSALS = {
    "null_logits": dict(logits=None),
    "null_out": dict(out=None),
    "k_zero": dict(K=0),
    "k_negative": dict(K=-1),
    "k_257": dict(K=257, ps=300),
    "b_zero": dict(B=0),
    "h_in_negative": dict(h=-1),
    "w_in_zero": dict(w=0),
    "h_out_zero": dict(H=0),
    "w_out_negative": dict(W=-3),
    "stride_below_k": dict(ps=4),
    "stride_zero": dict(ps=0),
    "output_rows_overflow": dict(B=1 << 16, H=1 << 16),                # B * H = 2^32 workgroups
    "input_rows_overflow": dict(B=1 << 16, h=1 << 16, H=1),
    "input_extent_overflows": dict(ps=1 << 62),                        # B * h * w * stride beyond int64
    "output_extent_overflows": dict(B=1 << 15, H=1 << 15, W=(1 << 31) - 1),     # 2^61 labels of 8 bytes
}


@pytest.mark.parametrize("name", sorted(ENTRY_REFUSALS))
def test_entry_refuses_before_any_launch(name):
    x, out, a = _entry_args()
    assert _call(a) == 0                                              # the unmodified call is valid
    torch.cuda.synchronize()
    want = ar.argmax_labels(x[..., :5].permute(0, 3, 1, 2).cpu().numpy(), (6, 8), False)
    assert np.array_equal(out.cpu().numpy(), want)
    out.fill_(POISON)
    assert _call(dict(a, **ENTRY_REFUSALS[name])) == -22
    torch.cuda.synchronize()
    assert bool((out == POISON).all())


def test_wrapper_refuses_before_any_launch():
    from openess_amd import hip
    x = torch.randn(2, 5, 3, 4, device=DEV)
    out = torch.full((2, 6, 8), POISON, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="no CPU fallback"):
        hip.argmax_labels(x.cpu(), (6, 8), out=out)
    with pytest.raises(ValueError, match="float32 / bfloat16"):
        hip.argmax_labels(x.half(), (6, 8), out=out)
    with pytest.raises(ValueError, match="float32 / bfloat16"):
        hip.argmax_labels(x.double(), (6, 8), out=out)
    with pytest.raises(ValueError, match="4-D"):
        hip.argmax_labels(x[0], (6, 8), out=out)
    with pytest.raises(ValueError, match="K <= 256"):
        hip.argmax_labels(torch.zeros(1, 257, 2, 2, device=DEV), (6, 8))
    with pytest.raises(ValueError, match="K <= 256"):
        hip.argmax_labels(torch.zeros(1, 0, 2, 2, device=DEV))
    for bad in (out[:, :5], out[:1], out.int(), out.cpu(), out.float(), out.view(2, 8, 6).transpose(1, 2), out.view(1, 2, 6, 8)):
        with pytest.raises(ValueError, match="out must be"):
            hip.argmax_labels(x, (6, 8), out=bad)
    with pytest.raises(ValueError, match="out must be"):
        hip.argmax_labels(x, out=out)                                  # size=None is the input size, 3 x 4
    torch.cuda.synchronize()
    assert bool((out == POISON).all())
    assert hip.argmax_labels(x.requires_grad_(True), (6, 8)).requires_grad is False
