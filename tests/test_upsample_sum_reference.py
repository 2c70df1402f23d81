"""CPU checks of the float64 restatement the GPU tests of K30 use (tests/upsample_sum_reference.py): it is torch's
F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) of the float64 sum, bit for bit, on every case of
tests/upsample_sum_cases.py; the exact family is exact; the bound's terms are what its docstring says."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import upsample_sum_cases as uc
from tests import upsample_sum_reference as ur


def _torch_ref(x, skip):
    s = x.double() if skip is None else x.double() + skip.double()
    up = F.interpolate(s.permute(0, 3, 1, 2).contiguous(), scale_factor=2, mode='bilinear', align_corners=False)
    return up.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("family", uc.FAMILIES)
@pytest.mark.parametrize("shape", uc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_is_torch_interpolate_of_the_float64_sum(shape, family, with_skip):
    x, skip = uc.operands(shape, family, with_skip)
    B, C, H, W = shape
    got = ur.upsample2x_sum(x.double().numpy(), None if skip is None else skip.double().numpy())
    want = _torch_ref(x, skip)
    assert got.shape == want.shape == (B, 2 * H, 2 * W, C) and got.dtype == np.float64
    assert np.array_equal(got, want)                       # bit-equal: bf16 operands and weights k / 16 are exact in float64


def test_axis_taps_are_the_documented_rule():
    i0, i1, lam = ur.axis_taps(1)
    assert i0.tolist() == [0, 0] and i1.tolist() == [0, 0]            # both taps on the only pixel
    i0, i1, lam = ur.axis_taps(4)
    assert i0.tolist() == [0, 0, 0, 1, 1, 2, 2, 3] and i1.tolist() == [1, 1, 1, 2, 2, 3, 3, 3]      # o = 7: both on the edge pixel
    assert lam.tolist() == [0.0, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0.25]   # interior weights {0.25, 0.75}, lambda 0 at o = 0


@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("shape", uc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_family_is_exact_in_bf16_and_not_vacuous(shape, with_skip):
    x, skip = uc.operands(shape, "exact", with_skip)
    ref = ur.upsample2x_sum(x.double().numpy(), None if skip is None else skip.double().numpy())
    assert np.array_equal(ref, np.rint(ref)) and np.abs(ref).max() <= 128
    assert np.array_equal(torch.from_numpy(ref).to(torch.bfloat16).double().numpy(), ref)
    if ref.size >= 64:
        assert (ref != 0).mean() >= 0.5


def test_cancelling_family_cancels_and_tap_magnitude_is_the_tap_maximum():
    shape = (2, 40, 5, 7)
    x, skip = uc.operands(shape, "large_offset_cancel", True)
    xs, ss = x.double().numpy(), skip.double().numpy()
    ref, A = ur.upsample2x_sum(xs, ss), ur.tap_magnitude(xs, ss)
    assert np.abs(ref).max() < 32 and A.min() > 1900          # |sum| of the order of a bf16 ulp at 1000, A near 2000
    # a constant operand: every tap has the same magnitude; a single spike reaches the outputs that tap it and no other
    one = np.zeros((1, 3, 3, 1))
    one[0, 1, 1, 0] = 5.0
    A = ur.tap_magnitude(one)[0, :, :, 0]
    assert A.shape == (6, 6) and (A[1:5, 1:5] == 5.0).all() and A[0].max() == 0 and A[:, 0].max() == 0 and A[5].max() == 0
    # the bound's two terms
    b = uc.bound(np.array([1.0, 0.0]), np.array([0.0, 1.0]))
    assert b.tolist() == [2.0 ** -8, 2.0 ** -20]


def test_layout_helpers_keep_the_poison():
    t, _ = uc.operands((1, 8, 1, 5), "exact", False)
    v, big = uc.place(t, "slice", "cpu")
    assert v.stride(2) == 32 and v.storage_offset() == 8 and torch.equal(v, t) and bool(torch.isnan(big[..., :8]).all())
    o, obig = uc.out_view((1, 8, 1, 5), "slice", "cpu")
    assert o.shape == (1, 2, 10, 8) and uc.neighbours_untouched(obig, "slice", 8)
    obig[0, 0, 0, 16] = 1.0
    assert not uc.neighbours_untouched(obig, "slice", 8)
