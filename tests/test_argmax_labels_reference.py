"""The float32 restatement of oess_argmax_labels' contract (tests/argmax_labels_reference.py) pinned against torch's float64
interpolation, without a GPU: (a) an exact family -- integer logits at power-of-two upsampling, where every product and sum is exact
in float32, so the labels must equal the float64 labels everywhere, exact ties included --, and (b) randn logits, where the labels
must equal the float64 labels at every pixel whose float64 top-2 margin exceeds the float32 error of the blend.

The margin of (b): the blend is 4 products, 2 + 1 sums and 2 outer products of values bounded by M = max_k |value| with weights in
[0, 1] that carry the index rule's float32 rounding (a few 2^-24 relative of a source coordinate <= 2^6 here, i.e. <= 2^-18 absolute
on a weight); 4 * 2^-20 * M covers both values of the pair with room to spare.  The share of pixels below the margin is a condition
(<= 1e-3), not a measurement: torch's own float32 CPU interpolation has 6.6e-5, 0, 1.8e-5 and 0 on the four cases below and disagrees
with float64 at no pixel above the margin."""
import numpy as np
import pytest
import torch

from tests import argmax_labels_reference as ar


@pytest.mark.parametrize("shape,scale", ar.EXACT_CASES, ids=[f"{'x'.join(map(str, s))}-x{k}" for s, k in ar.EXACT_CASES])
def test_exact_family_equals_float64_everywhere(shape, scale):
    x = ar.exact_logits(shape).numpy()
    size = (shape[2] * scale, shape[3] * scale)
    v32 = ar.upsampled(x, size, False)
    v64 = ar.float64_upsampled(x, size, False)
    assert np.array_equal(v32.astype(np.float64), v64)                    # exact values, not only exact labels
    want = torch.from_numpy(v64).argmax(1).numpy()
    got = ar.argmax_labels(x, size, False)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    margin, _ = ar.top2_margin(v64)
    ties = float((margin == 0).mean())
    print(f"exact family {shape} x{scale}: {ties:.3%} of the pixels are exact ties")
    assert 0.05 <= ties <= 0.11                                           # the first-index rule is exercised
    tied = margin == 0
    assert np.array_equal(got[tied], np.argmax(v64, axis=1)[tied])


@pytest.mark.parametrize("shape,size,align", ar.CAP_CASES, ids=[ar.case_id(*c) for c in ar.CAP_CASES])
def test_randn_labels_equal_float64_above_the_margin(shape, size, align):
    x = ar.randn_logits(shape, seed=0).numpy()
    v64 = ar.float64_upsampled(x, size, align)
    margin, peak = ar.top2_margin(v64)
    clear = margin > 4 * 2.0 ** -20 * peak
    share = 1.0 - float(clear.mean())
    got = ar.argmax_labels(x, size, align)
    want = np.argmax(v64, axis=1)
    bad = int((got != want)[clear].sum())
    print(f"{ar.case_id(shape, size, align)}: share below the margin {share:.2e}, disagreements above it {bad}, below it "
          f"{int((got != want)[~clear].sum())}")
    assert share <= 1e-3
    assert bad == 0


def test_same_size_is_the_raw_argmax_with_torchs_tie_and_nan_rule():
    x, planted = ar.special_logits()
    got = ar.argmax_labels(x.numpy())
    assert np.array_equal(got, x.argmax(1).numpy())
    assert all(got[p] == k for p, k in planted.items())
    assert np.array_equal(ar.argmax_labels(x.numpy(), (4, 6)), got)       # size == input size is the same path
    assert not ar.argmax_labels(np.zeros((1, 7, 3, 3), np.float32), (5, 9)).any()


def test_index_rule_matches_the_float64_rule_on_the_cases():
    """taps of the float32 rule against the rule evaluated in float64: same taps, weights within the rounding of the source coordinate"""
    for shape, size, align in ar.SHAPES + ar.CAP_CASES + [ar.GLOBAL_PATH_SHAPE]:
        if size is None:
            continue
        for n_in, n_out in ((shape[2], size[0]), (shape[3], size[1])):
            i0, i1, lam = ar.src_index(n_in, n_out, align)
            dst = np.arange(n_out, dtype=np.float64)
            s = dst * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0) if align else np.maximum((dst + 0.5) * n_in / n_out - 0.5, 0.0)
            assert i0.min() >= 0 and i1.max() <= n_in - 1 and ((i1 == i0) | (i1 == i0 + 1)).all()
            # coordinates below 64: three float32 roundings of at most 2^-19 each and the scale's 2^-24 relative error
            assert s.max() < 64 and np.abs((i0 + lam.astype(np.float64)) - s).max() <= 2.0 ** -16, (n_in, n_out, align)
