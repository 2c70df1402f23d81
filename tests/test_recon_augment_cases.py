"""CPU checks of the K27 yardstick (tests/recon_augment_reference.py): the float64 restatement is the reference's host code
(`_io.adjust_brightness` / `_io.adjust_contrast` / `torch.flip` on u8 / 255), its Philox is Philox-4x32-10, its uniforms stay in
(0, 1], and the grey levels' fp32 form is the PNG path's."""
import numpy as np
import pytest
import torch

from openess_amd.datasets import _io
from tests import recon_augment_cases as cases
from tests import recon_augment_reference as ref


def _host(u8, flip, brightness, contrast):
    """sequence_ov.py:204-221 in float64 through the project's own helpers, one sample."""
    x = torch.from_numpy(u8.astype(np.float64) / 255.0)[None].repeat(3, 1, 1)
    if flip:
        x = torch.flip(x, [2])
    if brightness is not None:
        x = _io.adjust_brightness(x, brightness)
    if contrast is not None:
        x = _io.adjust_contrast(x, contrast)
    return x.numpy()


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_restatement_equals_the_host_augmentation_in_float64(shape):
    u8 = cases.grey(shape)
    f32 = lambda v: float(np.float32(v))           # the restatement takes the fp32 factor the kernel receives
    rows = [(0, None, None), (1, None, None), (0, 0.5, None), (0, 2.0, None), (0, 0.83, None), (0, None, 0.8), (0, None, 1.2),
            (0, None, 0.0), (0, None, 2.0), (1, 1.19, 0.81)]
    for flip, bri, con in rows:
        for b in range(cases.B):
            got = ref.augment_sample(u8[b], flip, 1.0 if bri is None else bri, 1.0 if con is None else con, 0)
            want = _host(u8[b], flip, None if bri is None else f32(bri), None if con is None else f32(con))
            assert got.shape == want.shape == (3,) + shape
            assert np.abs(got - want).max() <= 1e-12, (shape, flip, bri, con, b)


def test_uniform_mapping_stays_inside_the_half_open_unit_interval():
    u = ref.unit24(np.array([0, 1, 255, 256, 0x7FFFFFFF, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint64))
    assert u[0] == 2.0 ** -24 and u[-1] == 1.0
    assert (u > 0).all() and (u <= 1).all()
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)          # exact in fp32: the kernel's uniforms are these
    assert np.isfinite(np.log(u)).all()


def test_grey_levels_in_fp32_are_the_png_paths():
    """k / 255 by IEEE fp32 division (the kernel's form) is np.float32(k / 255.0) (image_to_chw_float: float64 division, then one
    rounding) for all 256 levels.  The product with the rounded reciprocal, K13's float output, is NOT: it differs in the last
    bit on 126 levels, which is why the kernel divides."""
    k = np.arange(256)
    want = (k / 255.0).astype(np.float32)
    assert np.array_equal(k.astype(np.float32) / np.float32(255.0), want)
    assert np.array_equal((torch.arange(256, dtype=torch.float32) / 255.0).numpy(), want)
    recip = k.astype(np.float32) * np.float32(1.0 / 255.0)
    assert int((recip != want).sum()) == 126 and np.abs(recip.astype(np.float64) - want).max() <= 2.0 ** -24
    assert np.array_equal(np.round(recip.astype(np.float64) * 255.0), k)       # the same grey level either way


def test_philox_known_answers():
    """Random123's known-answer vectors of philox4x32_10."""
    def run(c, k):
        return [int(v[0]) for v in ref.philox4x32_10([np.array([x], dtype=np.uint64) for x in c], k)]
    assert run((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert run((0xffffffff,) * 4, (0xffffffff, 0xffffffff)) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert run((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_noise_restatement_is_standard_normal_and_seeded():
    n = ref.sample_noise(cases.SEEDS[0], (3,) + cases.STATS_SHAPE)
    cnt = n.size
    assert abs(n.mean()) <= 5 / np.sqrt(cnt) and abs(n.std() - 1) <= 5 / np.sqrt(2 * cnt)
    assert np.array_equal(n, ref.sample_noise(cases.SEEDS[0], (3,) + cases.STATS_SHAPE))
    assert not np.array_equal(n, ref.sample_noise(cases.SEEDS[1], (3,) + cases.STATS_SHAPE))
    assert not ref.sample_noise(0, (3, 5, 7)).any()
