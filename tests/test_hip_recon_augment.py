"""GPU tests of hip.recon_augment (K27, openess_amd/csrc/recon_augment.hip): grey levels -> the augmented three-channel student image.
Exact rows where fp32 arithmetic is exact, the float64 restatement (tests/recon_augment_reference.py) under bounds measured on
the CPU (tools/exp_recon_augment_bounds.py) where it is not, the noise against the restated Philox integers and against the
normal distribution, seeding, repeatability, streams, and the argument checks."""
import numpy as np
import pytest
import torch

from tests import recon_augment_cases as cases
from tests import recon_augment_reference as ref

pytestmark = pytest.mark.gpu

# max |torch fp32 on the CPU - float64 restatement| over the contrast / combined rows, per shape, and max |NumPy fp32 - float64| of
# the normal transform on the noise row's own integers (tools/exp_recon_augment_bounds.py); the kernel is allowed four times each
CONTRAST_FP32_ERR = {(5, 7): 8.0516e-08, (37, 53): 8.7945e-08, (64, 96): 1.01024e-07, (130, 257): 9.6210e-08}
NORMAL_FP32_ERR = {(5, 7): 7.3792e-07, (37, 53): 1.20090e-06, (64, 96): 1.40032e-06, (130, 257): 1.40032e-06}


@pytest.fixture(scope="module")
def inputs():
    """Per shape: the uint8 case on the host and on the device, made once and never written."""
    return {shape: (cases.grey(shape), torch.from_numpy(cases.grey(shape)).cuda()) for shape in cases.SHAPES}


def run(dev, c, **kw):
    from openess_amd import hip
    return hip.recon_augment(dev, c['flip'], c['brightness'], c['contrast'], c['noise_seed'], **kw)


def base_f32(u8):
    """u8 / 255 in fp32 on three channels, the PNG path's bits (np.float32(k / 255.0))."""
    return np.repeat((u8 / 255.0).astype(np.float32)[:, None], 3, axis=1)


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_all_off_is_the_grey_level_over_255(shape, inputs):
    u8, dev = inputs[shape]
    out = run(dev, cases.OFF)
    assert out.shape == (cases.B, 3) + shape and out.dtype == torch.float32 and out.is_contiguous()
    assert np.array_equal(out.cpu().numpy(), base_f32(u8))


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_flip_only_mirrors_the_bits_per_sample(shape, inputs):
    u8, dev = inputs[shape]
    for flips in ([1, 0, 1], [0, 1, 0], [1, 1, 1]):
        want = base_f32(u8)
        for b, f in enumerate(flips):
            if f:
                want[b] = want[b, :, :, ::-1]
        assert np.array_equal(run(dev, cases.case(flip=flips)).cpu().numpy(), want), flips


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_brightness_exact_products(shape, inputs):
    """0.5 and 2.0 are exact products, 1.0 is the identity; 2.0 reaches the clamp at 1."""
    u8, dev = inputs[shape]
    for factors in ([0.5, 1.0, 2.0], [2.0, 0.5, 1.0]):
        want = base_f32(u8)
        for b, f in enumerate(factors):
            want[b] = np.clip(np.float32(f) * want[b], np.float32(0), np.float32(1))
        got = run(dev, cases.case(brightness=factors)).cpu().numpy()
        assert np.array_equal(got, want), factors
        assert (got == 1.0).any() and got.dtype == np.float32


@pytest.mark.parametrize("name", sorted(cases.CONTRAST_CASES))
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_contrast_and_combined_rows_match_float64(shape, name, inputs):
    u8, dev = inputs[shape]
    c = cases.CONTRAST_CASES[name]
    want = ref.augment(u8, c['flip'], c['brightness'], c['contrast'], c['noise_seed'])
    got = run(dev, c).cpu().numpy().astype(np.float64)
    err = float(np.abs(got - want).max())
    print(f"recon_augment {name} {shape}: max |kernel - float64| = {err:.3e} (bound {4 * CONTRAST_FP32_ERR[shape]:.3e})")
    assert err <= 4 * CONTRAST_FP32_ERR[shape]
    assert got.min() >= 0.0 and got.max() <= 1.0
    # a sample whose factor is exactly 1 went through no blend: the bits of the brightness step alone
    for b in range(cases.B):
        if c['contrast'][b] == 1.0 and c['brightness'][b] == 1.0:
            want_b = base_f32(u8)[b]
            assert np.array_equal(got[b].astype(np.float32), want_b[:, :, ::-1] if c['flip'][b] else want_b)


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_noise_matches_the_restated_philox_integers(shape, inputs):
    u8, dev = inputs[shape]
    c = cases.NOISE_CASE
    pre = run(dev, dict(c, noise_seed=[0, 0, 0])).cpu().numpy().astype(np.float64)
    out = run(dev, c).cpu().numpy()
    assert np.isfinite(out).all()
    bound = 4 * NORMAL_FP32_ERR[shape] * 0.05
    for b, seed in enumerate(c['noise_seed']):
        want = 0.05 * ref.sample_noise(seed, (3,) + shape)
        err = float(np.abs((out[b].astype(np.float64) - pre[b]) - want).max())
        print(f"recon_augment noise {shape} sample {b}: max |kernel - float64| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (b, err)


def test_noise_statistics(inputs):
    """Five standard errors on n = 3 * 130 * 257 values: mean, standard deviation, and the correlation of any two channels."""
    u8, dev = inputs[cases.STATS_SHAPE]
    c = cases.case(noise_seed=list(cases.SEEDS))
    pre = run(dev, cases.OFF).cpu().numpy().astype(np.float64)
    out = run(dev, c).cpu().numpy().astype(np.float64)
    n = 3 * cases.STATS_SHAPE[0] * cases.STATS_SHAPE[1]
    for b in range(cases.B):
        z = (out[b] - pre[b]) / 0.05
        assert abs(z.mean()) <= 5 / np.sqrt(n), (b, z.mean())
        assert abs(z.std() - 1) <= 5 / np.sqrt(2 * n), (b, z.std())
        for i, j in ((0, 1), (0, 2), (1, 2)):
            r = np.corrcoef(z[i].ravel(), z[j].ravel())[0, 1]
            assert abs(r) <= 5 / np.sqrt(n / 3), (b, i, j, r)


@pytest.mark.parametrize("shape", [(37, 53), (130, 257)])
def test_noise_seeding(shape, inputs):
    from openess_amd import hip
    u8, dev = inputs[shape]
    s0, s1, s2 = cases.SEEDS
    full = dict(flip=[0, 1, 0], brightness=[1.0, 0.9, 1.1], contrast=[0.9, 1.1, 1.0])
    a = run(dev, cases.case(noise_seed=[s0, s1, s2], **full))
    assert torch.equal(a, run(dev, cases.case(noise_seed=[s0, s1, s2], **full)))          # same seeds, same bits
    other = run(dev, cases.case(noise_seed=[s1, s1, 0], **full))
    assert not torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])                 # another seed, other values
    assert torch.equal(other[2], run(dev, cases.case(**full))[2])                          # seed 0: no noise
    # a sample's result depends on neither its batch index nor B: sample 1 alone, and as sample 4 of a batch of 5
    alone = hip.recon_augment(dev[1:2].contiguous(), [1], [0.9], [1.1], [s1])
    assert torch.equal(alone[0], a[1])
    five = torch.cat([dev[2:3], dev[0:1], dev[2:3], dev[0:1], dev[1:2]]).contiguous()
    out5 = hip.recon_augment(five, [0, 0, 1, 1, 1], [1.1, 1.0, 0.7, 1.0, 0.9], [1.0, 0.9, 1.3, 1.0, 1.1], [s2, s0, 5, 0, s1])
    assert torch.equal(out5[4], a[1]) and torch.equal(out5[1], a[0]) and torch.equal(out5[0], a[2])


def test_batches_beyond_one_launch_chunk(inputs):
    """B = 70 samples cross the 32-sample launch chunk twice; every sample equals its single-sample call."""
    from openess_amd import hip
    u8, dev = inputs[(37, 53)]
    idx = [i % cases.B for i in range(70)]
    big = dev[idx].contiguous()
    flip = [i & 1 for i in range(70)]
    bri = [0.8 + 0.005 * i for i in range(70)]
    con = [1.0 if i % 3 == 0 else 0.8 + 0.005 * i for i in range(70)]
    seed = [0 if i % 4 == 0 else 1000 + i for i in range(70)]
    out = hip.recon_augment(big, flip, bri, con, seed)
    for i in (0, 31, 32, 33, 63, 64, 69):
        one = hip.recon_augment(big[i:i + 1].contiguous(), [flip[i]], [bri[i]], [con[i]], [seed[i]])
        assert torch.equal(out[i], one[0]), i


@pytest.mark.parametrize("shape", [(64, 96), (130, 257)])
def test_repeatable_and_stream_independent(shape, inputs):
    u8, dev = inputs[shape]
    c = dict(cases.NOISE_CASE, contrast=[0.85, 1.1, 1.0])
    a = run(dev, c)
    b = run(dev, c, out=torch.full_like(a, float('nan')))
    assert torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = run(dev, c)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(a, s)


def test_argument_checks_raise_before_any_launch(inputs):
    from openess_amd import hip
    u8, dev = inputs[(5, 7)]
    ok = (cases.OFF['flip'], cases.OFF['brightness'], cases.OFF['contrast'], cases.OFF['noise_seed'])
    with pytest.raises(ValueError):
        hip.recon_augment(dev.float(), *ok)                                       # wrong dtype
    with pytest.raises(ValueError):
        hip.recon_augment(torch.from_numpy(u8), *ok)                              # a CPU tensor
    with pytest.raises(ValueError):
        hip.recon_augment(dev[0], *ok)                                            # not [B, H, W]
    with pytest.raises(ValueError):
        hip.recon_augment(dev[:, :, ::2], *ok)                                    # not contiguous
    for k in range(4):
        bad = [list(v) for v in ok]
        bad[k] = bad[k][:2]
        with pytest.raises(ValueError):
            hip.recon_augment(dev, *bad)                                          # a per-sample array of the wrong length
    with pytest.raises(ValueError):
        hip.recon_augment(dev, [0, 2, 0], *ok[1:])
    with pytest.raises(ValueError):
        hip.recon_augment(dev, ok[0], [1.0, float('nan'), 1.0], ok[2], ok[3])
    with pytest.raises(ValueError):
        hip.recon_augment(dev, ok[0], ok[1], [1.0, -0.5, 1.0], ok[3])
    with pytest.raises(ValueError):
        hip.recon_augment(dev, *ok, out=torch.empty(cases.B, 3, 5, 7, device='cuda', dtype=torch.float64))
    with pytest.raises(ValueError):
        hip.recon_augment(dev, *ok, out=torch.empty(cases.B, 3, 5, 7))
    canary = torch.full((cases.B, 3, 5, 7), -7.0, device='cuda')
    with pytest.raises(ValueError):
        hip.recon_augment(dev, [0, 0], *ok[1:], out=canary)
    assert bool((canary == -7.0).all())                                           # nothing was launched on it
