"""The case list of the K27 tests (hip.recon_augment): shapes, inputs and per-sample augmentation columns, shared by the CPU checks
(tests/test_recon_augment_cases.py), the GPU tests (tests/test_hip_recon_augment.py) and tools/exp_recon_augment_bounds.py."""
import numpy as np

B = 3
# 5 x 7: smaller than one workgroup, odd W under flip; 37 x 53: ragged (H W % 4 != 0: the 4-byte store route, element groups
# that straddle channel planes); 64 x 96: the 16-byte route; 130 x 257: 33 410 pixels = 9 partials of 4096, so the second
# reduction level adds more than one partial (and H W % 4 != 0 again)
SHAPES = ((5, 7), (37, 53), (64, 96), (130, 257))
STATS_SHAPE = (130, 257)

SEEDS = (0x1234_5678_9ABC_DEF1, 7, (1 << 62) - 1)           # both key words used, a small one, the largest the loader draws


def grey(shape, seed=0):
    """uint8 [B, H, W]: smooth structure + texture, all 256 levels present where the sample is large enough, and saturated
    patches so that the clamps at 0 and 1 are exercised."""
    H, W = shape
    rng = np.random.default_rng(1205 + seed + 1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((B, H, W), dtype=np.uint8)
    for b in range(B):
        base = 127.5 + 100.0 * np.sin(0.11 * (b + 1) * yy) * np.cos(0.07 * (b + 2) * xx)
        img = np.clip(base + rng.normal(0, 30, (H, W)), 0, 255)
        img[: max(H // 6, 1), : max(W // 5, 1)] = 255
        img[-max(H // 7, 1):, -max(W // 6, 1):] = 0
        out[b] = img.astype(np.uint8)
    if H * W >= 256:
        out[0].reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    return out


OFF = dict(flip=[0, 0, 0], brightness=[1.0, 1.0, 1.0], contrast=[1.0, 1.0, 1.0], noise_seed=[0, 0, 0])


def case(**kw):
    return dict(OFF, **kw)


# rows compared against the float64 restatement under the measured fp32 bound (tools/exp_recon_augment_bounds.py): contrast alone
# (below, at and above 1; one sample without a blend next to two with one), and everything but the noise combined
CONTRAST_CASES = {
    'contrast': case(contrast=[0.8, 1.0, 1.2]),
    'contrast_extreme': case(contrast=[0.0, 2.0, 0.3]),
    'combined': case(flip=[1, 0, 1], brightness=[0.83, 1.19, 1.0], contrast=[1.17, 0.81, 0.93]),
}
NOISE_CASE = case(flip=[0, 1, 0], brightness=[1.0, 0.9, 1.1], contrast=[1.0, 1.1, 1.0], noise_seed=list(SEEDS))
