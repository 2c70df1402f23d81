"""Cases of the ConvGRU kernel tests (tests/test_hip_convgru.py, tests/test_convgru_host.py, tools/exp_convgru_bounds.py)."""
import numpy as np
import torch

# (B, H, W, C): ragged m-tile across a batch border; C = 64; C / 32 odd; more tiles than one round of workgroups (138 tiles
# of 128 pixels x 2 weight-row tiles in the gates launch), ragged last tile
GEOMS = [(2, 9, 11, 32), (1, 13, 10, 64), (3, 8, 8, 96), (1, 110, 160, 128)]
GEOMS_F32 = [(2, 9, 11, 32), (1, 13, 10, 64)]
# exact cases: 198 pixels = one full 128-pixel tile + a ragged one that starts inside batch 0 and ends batch 1; three 32-blocks
# of hidden channels (two weight-row tiles in the gates launch, the second half valid)
EXACT_GEOMS = [(2, 9, 11, 96), (1, 5, 7, 32)]


def random_case(B, H, W, C, seed=None):
    """Seeded operands of one step: x, h fp32 [B, C, H, W] and the three gates' weights [C, 2C, 3, 3] / biases [C], scaled so
    that the pre-activations are O(1)."""
    g = torch.Generator().manual_seed(1000 * B + 10 * C + H if seed is None else seed)
    r = lambda *s: torch.randn(*s, generator=g)
    sc = 1.5 / (9 * 2 * C) ** 0.5
    return {'x': r(B, C, H, W), 'h': 0.6 * r(B, C, H, W),
            'wu': sc * r(C, 2 * C, 3, 3), 'bu': 0.2 * r(C), 'wr': sc * r(C, 2 * C, 3, 3), 'br': 0.2 * r(C),
            'wo': sc * r(C, 2 * C, 3, 3), 'bo': 0.2 * r(C)}


def exact_case(B, H, W, C, seed=3):
    """Operands whose step is exact in every precision: x, h in {-1, +1}; every weight row is one-hot (one input channel at one
    tap, the tap varying per row over all nine, magnitude 256, alternating sign); biases are +-128.  Every pre-activation then
    has magnitude >= 128: sigmoid is exactly 0 or 1 and tanh exactly -1 or +1 in fp32 (fast forms included) and in float64.
    Returns the operands (as random_case) plus 'taps': per gate the (input channel, dy, dx, sign) of each row."""
    rng = np.random.default_rng(seed)
    pm = lambda *s: torch.from_numpy(rng.integers(0, 2, s) * 2 - 1).float()
    case = {'x': pm(B, C, H, W), 'h': pm(B, C, H, W), 'taps': {}}
    for gi, name in enumerate(('u', 'r', 'o')):
        w = torch.zeros(C, 2 * C, 3, 3)
        taps = []
        for hc in range(C):
            ci = (7 * hc + 3 + 5 * gi) % (2 * C)
            tap = (hc + 4 * gi) % 9
            sign = 1 if (hc + gi) % 2 == 0 else -1
            w[hc, ci, tap // 3, tap % 3] = 256.0 * sign
            taps.append((ci, tap // 3, tap % 3, sign))
        case['w' + name] = w
        case['b' + name] = torch.from_numpy((rng.integers(0, 2, C) * 2 - 1) * 128).float()
        case['taps'][name] = taps
    return case


def _pre_int(inp, taps, bias):
    """Integer pre-activations of one gate: inp int64 [B, 2C, H, W], zero padded by one pixel."""
    B, _, H, W = inp.shape
    p = torch.zeros(B, inp.shape[1], H + 2, W + 2, dtype=torch.int64)
    p[:, :, 1:-1, 1:-1] = inp
    rows = [256 * s * p[:, ci, dy:dy + H, dx:dx + W] for ci, dy, dx, s in taps]
    return torch.stack(rows, 1) + bias.to(torch.int64).view(1, -1, 1, 1)


def exact_expected(case):
    """(pre_u, pre_r, u, r * h, pre_o, h') of exact_case in integers (int64 [B, C, H, W])."""
    x, h = case['x'].to(torch.int64), case['h'].to(torch.int64)
    s = torch.cat([x, h], 1)
    pre_u = _pre_int(s, case['taps']['u'], case['bu'])
    pre_r = _pre_int(s, case['taps']['r'], case['br'])
    assert int(pre_u.abs().min()) >= 128 and int(pre_r.abs().min()) >= 128
    u, r = (pre_u > 0).to(torch.int64), (pre_r > 0).to(torch.int64)
    rh = r * h
    pre_o = _pre_int(torch.cat([x, rh], 1), case['taps']['o'], case['bo'])
    assert int(pre_o.abs().min()) >= 128
    o = torch.where(pre_o > 0, 1, -1)
    return pre_u, pre_r, u, rh, pre_o, h * (1 - u) + o * u
