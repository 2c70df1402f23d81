"""Cases of the bf16 ConvLSTM kernel tests (tests/test_hip_convlstm.py, tests/test_convlstm_host.py): seeded random operands,
the exact cases and their integer expectations.  Tensors are in the reference's own layout: x [B, Cx, H, W], h and the cell
[B, C, H, W], the Gates weight [4C, Cx + C, k, k] over cat(x, h) with rows gate * C + hc, gates (in, remember, out, cell)."""
import math

import numpy as np
import torch

GATES = ('i', 'r', 'o', 'c')             # row blocks of Gates.weight: in, remember, out, cell (submodules.py:205)
PREV_CELL = 40                           # previous cells of the exact cases are 0 or +-PREV_CELL
TANH1_BF16 = 0.76171875                  # bf16(tanh(1))

# ((B, H, W, Cx, C), k, {zero-state form?: route}): exact cases of the single launch hip.convlstm_fused, every route in both
# forms.  The zero-state form convolves x alone (Cin = Cx), which may be another kernel's
HALO, FASTK, SLOWK = 'HALO3X3_LSTM', 'LSTM_FASTK', 'LSTM_SLOWK'
EXACT_SINGLE = [
    # row-halo kernel: 198 pixels = a full 128-row tile + a ragged one that starts in batch 0 and ends batch 1; 4C = 384 = three
    # 128-column gate tiles.  Zero-state form: Cin = 96, the slow-K general kernel
    ((2, 9, 11, 96, 96), 3, {False: HALO, True: SLOWK}),
    ((1, 5, 7, 64, 64), 3, {False: HALO, True: HALO}),         # one ragged tile; a 128-row tile spans all five image rows
    ((1, 9, 20, 64, 64), 5, {False: FASTK, True: FASTK}),      # 5 x 5 gates: general kernel with fast K (Cin % 64 == 0), all 25 taps
    ((2, 9, 10, 64, 32), 3, {False: SLOWK, True: HALO}),       # Cin = 96: slow K, a tile across the batch border, one gate tile
    ((2, 9, 10, 32, 32), 3, {False: HALO, True: SLOWK}),       # zero-state form of a Cx = 32 block: Cin = 32, half a K slab per tap
]
# 138 m-tiles x 4 gate tiles = 552 workgroups: more than one round of the 512 resident ones, ragged last m-tile.  Exact case
# only: its expectation is a gather, no float64 convolution at this size
EXACT_LARGE = ((1, 110, 160, 128, 128), 3, {False: HALO, True: HALO})
# (B, H, W, C) with Cx = C: the grouped launch (hip.convlstm_fused_group), three problems, the middle one in the zero-state form.
# Every one is the row-halo kernel's and fits the 256-row tiles (halo rows 269 / 282 / 301 <= 320): 2 x 2, 1 x 4, 1 x 4 tiles
GROUP = [(1, 16, 24, 64), (1, 9, 11, 128), (3, 5, 6, 128)]
# the persistent w128 kernel: 4.5 tiles of 256 pixels (ragged, tiles across image borders); an odd width (every tile starts
# mid-row) with two 256-column gate tiles
W128 = [(3, 16, 24, 64), (1, 16, 41, 128)]
# float64 bounds (random_case): ((B, H, W, Cx, C), k, zero-state form?, route) at the geometries of
# test_convlstm_fused_step_matches_torch that a float64 convolution affords, on every route the single launch takes there
BOUND_CASES = [
    ((2, 9, 11, 32, 32), 3, False, HALO), ((2, 9, 11, 32, 32), 3, True, SLOWK), ((2, 9, 11, 32, 32), 5, False, FASTK),
    ((1, 13, 10, 64, 64), 3, False, HALO), ((1, 13, 10, 64, 64), 3, True, HALO), ((1, 13, 10, 64, 64), 5, False, FASTK),
    ((3, 8, 8, 96, 32), 3, False, HALO), ((3, 8, 8, 96, 32), 3, True, SLOWK), ((3, 8, 8, 96, 32), 5, False, FASTK), ((3, 8, 8, 96, 32), 5, True, SLOWK),
]
W128_BOUND_GEOM = (3, 16, 24, 64)
# the unfused gate kernel (the path of C % 32 != 0): (B, H, W, C), eight channels per thread
GATES_GEOM = (2, 5, 7, 40)


def random_case(B, H, W, Cx, C, k, seed=None):
    """Seeded operands of one step: x, h fp32, the previous cell 'c' O(1), the Gates weight 'w' [4C, Cx + C, k, k] scaled so that
    the pre-activations are O(1), and the bias 'b' [4C]."""
    g = torch.Generator().manual_seed(1000 * B + 10 * C + H + 7 * k if seed is None else seed)
    r = lambda *s: torch.randn(*s, generator=g)
    sc = 1.5 / (k * k * (Cx + C)) ** 0.5
    return {'x': r(B, Cx, H, W), 'h': 0.6 * r(B, C, H, W), 'c': r(B, C, H, W), 'w': sc * r(4 * C, Cx + C, k, k), 'b': 0.2 * r(4 * C)}


def old_scale_case(B, H, W, Cx, C, seed=0):
    """Operands on the scales of test_convlstm_fused_step_matches_torch (tests/test_hip_conv.py): weights 0.05 randn, bias
    0.1 randn, x randn; h and the cell as a recurrent step leaves them (|h| < 1, cell O(1))."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return {'x': r(B, Cx, H, W), 'h': torch.tanh(r(B, C, H, W)) * 0.5, 'c': 0.5 * r(B, C, H, W), 'w': 0.05 * r(4 * C, Cx + C, 3, 3),
            'b': 0.1 * r(4 * C)}


def exact_case(B, H, W, Cx, C, k, seed=3):
    """Operands whose step is known in integers: x, h in {-1, +1}; the previous cell in {0, +-40}; every gate row is one-hot (one
    input channel at one tap, magnitude 256, alternating sign); biases are +-128.  All are bf16-exact.  Every pre-activation is
    then an integer of magnitude >= 128 (128 where the tap falls into the zero padding), so the sigmoids are exactly 0 or 1 and
    tanh of the cell gate exactly +-1 in fp32, the fast forms of conv_args.h included.  Over the rows of a gate the tap
    (hc + 4 gate) % k^2 visits all k^2 taps and the input channel (7 hc + 3 + 5 gate) % (Cx + C) both halves of cat(x, h).
    Returns the operands (as random_case) plus 'taps': per gate the (input channel, dy, dx, sign) of each of its C rows."""
    rng = np.random.default_rng(seed)
    pm = lambda *s: torch.from_numpy(rng.integers(0, 2, s) * 2 - 1).float()
    Cin = Cx + C
    case = {'x': pm(B, Cx, H, W), 'h': pm(B, C, H, W), 'taps': {}}
    case['c'] = torch.from_numpy((rng.integers(0, 3, (B, C, H, W)) - 1) * PREV_CELL).float()
    w = torch.zeros(4 * C, Cin, k, k)
    for gi, name in enumerate(GATES):
        taps = []
        for hc in range(C):
            ci = (7 * hc + 3 + 5 * gi) % Cin
            tap = (hc + 4 * gi) % (k * k)
            sign = 1 if (hc + gi) % 2 == 0 else -1
            w[gi * C + hc, ci, tap // k, tap % k] = 256.0 * sign
            taps.append((ci, tap // k, tap % k, sign))
        case['taps'][name] = taps
    case['w'] = w
    case['b'] = torch.from_numpy((rng.integers(0, 2, 4 * C) * 2 - 1) * 128).float()
    return case


def bf16_of_tanh(c):
    """bf16(tanh(c)) of an integer c, as a Python float."""
    return float(torch.tensor(math.tanh(c), dtype=torch.float32).bfloat16())


def tie_margin(c):
    """Distance of tanh(c) from the nearest point at which its bf16 rounding changes (the midpoints between neighbouring bf16
    values), for an integer c != 0."""
    t = abs(math.tanh(c))
    e = math.floor(math.log2(t))
    ulp = 2.0 ** (e - 7)                 # bf16: 8 significand bits
    q = t / ulp
    return abs(q - (math.floor(q) + 0.5)) * ulp


def cell_update(pre, c):
    """The gate algebra on integer pre-activations: pre int64 [B, 4C, H, W] with |pre| >= 128, c int64 [B, C, H, W].  Returns
    (c' int64, h' fp32): c' = r c + i g with i, r in {0, 1} and g in {-1, +1}; h' = o bf16(tanh(c')), which is 0 where o = 0 or
    c' = 0, +-1 where |c'| >= 4 (tanh(4) = 0.99933 rounds to 1) and a fixed bf16 value in between (test_convlstm_host.py
    holds every such tanh(c') 1e-4 away from a rounding boundary)."""
    assert int(pre.abs().min()) >= 128
    pi, pr, po, pc = pre.chunk(4, 1)
    i, r, o = (pi > 0).to(torch.int64), (pr > 0).to(torch.int64), (po > 0).to(torch.int64)
    g = torch.where(pc > 0, 1, -1)
    cell = r * c + i * g
    th = torch.zeros(cell.shape, dtype=torch.float32)
    for v in cell.unique().tolist():
        th[cell == v] = bf16_of_tanh(v)
    return cell, o.float() * th


def exact_pre(case, fresh=False):
    """int64 pre-activations [B, 4C, H, W] of exact_case by gathers from the zero-padded input (no convolution).  fresh: the
    zero-state form, the x half of the weight alone (rows whose input channel lies in the h half are left with their bias)."""
    x = case['x'].to(torch.int64)
    inp = x if fresh else torch.cat([x, case['h'].to(torch.int64)], 1)
    B, Cin, H, W = inp.shape
    k = case['w'].shape[-1]
    pad = k // 2
    p = torch.zeros(B, Cin + 1, H + 2 * pad, W + 2 * pad, dtype=torch.int64)      # channel Cin: zeros, for the rows left out
    p[:, :Cin, pad:pad + H, pad:pad + W] = inp
    rows = [256 * s * p[:, ci if ci < Cin else Cin, dy:dy + H, dx:dx + W] for n in GATES for ci, dy, dx, s in case['taps'][n]]
    return torch.stack(rows, 1) + case['b'].to(torch.int64).view(1, -1, 1, 1)


def exact_expected(case, fresh=False):
    """(pre int64 [B, 4C, H, W], c' int64 [B, C, H, W], h' fp32 [B, C, H, W]) of one step on exact_case.  fresh: the zero-state
    form: only the x half of the weight, no previous cell."""
    pre = exact_pre(case, fresh)
    c = torch.zeros_like(case['c']) if fresh else case['c']
    return (pre,) + cell_update(pre, c.to(torch.int64))


def possible_cells(steps=2):
    """Every value the cell of an exact case can take after 1 .. `steps` steps from {0, +-40}: c' = r c + i g."""
    cur, seen = {0, PREV_CELL, -PREV_CELL}, set()
    for _ in range(steps):
        cur = {r * c + i * g for c in cur for r in (0, 1) for i in (0, 1) for g in (-1, 1)}
        seen |= cur
    return sorted(seen)


def exact_gates(B, H, W, C, seed=5):
    """Operands of the unfused gate kernel alone: bf16-exact gates of +-128 [B, 4C, H, W] and a previous cell in {0, +-40}."""
    rng = np.random.default_rng(seed)
    return {'gates': torch.from_numpy((rng.integers(0, 2, (B, 4 * C, H, W)) * 2 - 1) * 128).float(),
            'c': torch.from_numpy((rng.integers(0, 3, (B, C, H, W)) - 1) * PREV_CELL).float()}


def random_gates(B, H, W, C, seed=6):
    g = torch.Generator().manual_seed(seed)
    return {'gates': (2.0 * torch.randn(B, 4 * C, H, W, generator=g)).bfloat16().float(), 'c': torch.randn(B, C, H, W, generator=g)}
