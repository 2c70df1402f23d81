"""Cases, inputs and the bounds (confidence, name value) shared by the tests of oess_segment_render_grouped / oess_head_render and by
tools/exp_vocab_render_bounds.py.  Nothing here needs a GPU."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import segment_render_cases as sc

DTYPES = sc.DTYPES
case_id = sc.case_id


def offsets_of(sizes):
    return [0] + np.cumsum(sizes).tolist()


# the reference's pseudo-label writer: 36 names merged into 11 classes
SIZES_36 = [1, 2, 1, 5, 3, 1, 1, 5, 13, 1, 3]
# (P, class offsets): two classes; the writer's groups; one class of 255 names; 255 classes, the first 45 with two names
VOCABULARIES = {5: [0, 1, 5], 36: offsets_of(SIZES_36), 255: [0, 255], 300: offsets_of([2] * 45 + [1] * 210)}

# ---------------------------------------------------------------------------------------------------------------- grouped render
# (P, (B, P, h, w), (H, W) | None, align_corners)
GROUP_CASES = [(P, (B, P, h, w), size, False) for P in VOCABULARIES
               for (B, h, w), size in (((1, 1, 1), (3, 5)), ((2, 3, 4), (7, 9)), ((2, 3, 4), None))]
GROUP_CASES += [(36, (2, 36, 7, 9), (112, 144), False),
                (36, (2, 36, 3, 4), (7, 9), True),
                # two source rows of 25 x 300 fp32 = 60 000 bytes: above the 48 KB LDS budget, the taps come from global memory
                (300, (1, 300, 2, 25), (3, 40), False)]


def group_case_id(P, shape, size, align):
    return f"K{len(VOCABULARIES[P]) - 1}-" + case_id(shape, size, align)


def torch_group_conf(x, offsets, size, align, dtype):
    """max softmax over the per-group amax of F.interpolate(x), torch on the CPU in `dtype`: [B, H, W]"""
    v = x.to(dtype)
    if size is not None and tuple(size) != tuple(x.shape[2:]):
        v = F.interpolate(v, size=tuple(size), mode='bilinear', align_corners=align)
    c = torch.stack([v[:, a:b].amax(1) for a, b in zip(offsets[:-1], offsets[1:])], 1)
    return c.softmax(1).max(1).values


# -------------------------------------------------------------------------------------------------------------------- fused head
# exact operands: small integers, every product and partial sum exact in float32 (|v| <= 64 * 4 * 3 + 8)
EXACT_C = (1, 3, 32, 64)
EXACT_W = (1, 5, 257)
EXACT_GROUPS = [0, 2, 3, 7]                    # P = 7, K = 3; the singleton form has P = K = 5


def exact_case(C, W, dtype):
    """(x [2, C, 3, W], weight [P, C], bias | None, offsets | None, slice layout?) -- groups, bias and layout vary with the case"""
    n = EXACT_C.index(C) * len(EXACT_W) + EXACT_W.index(W) + (dtype == "bf16")
    g = torch.Generator().manual_seed(700 + n)
    grouped, with_bias, sliced = bool(n & 1), bool(n & 2) or C == 1, bool(n & 4)
    P = 7 if grouped else 5
    x = torch.randint(-4, 5, (2, C, 3, W), generator=g).float()
    weight = torch.randint(-3, 4, (P, C), generator=g).float()
    bias = torch.randint(-8, 9, (P,), generator=g).float() if with_bias else None
    return x, weight, bias, (EXACT_GROUPS if grouped else None), sliced


# random operands: (name, P, offsets); x [2, 32, 9, 13] ~ N(0, 1), weight ~ 0.3 N(0, 1), bias ~ N(0, 1)
RANDOM_SHAPE = (2, 32, 9, 13)
RANDOM_CASES = [("P36-K11", 36, VOCABULARIES[36]), ("P19-K19", 19, list(range(20)))]
SKIP_CAP = 0.01                                # share of pixels whose top-2 margin lies within the value bound


def random_case(P, dtype):
    g = torch.Generator().manual_seed(900 + P)
    x = torch.randn(*RANDOM_SHAPE, generator=g)
    x = x.to(torch.bfloat16).float() if dtype == "bf16" else x
    return x, 0.3 * torch.randn(P, RANDOM_SHAPE[1], generator=g), torch.randn(P, generator=g)


def torch_head(x, weight, bias, offsets, dtype):
    """(name values [B, P, H, W], confidence [B, H, W]) of torch on the CPU in `dtype`: 1 x 1 conv -> per-group amax -> softmax -> max"""
    v = F.conv2d(x.to(dtype), weight.to(dtype)[:, :, None, None], None if bias is None else bias.to(dtype))
    c = torch.stack([v[:, a:b].amax(1) for a, b in zip(offsets[:-1], offsets[1:])], 1)
    return v, c.softmax(1).max(1).values


def pixel_bound(scale):
    """[B, H, W]: the value bound of a pixel, VALUE_BOUND times its largest scale |bias_p| + sum_c |w[p][c] x[c]| over the names"""
    return VALUE_BOUND * np.asarray(scale).max(axis=1)


# ------------------------------------------------------------------------------------------------------------------------ bounds
# tools/exp_vocab_render_bounds.py measures torch's own float32 path against the same in float64 on the cases above (the convention
# of K19 - K35: a bound is four times its figure; test_vocab_render_reference.py holds the constants to what the tool measures).
# The confidence bound has one figure per kernel, each from that kernel's own cases:
# GROUP_CONF: |confidence32 - confidence64| over GROUP_CASES x DTYPES (interpolate -> per-group amax -> softmax -> max).
GROUP_CONF_FIGURE = 1.0649664405892878e-07     # at K11-2x36x7x9-112x144-fp32
GROUP_CONF_BOUND = 4.0 * GROUP_CONF_FIGURE
# HEAD_CONF: the same over RANDOM_CASES x DTYPES (1 x 1 conv -> per-group amax -> softmax -> max).
HEAD_CONF_FIGURE = 3.715204969223507e-07       # at P19-K19-bf16
HEAD_CONF_BOUND = 4.0 * HEAD_CONF_FIGURE
# VALUE: |v32 - v64| / (|bias_p| + sum_c |w[p][c] x[c]|) of the 1 x 1 conv over RANDOM_CASES x DTYPES: RELATIVE to the scale of a
# name value's terms, so that it carries over to operands of another magnitude (tests/test_hip_open_vocabulary.py).
VALUE_FIGURE = 2.98498363888397e-07            # at P19-K19-fp32
VALUE_BOUND = 4.0 * VALUE_FIGURE


def measure_figures(report=None):
    """{'group_conf' | 'head_conf' | 'value': (figure, where)} as described above"""
    from tests import vocab_render_reference as vr
    worst = {'group_conf': (0.0, None), 'head_conf': (0.0, None), 'value': (0.0, None)}

    def note(kind, name, d):
        if report is not None:
            report(kind, name, d)
        if d > worst[kind][0]:
            worst[kind] = (d, name)
    for P, shape, size, align in GROUP_CASES:
        for dtype in DTYPES:
            x, offs = sc.logits(shape, dtype), VOCABULARIES[P]
            d = (torch_group_conf(x, offs, size, align, torch.float32).double() - torch_group_conf(x, offs, size, align, torch.float64))
            note('group_conf', f"{group_case_id(P, shape, size, align)}-{dtype}", float(d.abs().max()))
    for name, P, offs in RANDOM_CASES:
        for dtype in DTYPES:
            x, w, b = random_case(P, dtype)
            v32, c32 = torch_head(x, w, b, offs, torch.float32)
            v64, c64 = torch_head(x, w, b, offs, torch.float64)
            scale = vr.head_values64(x.numpy(), w.numpy(), b.numpy())[1]
            note('head_conf', f"{name}-{dtype}", float((c32.double() - c64).abs().max()))
            note('value', f"{name}-{dtype}", float(((v32.double() - v64).abs().numpy() / scale).max()))
    return worst
