"""Cases of the tests of oess_upsample_bilinear2x_sum_nhwc_bf16: shapes, input families, buffer layouts and the
derived bound.  Shared by tests/test_upsample_sum_reference.py (CPU) and tests/test_hip_upsample_sum.py (GPU).  Nothing here
needs a GPU.

Bound of the non-exact families, from the number formats alone (not from what the kernel gives):

    |out - ref| <= 2^-8 |ref| + 2^-20 A,      A = the largest |x| + |skip| among the output's four taps

2^-8 |ref| is half a bf16 ulp (8 significand bits) of the ONE rounding at the store; 2^-20 A covers at most eight fp32 roundings
(2^-24 relative each, of quantities no larger than A, with a factor two to spare) of the sum and the two lerps in either order.
A result that needs more has rounded to bf16 twice somewhere."""
import numpy as np
import torch

SEED = 3011
# (B, C, H, W): single pixel, single row, single column, odd sizes, C no power of two, the decoder's widest level, and one
# that spans several workgroups (33 * 17 * 8 lanes = 18 workgroups of 256)
SHAPES = ((1, 8, 1, 1), (1, 8, 1, 5), (2, 8, 2, 1), (1, 24, 3, 2), (2, 40, 5, 7), (2, 256, 7, 9), (1, 64, 33, 17))
FAMILIES = ("exact", "randn", "large_offset", "large_offset_cancel")
# name -> (channel offset, extra channels of the wider buffer): pixel stride C + extra
LAYOUTS = {"dense": (0, 0), "slice": (8, 24)}
POISON_IN = float("nan")                  # the channels of a wider INPUT buffer that no lane may read
POISON_OUT = -7.0                         # the channels of a wider OUTPUT buffer that must survive


def case_id(shape, with_skip, layout):
    return "x".join(map(str, shape)) + ("_skip_" if with_skip else "_noskip_") + layout


def _gen(*key):
    h = SEED
    for k in key:
        for ch in str(k):
            h = (h * 1000003 + ord(ch)) % (1 << 31)
    return torch.Generator().manual_seed(h)


def operands(shape, family, with_skip):
    """(x, skip | None): CPU bf16 [B, H, W, C] tensors.
    exact: values of 16 * {-4 .. 4}: every sum and every weighted sum (weights k / 16) is an integer of magnitude <= 128, exact
    in bf16.  large_offset: 1000 + randn on both operands.  large_offset_cancel: the skip negated, so the fp32 sum cancels to
    the order of a bf16 ulp at 1000 while A stays near 2000."""
    B, C, H, W = shape
    g = _gen(shape, family, with_skip)

    def draw(sign=1.0):
        if family == "exact":
            return (16 * torch.randint(-4, 5, (B, H, W, C), generator=g)).to(torch.bfloat16)
        t = torch.randn(B, H, W, C, generator=g)
        if family != "randn":
            t = sign * (1000.0 + t)
        return t.to(torch.bfloat16)
    x = draw()
    skip = draw(-1.0 if family == "large_offset_cancel" else 1.0) if with_skip else None
    return x, skip


def place(t, layout, device, poison=POISON_IN):
    """CPU [B, H, W, C] bf16 -> (view on `device` laid out as `layout`, the buffer that holds it)."""
    c0, extra = LAYOUTS[layout]
    B, H, W, C = t.shape
    big = torch.full((B, H, W, C + extra), poison, dtype=torch.bfloat16, device=device)
    view = big[..., c0:c0 + C]
    view.copy_(t)
    return view, big


def out_view(shape, layout, device):
    """(output view [B, 2H, 2W, C] on `device`, the poisoned buffer that holds it)."""
    B, C, H, W = shape
    c0, extra = LAYOUTS[layout]
    big = torch.full((B, 2 * H, 2 * W, C + extra), POISON_OUT, dtype=torch.bfloat16, device=device)
    return big[..., c0:c0 + C], big


def neighbours_untouched(big, layout, C):
    c0, _ = LAYOUTS[layout]
    return bool((big[..., :c0] == POISON_OUT).all()) and bool((big[..., c0 + C:] == POISON_OUT).all())


def bound(ref, A):
    return 2.0 ** -8 * np.abs(ref) + 2.0 ** -20 * A
