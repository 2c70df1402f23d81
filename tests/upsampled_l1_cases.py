"""Shared cases of the fused upsampled-L1 node's test (K23, tests/test_hip_upsampled_l1_f32.py) and of the CPU measurement that
sets its bound (tools/exp_openess_fp32_bounds.py): seeded fp32 operands, conditioned so that no sign of the upsampled difference
sits on a rounding error, and the torch reference in any dtype (float64: the reference; float32 on the CPU: the yardstick the
bound is four times of).  Nothing here needs a GPU."""
import numpy as np
import torch
import torch.nn.functional as F

# (B, C, h, w, Ho, Wo, align_corners): small on purpose, each names one way the kernel can go wrong
CASES = [(2, 256, 3, 4, 44, 61, False),        # the workload's channel count, non-integer scale on both axes
         (1, 64, 5, 7, 37, 53, False),
         (3, 12, 2, 3, 9, 16, False),          # C % 64 != 0
         (2, 64, 1, 5, 8, 33, False),          # one source row: i1 == i0
         (2, 64, 4, 5, 13, 17, True),          # align_corners
         (1, 64, 2, 3, 64, 96, False),         # integer x32: wide border clamp
         (2, 256, 2, 3, 64, 96, False),
         (2, 256, 4, 6, 64, 96, False)]        # integer x16: the trainer test's geometry (any output_stride but 8 is stride 16)
SLICE_CASE, SLICE_OF, SLICE_AT = 1, 128, 32    # case 1 with both operands as channels [32:96] of 128-channel channels_last tensors
FALLBACK_CASE, FALLBACK_C = 2, 6               # case 2 with C = 6: refused by the entries, served by hip.l1_mean
MARGIN = 1e-5                                  # every |up(a) - up(b)| >= MARGIN * max|up(a) - up(b)|
MAX_ROUNDS = 20


def relerr(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def up(x, size, align):
    return F.interpolate(x, size=size, mode='bilinear', align_corners=align)


def _nearest_source(n_in, n_out, align):
    """nearest input index of every output index under ATen's bilinear source rule"""
    o = np.arange(n_out, dtype=np.float64)
    if align:
        src = o * ((n_in - 1) / (n_out - 1)) if n_out > 1 else np.zeros_like(o)
    else:
        src = np.maximum((o + 0.5) * n_in / n_out - 0.5, 0.0)
    return np.clip(np.rint(src).astype(np.int64), 0, n_in - 1)


def margin_of(a, b, size, align):
    """(smallest |up(a) - up(b)| / largest, the float64 upsampled difference)"""
    u = up(a.double(), size, align) - up(b.double(), size, align)
    return float(u.abs().min() / u.abs().max()), u


def condition(a, b, size, align):
    """Nudge `a` (float64 copy of the fp32 draw) until every |up(a) - up(b)| holds MARGIN: each element under it adds
    2^-5 (1 + round % 5), signed away from zero, to its nearest low-resolution element of a (a fixed size ping-pongs between two
    neighbours; the varying size converges).  Returns (a rounded to fp32, rounds)."""
    a64 = a.double().clone()
    ny, nx = _nearest_source(a.shape[2], size[0], align), _nearest_source(a.shape[3], size[1], align)
    for rnd in range(MAX_ROUNDS):
        m, u = margin_of(a64.float(), b, size, align)
        if m >= MARGIN:
            return a64.float(), rnd
        bad = (u.abs() < MARGIN * u.abs().max()).nonzero().numpy()                    # rows of (b, c, oy, ox)
        sign = np.where(u.numpy()[tuple(bad.T)] < 0, -1.0, 1.0)
        flat = np.ravel_multi_index((bad[:, 0], bad[:, 1], ny[bad[:, 2]], nx[bad[:, 3]]), tuple(a64.shape))
        flat, first = np.unique(flat, return_index=True)                              # one nudge per low-resolution element
        a64.view(-1)[torch.from_numpy(flat)] += torch.from_numpy(sign[first] * 2.0 ** -5 * (1 + rnd % 5))
    raise AssertionError("conditioning did not converge")


def reference(a, b, size, align, dtype):
    """(loss, grad_a, grad_b) of F.l1_loss(F.interpolate(a), F.interpolate(b)) in `dtype` with torch's autograd on the CPU"""
    aa, bb = a.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
    loss = F.l1_loss(up(aa, size, align), up(bb, size, align))
    ga, gb = torch.autograd.grad(loss, (aa, bb))
    return loss.detach(), ga, gb


_CACHE = {}


def case(i, C=None):
    """dict of case i (C: another channel count from the same seed): fp32 `a`, `b` [B, C, h, w], `size`, `align`, the float64
    reference `loss`, `grad_a`, `grad_b`, the `margin` that holds for EVERY element and the conditioning `rounds`"""
    key = (i, C)
    if key not in _CACHE:
        B, C0, h, w, Ho, Wo, align = CASES[i]
        C = C0 if C is None else C
        g = torch.Generator().manual_seed(2300 + i)
        a, b = torch.randn(B, C, h, w, generator=g), torch.randn(B, C, h, w, generator=g)
        a, rounds = condition(a, b, (Ho, Wo), align)
        margin, _ = margin_of(a, b, (Ho, Wo), align)
        assert margin >= MARGIN, (CASES[i], C, margin)                                # no element is left out
        loss, ga, gb = reference(a, b, (Ho, Wo), align, torch.float64)
        _CACHE[key] = dict(a=a, b=b, size=(Ho, Wo), align=align, loss=loss, grad_a=ga, grad_b=gb, margin=margin, rounds=rounds)
    return _CACHE[key]


def fp32_cpu_errors(i, C=None):
    """relerr of torch's fp32 CPU run against the float64 reference: {'loss', 'grad_a', 'grad_b'}"""
    c = case(i, C)
    loss, ga, gb = reference(c['a'], c['b'], c['size'], c['align'], torch.float32)
    return {'loss': relerr(loss.numpy(), c['loss'].numpy()), 'grad_a': relerr(ga.numpy(), c['grad_a'].numpy()),
            'grad_b': relerr(gb.numpy(), c['grad_b'].numpy())}
