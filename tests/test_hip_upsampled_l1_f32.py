"""K23: hip.upsampled_l1_mean, the joint stage's fp32 L1 feature-consistency loss as one node on the two low-resolution maps
(openess_amd/csrc/upsampled_l1_f32.hip), against float64 F.l1_loss(F.interpolate(a), F.interpolate(b)) with its autograd.

Cases and conditioning: tests/upsampled_l1_cases.py (every |up(a) - up(b)| holds 1e-5 of the largest, asserted there on the
float64 side, so no sign sits on a rounding error).  Measure: max|delta| / max|expected| per tensor.  Bound: the project's rule,
four times torch's own fp32 CPU error with a floor of 1e-5; tools/exp_openess_fp32_bounds.py prints those figures (loss <= 5.7e-8,
gradients <= 2.4e-6, case 0), so the bound is 1e-5 for the loss and both gradients.
Measured on the MI355X over the eight cases and the two variants: loss <= 3.2e-8, gradients <= 5.3e-7 (case 0); the table is in
DESIGN.md K23."""
import pytest
import torch

from tests import upsampled_l1_cases as uc

pytestmark = pytest.mark.gpu
BOUND = 1e-5


def _run(a, b, size, align, need=(True, True)):
    """(loss, grad_a, grad_b) of the node on device operands a, b (logical NCHW)"""
    from openess_amd import hip
    a = a.detach().requires_grad_(need[0])
    b = b.detach().requires_grad_(need[1])
    loss = hip.upsampled_l1_mean(hip.UpsampledFeature(a, size, align), hip.UpsampledFeature(b, size, align))
    loss.backward()
    return loss.detach(), a.grad, b.grad


def _check(c, loss, ga, gb, what):
    errs = {'loss': uc.relerr(loss.cpu().numpy(), c['loss'].numpy()), 'grad_a': uc.relerr(ga.cpu().numpy(), c['grad_a'].numpy()),
            'grad_b': uc.relerr(gb.cpu().numpy(), c['grad_b'].numpy())}
    print(f"upsampled_l1 {what}: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f" (margin {c['margin']:.3e})")
    for k, v in errs.items():
        assert v <= BOUND, (what, k, v)


@pytest.mark.parametrize("i", range(len(uc.CASES)))
def test_matches_float64(i):
    c = uc.case(i)
    assert c['margin'] >= uc.MARGIN
    a, b = c['a'].cuda(), c['b'].cuda()
    loss, ga, gb = _run(a, b, c['size'], c['align'])
    assert ga.shape == a.shape and gb.shape == b.shape and ga.dtype == gb.dtype == torch.float32
    _check(c, loss, ga, gb, f"case {i} {uc.CASES[i]}")
    assert torch.equal(gb, -ga)                                          # bit for bit
    loss2, ga2, gb2 = _run(a, b, c['size'], c['align'])                  # no atomics, fixed-order sums: the same bits twice
    assert torch.equal(loss, loss2) and torch.equal(ga, ga2) and torch.equal(gb, gb2)
    # channels_last operands (what the network hands over) are used in place and give the same bits
    loss3, ga3, gb3 = _run(a.contiguous(memory_format=torch.channels_last), b.contiguous(memory_format=torch.channels_last),
                           c['size'], c['align'])
    assert torch.equal(loss, loss3) and torch.equal(ga, ga3) and torch.equal(gb, gb3)


def test_channel_slices_in_place():
    """case 1 with both operands as channels [32:96] of 128-channel channels_last tensors: the pixel stride is not C"""
    from openess_amd import hip
    c = uc.case(uc.SLICE_CASE)
    lo, hi = uc.SLICE_AT, uc.SLICE_AT + c['a'].shape[1]
    ops = []
    for t in (c['a'], c['b']):
        big = torch.full((t.shape[0], uc.SLICE_OF, t.shape[2], t.shape[3]), float('nan')).cuda().contiguous(memory_format=torch.channels_last)
        big[:, lo:hi] = t.cuda()
        ops.append(big[:, lo:hi])
    an = hip._nhwc_any(ops[0])
    assert an.data_ptr() == ops[0].data_ptr() and hip._pix_stride(an) == uc.SLICE_OF          # no copy was made
    loss, ga, gb = _run(ops[0], ops[1], c['size'], c['align'])
    _check(c, loss, ga, gb, "case 1, channel slices")
    ref = _run(c['a'].cuda(), c['b'].cuda(), c['size'], c['align'])
    assert torch.equal(loss, ref[0]) and torch.equal(ga, ref[1]) and torch.equal(gb, ref[2])


def test_refused_channel_count_falls_back():
    """case 2 with C = 6: the entries refuse it, hip.l1_mean serves it and must still match"""
    from openess_amd import hip
    c = uc.case(uc.FALLBACK_CASE, C=uc.FALLBACK_C)
    assert not hip.upsampled_l1_supported(uc.FALLBACK_C, c['a'].shape[2:], c['size'])
    loss, ga, gb = _run(c['a'].cuda(), c['b'].cuda(), c['size'], c['align'])
    _check(c, loss, ga, gb, "case 2, C = 6 (fallback)")


@pytest.mark.parametrize("need", [(True, False), (False, True)])
def test_one_sided_gradient(need):
    c = uc.case(3)
    loss, ga, gb = _run(c['a'].cuda(), c['b'].cuda(), c['size'], c['align'], need=need)
    full = _run(c['a'].cuda(), c['b'].cuda(), c['size'], c['align'])
    assert torch.equal(loss, full[0])
    for got, want, needed in ((ga, full[1], need[0]), (gb, full[2], need[1])):
        assert (got is None) if not needed else torch.equal(got, want)


def test_node_returns_none_for_an_operand_without_gradient():
    """autograd drops whatever a node returns for an input that needs nothing, so the node's backward is called by hand"""
    from openess_amd import hip
    c = uc.case(3)

    class Ctx:
        saved_tensors = tuple(hip._nhwc_any(c[k].cuda()) for k in ('a', 'b'))
        meta = (c['size'][0], c['size'][1], int(c['align']))
    g = torch.ones((), device='cuda')
    full = _run(c['a'].cuda(), c['b'].cuda(), c['size'], c['align'])
    for need in ((True, False), (False, True), (False, False)):
        Ctx.needs_input_grad = need + (False, False, False)
        out = hip._UpsampledL1Mean.backward(Ctx, g)
        assert len(out) == 5 and out[2:] == (None, None, None)
        for got, want, needed in zip(out[:2], full[1:], need):
            assert (got is None) if not needed else torch.equal(got, want)


def test_raw_entries_refuse_geometry():
    from openess_amd import _lib
    lib = _lib.load()
    EINVAL = -22                                                          # OESS_EINVAL of include/oess.h
    B, C, h, w, Ho, Wo = 1, 8, 2, 3, 4, 6
    a = torch.zeros(B, h, w, C, device='cuda')
    ga = torch.zeros_like(a)
    g = torch.ones(1, device='cuda')
    loss = torch.zeros(1, device='cuda')
    ws = torch.zeros(1 << 12, dtype=torch.uint8, device='cuda')
    st = torch.cuda.current_stream().cuda_stream

    def fwd(C=C, h=h, w=w, Ho=Ho, Wo=Wo, aps=C, bps=C):
        return lib.oess_upsampled_l1_fwd_f32(a.data_ptr(), aps, a.data_ptr(), bps, B, h, w, C, Ho, Wo, 0, ws.data_ptr(), ws.numel(),
                                             loss.data_ptr(), st)

    def bwd(C=C, h=h, w=w, Ho=Ho, Wo=Wo, aps=C, gaps=C):
        return lib.oess_upsampled_l1_bwd_f32(a.data_ptr(), aps, a.data_ptr(), C, B, h, w, C, Ho, Wo, 0, g.data_ptr(), ga.data_ptr(), gaps,
                                             None, C, st)
    assert fwd() == 0 and bwd() == 0                                      # the accepted geometry, for contrast
    for kw in (dict(C=6), dict(C=1028), dict(Ho=1), dict(Wo=2), dict(aps=4), dict(h=0)):
        assert fwd(**kw) == EINVAL, kw
    assert fwd(bps=4) == EINVAL
    assert lib.oess_upsampled_l1_workspace_bytes(B, h, w, 6, Ho, Wo) == 0 < lib.oess_upsampled_l1_workspace_bytes(B, h, w, C, Ho, Wo)
    for kw in (dict(C=6), dict(C=1028), dict(Ho=1), dict(Wo=2), dict(aps=4), dict(gaps=4), dict(h=0)):
        assert bwd(**kw) == EINVAL, kw
    torch.cuda.synchronize()
