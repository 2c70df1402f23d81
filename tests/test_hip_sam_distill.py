"""K34: hip.sam_distill_loss, the SAM distillation loss of the frame2recon pre-training step as one node on the two small maps
(openess_amd/csrc/sam_distill.hip), against the float64 restatement of the reference's lines in tests/sam_distill_reference.py.

Cases and conditioning: sam_distill_reference.CASES, each with an fp32 and a bf16 student map (the reference then runs on the
bf16-rounded values); every interpolated norm exceeds 1e-3, asserted on the float64 side, so no pixel is near the eps clamp.
Bounds: four times torch's own fp32-against-float64 figure on these cases, the worst over the cases, as
tools/exp_sam_distill_bounds.py prints them (FIG below):
    |loss - loss64| <= 4 FIG_LOSS
    |g - g64|       <= 4 FIG_GRAD max|g64|  (+ 2^-8 |g64| elementwise for a bf16 map: one rounding of the stored gradient)
Measured on the MI355X: DESIGN.md K34."""
import pytest
import torch

from tests import sam_distill_reference as sr

pytestmark = pytest.mark.gpu
# tools/exp_sam_distill_bounds.py, "worst" rows: (loss, grad) for an fp32 / a bf16 student map
FIG = {False: (1.123e-07, 1.453e-06), True: (1.365e-07, 1.516e-06)}
VARIANTS = [(i, align, bf16) for i, align in sr.variants() for bf16 in (False, True)]


def _run(sam, amap, size, align, need_grad=True):
    """(loss, grad of the map) of hip.sam_distill_loss on device operands (logical NCHW)"""
    from openess_amd import hip
    a = amap.detach().requires_grad_(need_grad)
    loss = hip.sam_distill_loss(sam, hip.UpsampledFeature(a, size, align))
    if need_grad:
        loss.backward()
    return loss.detach(), a.grad


def _operands(c, bf16):
    return c['sam'].cuda(), c['map'].cuda().to(torch.bfloat16 if bf16 else torch.float32)


def _check(loss, grad, loss64, grad64, bf16, what, roundings=1):
    fl, fg = FIG[bf16]
    el = abs(float(loss.double().cpu()) - float(loss64))
    d = (grad.double().cpu() - grad64).abs()
    allowed = 4 * fg * grad64.abs().max() + (roundings * 2.0 ** -8 * grad64.abs() if bf16 else 0)
    print(f"sam_distill {what}: loss err {el:.3e} (bound {4 * fl:.3e})  grad err {float(d.max() / grad64.abs().max()):.3e} rel max "
          f"(fp32 part of the bound {4 * fg:.3e}), worst excess ratio {float((d / allowed).max()):.3f}")
    assert el <= 4 * fl, (what, el)
    assert bool((d <= allowed).all()), (what, float((d / allowed).max()))


def _sliced(t):
    """t as channels [8, 8 + C) of a NaN-filled channels_last buffer with C + 24 channels"""
    B, C, H, W = t.shape
    big = torch.full((B, C + sr.SLICE_EXTRA, H, W), float('nan'), dtype=t.dtype, device=t.device).contiguous(memory_format=torch.channels_last)
    big[:, sr.SLICE_OFFSET:sr.SLICE_OFFSET + C] = t
    return big[:, sr.SLICE_OFFSET:sr.SLICE_OFFSET + C]


@pytest.mark.parametrize("i,align,bf16", VARIANTS)
def test_matches_float64(i, align, bf16):
    from openess_amd import hip
    c = sr.case(i, bf16, align)
    sam, amap = _operands(c, bf16)
    assert hip.sam_distill_supported(amap.shape[1], amap.shape[2:], c['size'])           # the fused node, not the fallback
    loss, grad = _run(sam, amap, c['size'], align)
    assert grad.shape == amap.shape and grad.dtype == amap.dtype and loss.dtype == torch.float32
    _check(loss, grad, c['loss'], c['grad'], bf16, f"case {i} align={int(align)} {'bf16' if bf16 else 'fp32'}")
    loss2, grad2 = _run(sam, amap, c['size'], align)                                      # no atomics, fixed-order sums
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    loss3, _ = _run(sam, amap, c['size'], align, need_grad=False)                         # the forward without the planes
    assert torch.equal(loss, loss3)
    # both maps as channel slices of NaN-filled buffers: pixel stride C + 24, used in place
    ssam, smap = _sliced(sam), _sliced(amap)
    if amap.shape[2] * amap.shape[3] > 1:
        an = hip._nhwc_any(smap)
        assert an.data_ptr() == smap.data_ptr() and hip._pix_stride(an) == amap.shape[1] + sr.SLICE_EXTRA
    loss4, grad4 = _run(ssam, smap, c['size'], align)
    _check(loss4, grad4, c['loss'], c['grad'], bf16, f"case {i} align={int(align)} {'bf16' if bf16 else 'fp32'}, channel slices")
    assert torch.equal(loss, loss4) and torch.equal(grad, grad4)


@pytest.mark.parametrize("i,align,bf16", VARIANTS)
def test_fused_against_composed(i, align, bf16, monkeypatch):
    """the sibling: the same operands through bilinear_resize, the crop and cosine_mean_loss (what refused geometry falls back to)"""
    from openess_amd import hip
    c = sr.case(i, bf16, align)
    sam, amap = _operands(c, bf16)
    loss, grad = _run(sam, amap, c['size'], align)
    monkeypatch.setattr(hip, 'sam_distill_supported', lambda *a: False)
    loss_c, grad_c = _run(sam, amap, c['size'], align)
    _check(loss_c, grad_c, c['loss'], c['grad'], bf16, f"case {i} composed vs float64")
    _check(loss, grad, loss_c.double().cpu(), grad_c.double().cpu(), bf16, f"case {i} fused vs composed",
           roundings=2)                         # two bf16-stored gradients against each other: one rounding each


def test_plain_tensor_takes_the_composed_route():
    from openess_amd import hip
    c = sr.case(2)
    sam, amap = _operands(c, False)
    a = amap.detach().requires_grad_(True)
    loss = hip.sam_distill_loss(sam, hip.bilinear_resize(a, size=c['size']))
    loss.backward()
    _check(loss.detach(), a.grad, c['loss'], c['grad'], False, "case 2, plain tensor")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_zero_student_map_gives_exactly_one(dtype):
    c = sr.case(4)
    loss, _ = _run(c['sam'].cuda(), torch.zeros_like(c['map']).cuda().to(dtype), c['size'], False, need_grad=False)
    assert float(loss) == 1.0


def test_peak_memory_stays_below_one_full_resolution_tensor():
    from openess_amd import hip
    B, C, (h, w), (H, W) = 2, 256, (7, 10), (110, 160)
    g = torch.Generator().manual_seed(34)
    amap = torch.randn(B, C, h, w, generator=g).cuda().bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    sam = (1 + 0.5 * torch.randn(B, C, 64, 64, generator=g)).cuda()
    hip._workspace(1, amap.device, tag="upsampled_cosine")             # the cached workspace is live before the call, as in a run
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = hip.sam_distill_loss(sam, hip.UpsampledFeature(amap, (H, W)))
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"sam_distill peak above live: {peak} bytes; one bf16 tensor: {B * C * H * W * 2}")
    assert peak < B * C * H * W * 2
    assert bool(torch.isfinite(amap.grad.float()).all())


def test_wrapper_refusals_leave_the_operands_alone():
    from openess_amd import hip
    sam = torch.ones(2, 8, 4, 4, device='cuda')
    a = torch.randn(2, 8, 3, 4, device='cuda', requires_grad=True)
    feat = hip.UpsampledFeature(a, (6, 8))
    for bad_sam, bad_feat in ((sam.cpu(), feat), (sam, a.detach().cpu()), (sam.double(), feat), (sam.bfloat16(), feat), (sam[0], feat),
                              (sam, a.detach()[0]), (sam[:1], feat), (sam[:, :4], feat), (sam, hip.UpsampledFeature(a, (9, 8))),
                              (sam, a.detach().half())):
        with pytest.raises(ValueError):
            hip.sam_distill_loss(bad_sam, bad_feat)
    assert a.grad is None and bool((sam == 1).all())


def test_raw_entries_refuse_and_write_nothing():
    from openess_amd import _lib
    lib = _lib.load()
    EINVAL = -22                                                          # OESS_EINVAL of include/oess.h
    B, C, h, w, Ho, Wo, ht, wt, M = 1, 8, 2, 3, 4, 6, 5, 5, 6
    a = torch.ones(B, h, w, C, device='cuda')
    t = torch.ones(B, ht, wt, C, device='cuda')
    nws = lib.oess_upsampled_cosine_workspace_bytes(B, h, w, C, Ho, Wo)
    npl = lib.oess_upsampled_cosine_planes_floats(B, Ho, Wo)
    assert nws > 0 and npl == 2 * B * Ho * Wo and lib.oess_upsampled_cosine_workspace_bytes(B, h, w, 6, Ho, Wo) == 0
    ws = torch.full((nws,), 7, dtype=torch.uint8, device='cuda')
    planes = torch.full((npl,), -3.0, device='cuda')
    loss = torch.full((1,), -3.0, device='cuda')
    ga = torch.full((B, h, w, C), -3.0, device='cuda')
    g = torch.ones(1, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    ok = dict(a=a.data_ptr(), t=t.data_ptr(), C=C, h=h, w=w, Ho=Ho, Wo=Wo, ht=ht, wt=wt, Mh=M, Mw=M, aps=C, tps=C, gaps=C, B=B,
              ws=ws.data_ptr(), nws=nws, loss=loss.data_ptr(), planes=planes.data_ptr(), g=g.data_ptr(), ga=ga.data_ptr())

    def fwd(**kw):
        k = dict(ok, **kw)
        return lib.oess_upsampled_cosine_fwd(k['a'], 0, k['aps'], k['t'], k['tps'], k['B'], k['h'], k['w'], k['C'], k['Ho'], k['Wo'], 0, k['ht'],
                                             k['wt'], k['Mh'], k['Mw'], 1e-8, k['ws'], k['nws'], k['planes'], k['loss'], st)

    def bwd(**kw):
        k = dict(ok, **kw)
        return lib.oess_upsampled_cosine_bwd(k['a'], 0, k['aps'], k['t'], k['tps'], k['B'], k['h'], k['w'], k['C'], k['Ho'], k['Wo'], 0, k['ht'],
                                             k['wt'], k['Mh'], k['Mw'], k['planes'], k['g'], k['ga'], k['gaps'], st)
    common = (dict(a=None), dict(t=None), dict(C=6), dict(C=1028, aps=1028, tps=1028, gaps=1028), dict(Ho=1), dict(Wo=2), dict(aps=4),
              dict(tps=7), dict(h=0), dict(w=-1), dict(B=0), dict(ht=0), dict(wt=-2), dict(Mh=3), dict(Mw=5))
    for kw in common + (dict(ws=None), dict(loss=None), dict(nws=nws - 1), dict(nws=0)):
        assert fwd(**kw) == EINVAL, kw
    for kw in common + (dict(planes=None), dict(g=None), dict(ga=None), dict(gaps=4)):
        assert bwd(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert bool((ws == 7).all()) and bool((planes == -3).all()) and float(loss) == -3 and bool((ga == -3).all())
    assert fwd() == 0 and bwd() == 0                                      # the accepted geometry, for contrast
    torch.cuda.synchronize()
    assert abs(float(loss)) < 1e-6 and bool((ga != -3).all())             # ones against ones: cos = 1
