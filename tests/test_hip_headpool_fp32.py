"""GPU tests of the fused fp32 head-pool node (K20, openess_amd/csrc/headpool_f32.hip, hip._BilinearL2NormPoolF32 behind
hip.UpsampledNormalizedFeature.pool on an fp32 map): k = scatter_mean(F.normalize(Upsample(x4, bilinear, align_corners=True)(x)))
and its input gradient against float64 autograd of the reference ops (F.interpolate, F.normalize, index_add_, / (count + 1e-6)),
inputs built as tests/test_hip_losses.py::test_upsampled_normalized_feature_pool builds them (tests/pretrain_fp32_cases.py).

Bounds (the rule of K16 - K19): four times the largest error torch's OWN fp32 CPU autograd of the same ops reaches against float64 on
the same cases, floor 1e-5; measured by tools/exp_pretrain_fp32_bounds.py.  k and grad_x by max|a - a64| / max|a64|, the zero-norm
case's grad_x and the convolution's tensors by |a - a64|_2 / |a64|_2.

    figure                                   torch fp32 CPU     bound      MI355X
    k, five cases + three variants           9.3e-07            1e-5       9.6e-07
    grad_x, five cases + two variants        1.28e-06           1e-5       1.28e-06
    grad_x, zero-norm case, L2 ratio         1.6e-07            1e-5       1.7e-07
    fused against the materialised chain     (same bound)       1e-5       1.1e-07 (k), 1.8e-07 (grad_x)
    head conv 2048 -> 256: y, dx, dw, db     5.2e-07            1e-5       5.7e-07
"""
import pytest
import torch

from tests import pretrain_fp32_cases as pc

pytestmark = pytest.mark.gpu
BOUND = 1e-5
_REF = {}


def _report(name, value):
    print(f"[headpool_fp32] {name}: {value:.3e} (bound {BOUND:.0e})", flush=True)
    return value


def _case(key):
    """inputs (CPU) and the float64 reference of a case or variant, computed once"""
    if key not in _REF:
        if isinstance(key, str):
            v = pc.HEADPOOL_VARIANTS[key]
            inp = pc.headpool_inputs(*v[:4], sps=v[4], nids=v[5], S=v[6], zero_block=v[7])
        else:
            inp = pc.headpool_inputs(*key)
        _REF[key] = (inp, pc.headpool_reference(*inp, torch.float64))
    return _REF[key]


def _run(x, sp, sps, S, gk, fused=True):
    """(k, count | None, grad_x) of the node (or of the materialised fp32 chain) on the GPU"""
    from openess_amd import hip
    xg = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    feat = hip.UpsampledNormalizedFeature(xg, pc.SCALE)
    cnt = None
    if fused:
        k, cnt = feat.pool(sp.cuda(), sps, S, with_count=True)
    else:
        k = hip.superpixel_pool(feat.materialize(), sp.cuda(), sps, S)
    k.backward(gk.cuda())
    return k.detach().cpu(), None if cnt is None else cnt.cpu(), xg.grad.cpu()


@pytest.mark.parametrize("case", pc.HEADPOOL_CASES)
def test_fused_node_matches_float64_and_the_materialised_chain(case):
    (x, sp, sps, S, gk), (k64, cnt64, g64) = _case(tuple(case))
    k, cnt, gx = _run(x, sp, sps, S, gk)
    assert k.dtype == torch.float32 and gx.dtype == torch.float32 and gx.shape == x.shape
    assert torch.equal(cnt.double(), cnt64)                                     # the integer pixel counts, exactly
    empty = cnt64 == 0
    assert bool(empty.any()) and float(k[empty].abs().max()) == 0.0
    ek, eg = _report(f"{case} k", pc.max_ratio(k, k64)), _report(f"{case} grad_x", pc.max_ratio(gx, g64))
    k2, cnt2, gx2 = _run(x, sp, sps, S, gk)                                     # bit-repeatable
    assert torch.equal(k, k2) and torch.equal(cnt, cnt2) and torch.equal(gx, gx2)
    km, _, gm = _run(x, sp, sps, S, gk, fused=False)                            # the composed fp32 chain on the GPU
    ekm, egm = _report(f"{case} k fused~materialised", pc.max_ratio(k, km)), _report(f"{case} grad_x fused~materialised", pc.max_ratio(gx, gm))
    assert ek <= BOUND and eg <= BOUND and ekm <= BOUND and egm <= BOUND, (ek, eg, ekm, egm)


def test_raw_ids_above_255_take_the_global_accumulators():
    (x, sp, sps, S, gk), (k64, cnt64, g64) = _case('global_route')
    assert int(sp.max()) == 299 and int((sp >= 256).sum()) > 0
    k, cnt, gx = _run(x, sp, sps, S, gk)
    assert torch.equal(cnt.double(), cnt64)
    ek, eg = _report("global route k", pc.max_ratio(k, k64)), _report("global route grad_x", pc.max_ratio(gx, g64))
    k2, _, gx2 = _run(x, sp, sps, S, gk)
    assert torch.equal(k, k2) and torch.equal(gx, gx2)
    assert ek <= BOUND and eg <= BOUND, (ek, eg)


def test_rows_beyond_S_are_ignored():
    (x, sp, sps, S, gk), (k64, cnt64, g64) = _case('rows_beyond_S')
    off = sp + torch.arange(x.shape[0])[:, None, None] * sps
    assert int(off.max()) + 1 > S and int((off >= S).sum()) > 0
    k, cnt, gx = _run(x, sp, sps, S, gk)
    assert k.shape == (S, x.shape[1]) and torch.equal(cnt.double(), cnt64) and int(cnt.sum()) == int((off < S).sum())
    ek, eg = _report("rows beyond S k", pc.max_ratio(k, k64)), _report("rows beyond S grad_x", pc.max_ratio(gx, g64))
    assert ek <= BOUND and eg <= BOUND, (ek, eg)


def test_zero_norm_pixels_take_the_clamp_branch():
    (x, sp, sps, S, gk), (k64, cnt64, g64) = _case('zero_norm')
    assert float(x[:, :, 2:4, 3:5].abs().max()) == 0.0
    assert float(g64.abs().max()) > 1e9                                         # g / eps on the zero-norm pixels: the branch is reached
    k, cnt, gx = _run(x, sp, sps, S, gk)
    ek, eg = _report("zero norm k", pc.max_ratio(k, k64)), _report("zero norm grad_x L2 ratio", pc.l2_ratio(gx, g64))
    assert bool(torch.isfinite(gx).all()) and ek <= BOUND and eg <= BOUND, (ek, eg)


def test_refusals_come_before_any_launch():
    from openess_amd import hip
    sp = torch.zeros(1, 28, 36, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="C in"):
        hip.UpsampledNormalizedFeature(torch.zeros(1, 96, 7, 9, device="cuda"), 4)
    with pytest.raises(ValueError, match="bfloat16 or float32"):
        hip.UpsampledNormalizedFeature(torch.zeros(1, 64, 7, 9, device="cuda", dtype=torch.float16), 4)
    ids = sp.reshape(-1)
    with pytest.raises(ValueError, match="float32"):                            # a bf16 map handed to the f32 node
        hip._BilinearL2NormPoolF32.apply(torch.zeros(1, 64, 7, 9, device="cuda", dtype=torch.bfloat16), 4, ids, 50, 50)
    buf = torch.zeros(1, 7, 9, 65, device="cuda")                               # pixel stride 65 floats: rows not 16-byte aligned
    x = buf[..., :64].permute(0, 3, 1, 2)
    with pytest.raises(RuntimeError, match="invalid argument"):
        hip._BilinearL2NormPoolF32.apply(x, 4, ids, 50, 50)
    torch.cuda.synchronize()


def test_a_non_finite_input_makes_the_whole_of_k_nan():
    (x, sp, sps, S, gk), _ = _case((1, 64, 7, 9))
    from openess_amd import hip
    xb = x.clone()
    xb[0, 3, 2, 4] = float('inf')
    k = hip.UpsampledNormalizedFeature(xb.cuda().contiguous(memory_format=torch.channels_last), pc.SCALE).pool(sp.cuda(), sps, S)
    assert bool(torch.isnan(k).all())


def test_teacher_head_conv_backward_at_2048_input_channels():
    from openess_amd import hip
    x, w, b, gy = pc.head_conv_inputs()
    y64, dx64, dw64, db64 = pc.head_conv_reference(x, w, b, gy, torch.float64)
    xg = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wg, bg = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = hip.conv2d_f32_train(xg, wg, bg)
    y.backward(gy.cuda().contiguous(memory_format=torch.channels_last))
    errs = {n: _report(f"head conv {n}", pc.l2_ratio(a.detach().cpu(), r))
            for n, a, r in (('y', y, y64), ('dx', xg.grad, dx64), ('dw', wg.grad, dw64), ('db', bg.grad, db64))}
    assert max(errs.values()) <= BOUND, errs
