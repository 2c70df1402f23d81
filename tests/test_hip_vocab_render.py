"""GPU tests of K36's kernels: oess_segment_render_grouped (hip.segment_render(class_offsets=...)) and oess_head_render
(hip.vocab_render) on the cases of tests/vocab_render_cases.py against the restatement of tests/vocab_render_reference.py.

  grouped  singleton groups: the bits of hip.segment_render without offsets on every K35 shape; real groups: labels torch.equal to
           hip.bilinear_resize -> per-group amax -> argmax, confidence against the float64 restatement within GROUP_CONF_BOUND =
           4 x 1.065e-07 (torch float32 against float64 on these cases, tools/exp_vocab_render_bounds.py); NaN / +-inf members, equal
           values, min_conf, the palette blend, output subsets, every refusal with the outputs untouched
  head     exact integer operands: the bits of the grouped render on torch's integer logits; random operands: labels equal the
           float64 restatement wherever its top-2 class margin exceeds the pixel's value bound (VALUE_BOUND = 4 x 2.985e-07 times
           the scale of the name values' terms; the skipped share is asserted <= 1 %), confidence within HEAD_CONF_BOUND =
           4 x 3.715e-07; peak memory below one [B, P, H, W] tensor; the LDS limit and the refusal above it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import segment_render_cases as sc
from tests import segment_render_reference as sr
from tests import vocab_render_cases as vc
from tests import vocab_render_reference as vr

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0xA5


def _dev(x, dtype):
    return x.to(torch.bfloat16 if dtype == "bf16" else torch.float32).to(DEV)


def _slice(x, dtype, lead=8, extra=24):
    """logical [B, C, h, w] device tensor: channels lead ... lead + C of a NaN-filled NHWC buffer of C + extra channels"""
    x = _dev(x, dtype)
    B, C, h, w = x.shape
    big = torch.full((B, h, w, C + extra), float('nan'), dtype=x.dtype, device=DEV)
    big[..., lead:lead + C] = x.permute(0, 2, 3, 1)
    return big[..., lead:lead + C].permute(0, 3, 1, 2)


def _group_amax(v, offs):
    return torch.stack([v[:, a:b].amax(1) for a, b in zip(offs[:-1], offs[1:])], 1)


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


# ---------------------------------------------------------------------------------------------------------------- grouped render
@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("shape,size,align", sc.ALL_SHAPES, ids=[sc.case_id(*c) for c in sc.ALL_SHAPES])
def test_singleton_groups_give_the_bits_of_the_plain_render(shape, size, align, dtype):
    from openess_amd import hip
    B, K = shape[:2]
    H, W = sc.out_size(shape, size)
    x = _dev(sc.logits(shape, dtype), dtype)
    kw = dict(size=size, align_corners=align, palette=sc.palette(K).to(DEV), background=sc.grey(B, H, W).to(DEV), alpha=0.5)
    plain = hip.segment_render(x, **kw)
    assert _same(hip.segment_render(x, class_offsets=list(range(K + 1)), **kw), plain)
    assert _same(hip.segment_render(x, class_offsets=torch.arange(K + 1), **kw), plain)


@pytest.mark.parametrize("dtype", vc.DTYPES)
@pytest.mark.parametrize("P,shape,size,align", vc.GROUP_CASES, ids=[vc.group_case_id(*c) for c in vc.GROUP_CASES])
def test_real_groups(P, shape, size, align, dtype):
    from openess_amd import hip
    offs = vc.VOCABULARIES[P]
    B, K = shape[0], len(offs) - 1
    H, W = sc.out_size(shape, size)
    x = sc.logits(shape, dtype)
    xv = _slice(x, dtype) if shape[2] == 3 else _dev(x, dtype)
    pal, grey = sc.palette(K), sc.grey(B, H, W)
    want = vr.grouped_render(x.numpy(), offs, size, align, pal.numpy(), grey.numpy(), alpha256=128)
    got = hip.segment_render(xv, size=size, align_corners=align, palette=pal.to(DEV), background=grey.to(DEV), alpha=0.5,
                             class_offsets=offs)
    assert got['labels'].shape == (B, H, W) and got['labels'].dtype == torch.uint8 and got['rgb'].shape == (B, H, W, 3)
    up = xv.float() if size is None else hip.bilinear_resize(xv.float(), size=size, align_corners=align)
    assert torch.equal(got['labels'].long(), _group_amax(up, offs).argmax(1))                 # the composed path, bit for bit
    assert np.array_equal(got['labels'].cpu().numpy(), want['labels'])
    d = float(np.abs(got['conf'].cpu().numpy().astype(np.float64) - want['conf']).max())
    print(f"{vc.group_case_id(P, shape, size, align)}-{dtype}: |conf - float64| {d:.3e} (bound {vc.GROUP_CONF_BOUND:.3e})")
    assert sc.finite_pixels(want['values']).all() and d <= vc.GROUP_CONF_BOUND
    assert np.array_equal(got['rgb'].cpu().numpy(), want['rgb'])
    again = hip.segment_render(xv, size=size, align_corners=align, palette=pal.to(DEV), background=grey.to(DEV), alpha=0.5,
                               class_offsets=offs)
    assert _same(got, again)                                              # two calls, the same bits


@pytest.mark.parametrize("size", [None, (12, 16)], ids=["same", "12x16"])
def test_non_finite_members_follow_amax_and_argmax(size):
    """NaN, +inf and -inf in members of different groups: torch.amax makes a class NaN, torch.argmax puts NaN above +inf"""
    from openess_amd import hip
    offs = vc.VOCABULARIES[36]
    x = sc.logits((2, 36, 3, 4), "fp32", seed_offset=3)
    x[0, 5, 1, 1] = float('nan')                  # class 3 (names 4 ... 8)
    x[0, 20, 1, 1] = float('inf')                 # class 8: NaN is above it
    x[1, 1, 0, 3] = float('inf')                  # class 1
    x[1, 9, 2, 0] = float('-inf')                 # class 4: its other members decide
    x[1, 0, 2, 2] = float('-inf')                 # class 0 is this one name
    x[0, 2, 0, 0], x[0, 35, 0, 0] = float('nan'), float('nan')            # classes 1 and 10: the first NaN wins
    xd = x.to(DEV)
    got = hip.segment_render(xd, size=size, class_offsets=offs, want=('labels', 'conf'))
    up = xd if size is None else hip.bilinear_resize(xd, size=size)
    c = _group_amax(up, offs)
    assert torch.equal(got['labels'].long(), c.argmax(1))
    want = vr.grouped_render(x.numpy(), offs, size)
    assert np.array_equal(got['labels'].cpu().numpy(), want['labels'])
    if size is None:
        lab = got['labels']
        assert int(lab[0, 1, 1]) == 3 and int(lab[1, 0, 3]) == 1 and int(lab[0, 0, 0]) == 1 and int(lab[1, 2, 2]) != 0
        assert float(got['conf'][1, 0, 3]) == 1.0                          # one +inf: every other term is exp(-inf) = 0
    fin = sc.finite_pixels(want['values'])
    assert 0 < fin.sum() < fin.size
    assert float(np.abs(got['conf'].cpu().numpy()[fin] - want['conf'][fin]).max()) <= vc.GROUP_CONF_BOUND
    assert bool(torch.isnan(got['conf'][torch.isnan(c).any(1)]).all())


@pytest.mark.parametrize("P", sorted(vc.VOCABULARIES))
def test_equal_values_give_label_zero_and_exactly_one_over_k(P):
    from openess_amd import hip
    offs = vc.VOCABULARIES[P]
    K = len(offs) - 1
    want = float(np.float32(1) / np.float32(K))
    for value in (0.0, -3.5):
        x = torch.full((2, P, 3, 5), value, device=DEV)
        for size in (None, (6, 11)):
            got = hip.segment_render(x, size=size, class_offsets=offs, want=('labels', 'conf'))
            assert not got['labels'].any() and bool((got['conf'] == want).all()), (P, value, size)


def test_threshold_uses_the_kernels_own_confidence_over_the_classes():
    from openess_amd import hip
    offs, shape, size = vc.VOCABULARIES[36], (2, 36, 7, 9), (28, 36)
    x = (sc.logits(shape, "fp32", seed_offset=1) * 3).to(DEV)
    pal = sc.palette(11).to(DEV)
    got = hip.segment_render(x, size=size, palette=pal, min_conf=0.5, ignore_label=200, class_offsets=offs)
    idx = _group_amax(hip.bilinear_resize(x, size=size), offs).argmax(1)
    below = got['conf'] < 0.5
    assert 0 < int(below.sum()) < below.numel()
    assert torch.equal(got['labels'].long(), torch.where(below, torch.full_like(idx, 200), idx))
    assert np.array_equal(got['rgb'].cpu().numpy(), sr.colour(got['labels'].cpu().numpy(), pal.cpu().numpy(), ignore=200))
    assert bool((got['rgb'][below] == 0).all())


def test_palette_blend_over_grey():
    from openess_amd import hip
    offs, shape, size = vc.VOCABULARIES[5], (2, 5, 5, 6), (13, 17)
    x = sc.logits(shape, "fp32") * 3
    pal, grey = sc.palette(2, seed=1), sc.grey(2, 13, 17, seed=1)
    got = hip.segment_render(x.to(DEV), size=size, palette=pal.to(DEV), background=grey.to(DEV), alpha=77 / 256, min_conf=0.7,
                             class_offsets=offs)
    labels = got['labels'].cpu().numpy()
    assert (labels == 255).any() and (labels == 0).any() and (labels == 1).any()
    assert np.array_equal(got['rgb'].cpu().numpy(), sr.colour(labels, pal.numpy(), grey.numpy(), 77))


@pytest.mark.parametrize("want", [('labels',), ('conf', 'rgb')], ids=["labels", "conf+rgb"])
def test_an_output_not_asked_for_is_never_written(want):
    from openess_amd import _lib, hip
    offs, (B, P, h, w), (H, W) = vc.VOCABULARIES[36], (2, 36, 7, 9), (28, 261)                # 261: two chunks, odd row phases
    x = sc.logits((B, P, h, w), "fp32")
    xn = x.to(DEV).permute(0, 2, 3, 1).contiguous()
    pal, grey = sc.palette(11).to(DEV), sc.grey(B, H, W).to(DEV)
    ref = vr.grouped_render(x.numpy(), offs, (H, W), False, pal.cpu().numpy(), grey.cpu().numpy(), alpha256=77)
    bufs = {'labels': torch.full((B, H, W), POISON, dtype=torch.uint8, device=DEV),
            'conf': torch.full((B, H, W), -3.0, dtype=torch.float32, device=DEV),
            'rgb': torch.full((B, H, W, 3), POISON, dtype=torch.uint8, device=DEV)}
    ptr = {k: (bufs[k].data_ptr() if k in want else None) for k in bufs}
    od = torch.tensor(offs, dtype=torch.int32, device=DEV)
    rc = _lib.load().oess_segment_render_grouped(xn.data_ptr(), 0, P, B, 11, P, h, w, H, W, 0, od.data_ptr(), pal.data_ptr(),
                                                 grey.data_ptr(), 77, 0.0, 255, ptr['labels'], ptr['conf'], ptr['rgb'], hip._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(bufs['labels'].cpu().numpy(), ref['labels']) if 'labels' in want else bool((bufs['labels'] == POISON).all())
    assert (float(np.abs(bufs['conf'].cpu().numpy() - ref['conf']).max()) <= vc.GROUP_CONF_BOUND) if 'conf' in want \
        else bool((bufs['conf'] == -3.0).all())
    assert np.array_equal(bufs['rgb'].cpu().numpy(), ref['rgb']) if 'rgb' in want else bool((bufs['rgb'] == POISON).all())
    got = hip.segment_render(xn.permute(0, 3, 1, 2), size=(H, W), palette=pal, background=grey, alpha=77 / 256, want=want,
                             class_offsets=offs)
    assert set(got) == set(want) and all(torch.equal(got[k], bufs[k]) for k in want)


def _grouped_args(B=2, K=3, P=7, h=3, w=4, H=6, W=8):
    from openess_amd import hip
    x = torch.randn(B, h, w, P + 3, device=DEV)
    outs = (torch.full((B, H, W), POISON, dtype=torch.uint8, device=DEV), torch.full((B, H, W), -3.0, device=DEV),
            torch.full((B, H, W, 3), POISON, dtype=torch.uint8, device=DEV))
    keep = (sc.palette(K).to(DEV), sc.grey(B, H, W).to(DEV), torch.tensor(vc.EXACT_GROUPS, dtype=torch.int32, device=DEV))
    a = dict(logits=x.data_ptr(), is_bf16=0, ps=P + 3, B=B, K=K, P=P, h=h, w=w, H=H, W=W, ac=0, offs=keep[2].data_ptr(),
             palette=keep[0].data_ptr(), grey=keep[1].data_ptr(), alpha256=128, min_conf=0.0, ignore=255, labels=outs[0].data_ptr(),
             conf=outs[1].data_ptr(), rgb=outs[2].data_ptr(), stream=hip._stream())
    return x, outs, keep, a


def _call_grouped(a):
    from openess_amd import _lib
    return _lib.load().oess_segment_render_grouped(a['logits'], a['is_bf16'], a['ps'], a['B'], a['K'], a['P'], a['h'], a['w'], a['H'],
                                                   a['W'], a['ac'], a['offs'], a['palette'], a['grey'], a['alpha256'], a['min_conf'],
                                                   a['ignore'], a['labels'], a['conf'], a['rgb'], a['stream'])


GROUPED_REFUSALS = {
    "null_logits": dict(logits=None), "null_offsets": dict(offs=None), "no_output": dict(labels=None, conf=None, rgb=None),
    "rgb_without_palette": dict(palette=None), "k_zero": dict(K=0), "k_256": dict(K=256, P=300, ps=300),
    "p_below_k": dict(P=2), "p_1025": dict(P=1025, ps=1025), "stride_below_p": dict(ps=6), "ignore_is_a_class": dict(ignore=2),
    "ignore_256": dict(ignore=256), "alpha_257": dict(alpha256=257), "min_conf_nan": dict(min_conf=float('nan')),
    "min_conf_negative": dict(min_conf=-0.25), "b_zero": dict(B=0), "w_in_zero": dict(w=0), "h_out_zero": dict(H=0),
    "output_rows_overflow": dict(B=1 << 16, H=1 << 16), "input_extent_overflows": dict(ps=1 << 62),
}


@pytest.mark.parametrize("name", sorted(GROUPED_REFUSALS))
def test_grouped_entry_refuses_before_any_launch(name):
    x, outs, keep, a = _grouped_args()
    assert _call_grouped(a) == 0                                          # the unmodified call is valid
    torch.cuda.synchronize()
    want = vr.grouped_render(x[..., :7].permute(0, 3, 1, 2).cpu().numpy(), vc.EXACT_GROUPS, (6, 8), False, keep[0].cpu().numpy(),
                             keep[1].cpu().numpy(), 128)
    assert np.array_equal(outs[0].cpu().numpy(), want['labels']) and np.array_equal(outs[2].cpu().numpy(), want['rgb'])
    outs[0].fill_(POISON), outs[1].fill_(-3.0), outs[2].fill_(POISON)
    assert _call_grouped(dict(a, **GROUPED_REFUSALS[name])) == -22
    torch.cuda.synchronize()
    assert bool((outs[0] == POISON).all()) and bool((outs[1] == -3.0).all()) and bool((outs[2] == POISON).all())


def test_wrapper_refuses_bad_offsets_before_any_launch():
    from openess_amd import hip
    x = torch.randn(2, 7, 3, 4, device=DEV)
    assert set(hip.segment_render(x, class_offsets=vc.EXACT_GROUPS, want=('labels',))) == {'labels'}
    for bad in ([1, 3, 7], [0, 3, 3, 7], [0, 4, 2, 7], [0, 2, 6], [0, 2, 8], [0], [], [0, 2.5, 7], [0, True, 7]):
        with pytest.raises(ValueError, match="class_offsets must start at 0"):
            hip.segment_render(x, class_offsets=bad, want=('labels',))
    with pytest.raises(ValueError, match="K <= 255"):
        hip.segment_render(torch.zeros(1, 256, 2, 2, device=DEV), class_offsets=list(range(257)), want=('labels',))
    with pytest.raises(ValueError, match="P <= 1024"):
        hip.segment_render(torch.zeros(1, 1025, 1, 1, device=DEV), class_offsets=[0, 1025], want=('labels',))
    with pytest.raises(ValueError, match="palette must be"):             # the palette has K rows, not P
        hip.segment_render(x, class_offsets=vc.EXACT_GROUPS, palette=sc.palette(7).to(DEV))
    with pytest.raises(ValueError, match="ignore_label"):
        hip.segment_render(x, class_offsets=vc.EXACT_GROUPS, ignore_label=2, want=('labels',))
    assert int(hip.segment_render(x, class_offsets=vc.EXACT_GROUPS, ignore_label=3, min_conf=2.0, want=('labels',))['labels'].min()) == 3


# -------------------------------------------------------------------------------------------------------------------- fused head
@pytest.mark.parametrize("dtype", vc.DTYPES)
@pytest.mark.parametrize("W", vc.EXACT_W)
@pytest.mark.parametrize("C", vc.EXACT_C)
def test_head_on_exact_operands_gives_the_bits_of_the_grouped_render(C, W, dtype):
    from openess_amd import hip
    x, w, b, offs, sliced = vc.exact_case(C, W, dtype)
    logits = F.conv2d(x.double(), w.double()[:, :, None, None], None if b is None else b.double()).float()       # exact integers
    K = w.shape[0] if offs is None else len(offs) - 1
    B, _, H, _ = x.shape
    kw = dict(palette=sc.palette(K).to(DEV), background=sc.grey(B, H, W).to(DEV), alpha=0.25, min_conf=0.4)
    want = hip.segment_render(logits.to(DEV), class_offsets=offs, **kw)
    xv = _slice(x, dtype, lead=3, extra=5) if sliced else _dev(x, dtype)   # a pixel stride above C, no 16-byte alignment
    got = hip.vocab_render(xv, w.to(DEV), None if b is None else b.to(DEV), class_offsets=offs, **kw)
    assert _same(got, want)
    assert _same(hip.vocab_render(xv, w.to(DEV), None if b is None else b.to(DEV), class_offsets=offs, **kw), got)


@pytest.mark.parametrize("dtype", vc.DTYPES)
@pytest.mark.parametrize("name,P,offs", vc.RANDOM_CASES, ids=[c[0] for c in vc.RANDOM_CASES])
def test_head_on_random_operands_within_the_bounds(name, P, offs, dtype):
    from openess_amd import hip
    x, w, b = vc.random_case(P, dtype)
    want = vr.head_render(x.numpy(), w.numpy(), b.numpy(), offs)
    singletons = len(offs) - 1 == P
    got = hip.vocab_render(_dev(x, dtype), w.to(DEV), b.to(DEV), class_offsets=None if singletons else offs, want=('labels', 'conf'))
    sure = want['margin'] > vc.pixel_bound(want['scale'])
    skipped = 1.0 - float(sure.mean())
    wrong = int((got['labels'].cpu().numpy()[sure] != want['argmax'][sure]).sum())
    d = float(np.abs(got['conf'].cpu().numpy().astype(np.float64) - want['conf']).max())
    print(f"{name}-{dtype}: skipped share {skipped:.4f} (cap {vc.SKIP_CAP}), wrong labels {wrong}, |conf - float64| {d:.3e} "
          f"(bound {vc.HEAD_CONF_BOUND:.3e})")
    assert skipped <= vc.SKIP_CAP and wrong == 0
    assert d <= vc.HEAD_CONF_BOUND


def test_head_forms_no_logit_tensor():
    from openess_amd import hip
    B, C, H, W, P = 2, 32, 64, 96, 128
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16).to(DEV).permute(0, 3, 1, 2)
    w, b = (0.3 * torch.randn(P, C, generator=g)).to(DEV), torch.randn(P, generator=g).to(DEV)
    offs = list(range(0, P + 1, 2))                                       # 64 classes of two names
    pal = sc.palette(64).to(DEV)
    hip.vocab_render(x, w, b, class_offsets=offs, palette=pal)            # once before: the library is loaded
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = hip.vocab_render(x, w, b, class_offsets=offs, palette=pal)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"vocab_render 2 x 32 x 64 x 96, P = 128: peak {peak} bytes; an fp32 logit tensor has {B * P * H * W * 4}")
    assert peak < B * P * H * W * 4
    logits = F.conv2d(x.float(), w[:, :, None, None], b)
    sure = vr.head_render(x.float().cpu().numpy(), w.cpu().numpy(), b.cpu().numpy(), offs)
    ok = sure['margin'] > vc.pixel_bound(sure['scale'])
    assert np.array_equal(out['labels'].cpu().numpy()[ok], sure['argmax'][ok]) and ok.mean() > 0.99
    assert float((out['labels'].long() == _group_amax(logits, offs).argmax(1)).float().mean()) > 0.99


def test_head_at_the_lds_limit_and_the_refusal_above_it():
    from openess_amd import _lib, hip
    lib = _lib.load()
    assert [hip.vocab_render_max_names(C) for C in (1, 32, 64)] == [1024 * 48 // (4 * 2), 1024 * 48 // (4 * 33), 1024 * 48 // (4 * 65)]
    assert hip.vocab_render_max_names(0) == 0 and hip.vocab_render_max_names(65) == 0
    C = 64
    P = hip.vocab_render_max_names(C)                                     # 189 names
    g = torch.Generator().manual_seed(6)
    x = torch.randint(-4, 5, (1, C, 2, 5), generator=g).float()
    w, b = torch.randint(-3, 4, (P + 1, C), generator=g).float(), torch.randint(-8, 9, (P + 1,), generator=g).float()
    logits = F.conv2d(x, w[:, :, None, None], b)
    got = hip.vocab_render(x.to(DEV), w[:P].contiguous().to(DEV), b[:P].contiguous().to(DEV), want=('labels', 'conf'))
    assert _same(got, hip.segment_render(logits[:, :P].to(DEV), want=('labels', 'conf')))
    offs = [0, P + 1]
    with pytest.raises(ValueError, match=f"at most {P} names"):
        hip.vocab_render(x.to(DEV), w.to(DEV), b.to(DEV), class_offsets=offs, want=('labels',))
    # ... which the caller answers with the logits and the grouped render
    lab = hip.segment_render(logits.to(DEV), class_offsets=offs, want=('labels',))['labels']
    assert not lab.any()
    out = torch.full((1, 2, 5), POISON, dtype=torch.uint8, device=DEV)
    xd, wd, od = x.to(DEV).permute(0, 2, 3, 1).contiguous(), w.to(DEV), torch.tensor(offs, dtype=torch.int32, device=DEV)
    rc = lib.oess_head_render(xd.data_ptr(), 0, C, 1, C, 2, 5, wd.data_ptr(), None, 1, P + 1, od.data_ptr(), None, None, 128, 0.0, 255,
                              out.data_ptr(), None, None, hip._stream())
    torch.cuda.synchronize()
    assert rc == -22 and bool((out == POISON).all())


def test_head_wrapper_and_entry_refuse_before_any_launch():
    from openess_amd import _lib, hip
    x = torch.randn(2, 8, 3, 4, device=DEV)
    w, b = torch.randn(7, 8, device=DEV), torch.randn(7, device=DEV)
    pal = sc.palette(3).to(DEV)
    ok = dict(class_offsets=vc.EXACT_GROUPS, palette=pal)
    assert set(hip.vocab_render(x, w, b, **ok)) == {'labels', 'conf', 'rgb'}
    with pytest.raises(ValueError, match="no CPU fallback"):
        hip.vocab_render(x.cpu(), w, b, **ok)
    with pytest.raises(ValueError, match="float32 / bfloat16"):
        hip.vocab_render(x.half(), w, b, **ok)
    with pytest.raises(ValueError, match="C <= 64"):
        hip.vocab_render(torch.zeros(1, 65, 2, 2, device=DEV), torch.zeros(7, 65, device=DEV), **ok)
    for bad in (w.cpu(), w.double(), w[:, :7], w.t().contiguous().t(), w[None]):
        with pytest.raises(ValueError, match="weight must be"):
            hip.vocab_render(x, bad, b, **ok)
    for bad in (b.cpu(), b[:6], b.double(), b[None]):
        with pytest.raises(ValueError, match="bias must be"):
            hip.vocab_render(x, w, bad, **ok)
    with pytest.raises(ValueError, match="class_offsets must start at 0"):
        hip.vocab_render(x, w, b, class_offsets=[0, 2, 6], palette=pal)
    with pytest.raises(ValueError, match="palette must be"):
        hip.vocab_render(x, w, b, palette=pal)                            # singletons: K = 7
    with pytest.raises(ValueError, match="K <= 255"):
        hip.vocab_render(x, torch.zeros(256, 8, device=DEV), want=('labels',))
    with pytest.raises(ValueError, match="want must name"):
        hip.vocab_render(x, w, b, want=(), **ok)
    with pytest.raises(ValueError, match="min_conf"):
        hip.vocab_render(x, w, b, min_conf=-1.0, **ok)
    out = torch.full((2, 3, 4), POISON, dtype=torch.uint8, device=DEV)
    xn, od = x.permute(0, 2, 3, 1).contiguous(), torch.tensor(vc.EXACT_GROUPS, dtype=torch.int32, device=DEV)
    f = _lib.load().oess_head_render

    def call(**kw):
        a = dict(dict(x=xn.data_ptr(), ps=8, B=2, C=8, H=3, W=4, w=w.data_ptr(), K=3, P=7, offs=od.data_ptr(), ignore=255, out=out.data_ptr()), **kw)
        return f(a['x'], 0, a['ps'], a['B'], a['C'], a['H'], a['W'], a['w'], b.data_ptr(), a['K'], a['P'], a['offs'], None, None, 128, 0.0,
                 a['ignore'], a['out'], None, None, hip._stream())
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, hip.vocab_render(x, w, b, class_offsets=vc.EXACT_GROUPS, want=('labels',))['labels'])
    out.fill_(POISON)
    for bad in (dict(x=None), dict(w=None), dict(out=None), dict(C=0), dict(C=65), dict(ps=7), dict(K=0), dict(K=8), dict(P=1025),
                dict(offs=None), dict(ignore=2), dict(B=0), dict(H=0), dict(W=-1), dict(ps=1 << 62)):
        assert call(**bad) == -22, bad
    torch.cuda.synchronize()
    assert bool((out == POISON).all())
