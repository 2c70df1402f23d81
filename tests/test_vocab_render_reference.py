"""The restatement of the open-vocabulary render contracts (tests/vocab_render_reference.py) pinned without a GPU:
(a) against an explicit torch float64 composition -- a loop of torch.maximum into -inf planes per class, as the reference's
pseudo-label writer merges its 36 names into 11 classes; (b) the PASCAL-VOC palette rule; (c) build_vocabulary's offsets; (d) the
bound constants against what tools/exp_vocab_render_bounds.py measures; (e) for every label-compared case of the fused head, the
share of pixels whose float64 top-2 class margin lies within the value bound -- the share the GPU test may skip, capped at 1 %."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import segment_render_cases as sc
from tests import vocab_render_cases as vc
from tests import vocab_render_reference as vr


def _merge_like_the_writer(v, offsets):
    """[B, K, H, W]: planes of -inf, torch.maximum with every member in turn (generate_pl_dsec.py's merge)"""
    out = torch.full((v.shape[0], len(offsets) - 1) + tuple(v.shape[2:]), float('-inf'), dtype=v.dtype)
    for k, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        for p in range(a, b):
            out[:, k] = torch.maximum(out[:, k], v[:, p])
    return out


def test_the_vocabularies_are_what_the_issue_lists():
    assert vc.VOCABULARIES[36] == [0, 1, 3, 4, 9, 12, 13, 14, 19, 32, 33, 36] and len(vc.SIZES_36) == 11
    assert vc.VOCABULARIES[300][-1] == 300 and len(vc.VOCABULARIES[300]) == 256 and vc.VOCABULARIES[255] == [0, 255]
    for P, offs in vc.VOCABULARIES.items():
        assert offs[0] == 0 and offs[-1] == P and all(b > a for a, b in zip(offs, offs[1:]))
    # the global-tap case exceeds the LDS budget of two source rows, every other case fits
    over = [(P, shape) for P, shape, size, _ in vc.GROUP_CASES if size is not None and 2 * shape[3] * P * 4 > 48 * 1024]
    assert over == [(300, (1, 300, 2, 25))]


@pytest.mark.parametrize("P,shape,size,align", vc.GROUP_CASES, ids=[vc.group_case_id(*c) for c in vc.GROUP_CASES])
def test_grouped_restatement_equals_the_writers_merge(P, shape, size, align):
    offs = vc.VOCABULARIES[P]
    x = sc.logits(shape, "fp32")
    got = vr.grouped_render(x.numpy(), offs, size, align)
    # the merge itself is exact on the restatement's own float32 name values
    want = _merge_like_the_writer(torch.from_numpy(got['values']), offs)
    assert np.array_equal(got['classes'], want.numpy()) and np.array_equal(got['argmax'], want.argmax(1).numpy())
    # ... and the whole against torch in float64 (the float32 blend moves a confidence by less than the figure)
    v64 = x.double() if size is None else F.interpolate(x.double(), size=size, mode='bilinear', align_corners=align)
    c64 = _merge_like_the_writer(v64, offs)
    d = float(np.abs(got['conf'] - c64.softmax(1).max(1).values.numpy()).max())
    assert got['conf'].dtype == np.float64 and d <= vc.GROUP_CONF_FIGURE, d


def test_group_amax_follows_torch_on_non_finite_members():
    v = torch.randn(1, 5, 2, 3, generator=torch.Generator().manual_seed(2))
    v[0, 1, 0, 0], v[0, 3, 0, 1], v[0, 4, 0, 2], v[0, 0, 1, 0] = float('nan'), float('inf'), float('-inf'), float('nan')
    v[0, 2, 1, 0] = float('nan')
    offs = [0, 1, 5]
    c = vr.group_amax(v.numpy(), offs)
    want = torch.stack([v[:, a:b].amax(1) for a, b in zip(offs[:-1], offs[1:])], 1)
    assert np.array_equal(c, want.numpy(), equal_nan=True)
    from tests import argmax_labels_reference as ar
    assert np.array_equal(ar.first_argmax(c), want.argmax(1).numpy())


@pytest.mark.parametrize("dtype", vc.DTYPES)
@pytest.mark.parametrize("name,P,offs", vc.RANDOM_CASES, ids=[c[0] for c in vc.RANDOM_CASES])
def test_head_restatement_and_the_share_of_near_ties(name, P, offs, dtype):
    x, w, b = vc.random_case(P, dtype)
    got = vr.head_render(x.numpy(), w.numpy(), b.numpy(), offs)
    v64 = F.conv2d(x.double(), w.double()[:, :, None, None], b.double())
    c64 = _merge_like_the_writer(v64, offs)
    assert np.allclose(got['values'], v64.numpy(), rtol=0, atol=1e-13)
    assert np.array_equal(got['argmax'], c64.argmax(1).numpy())
    assert np.allclose(got['conf'], c64.softmax(1).max(1).values.numpy(), rtol=0, atol=1e-14)
    near = got['margin'] <= vc.pixel_bound(got['scale'])
    share = float(near.mean())
    print(f"{name}-{dtype}: {int(near.sum())} of {near.size} pixels within the value bound ({share:.4f}); "
          f"largest bound {float(vc.pixel_bound(got['scale']).max()):.3e}, smallest margin {float(got['margin'].min()):.3e}")
    assert share <= vc.SKIP_CAP
    assert len(np.unique(got['argmax'])) > 2                              # the labels are not one class


@pytest.mark.parametrize("dtype", vc.DTYPES)
@pytest.mark.parametrize("W", vc.EXACT_W)
@pytest.mark.parametrize("C", vc.EXACT_C)
def test_exact_cases_are_exact_in_float32(C, W, dtype):
    x, w, b, offs, _ = vc.exact_case(C, W, dtype)
    assert torch.equal(x, x.to(torch.bfloat16).float())                   # the bf16 form holds the same integers
    v64 = vr.head_values64(x.numpy(), w.numpy(), None if b is None else b.numpy())
    assert np.array_equal(v64[0], np.round(v64[0])) and float(v64[1].max()) < 2 ** 24
    acc = np.zeros(v64[0].shape, np.float32) if b is None else np.broadcast_to(b.numpy()[None, :, None, None], v64[0].shape).copy()
    for c in range(C):                                                    # the kernel's chain, one float32 operation per step
        acc = (w.numpy()[None, :, c, None, None] * x.numpy()[:, None, c] + acc).astype(np.float32)
    assert np.array_equal(acc.astype(np.float64), v64[0])


def test_cases_module_holds_the_measured_figures():
    worst = vc.measure_figures()
    print({k: f"{v[0]:.3e} at {v[1]}" for k, v in worst.items()})
    # torch's CPU kernels may vectorise differently on another host: a recorded figure has to be of the measured size
    for key, const, bound in (('group_conf', vc.GROUP_CONF_FIGURE, vc.GROUP_CONF_BOUND), ('head_conf', vc.HEAD_CONF_FIGURE, vc.HEAD_CONF_BOUND),
                              ('value', vc.VALUE_FIGURE, vc.VALUE_BOUND)):
        assert 0.5 * const <= worst[key][0] <= 2.0 * const and bound == 4.0 * const, key


def test_voc_palette_rule():
    from openess_amd.inference import voc_palette
    pal = voc_palette(255)
    assert pal.dtype == np.uint8 and pal.shape == (255, 3)
    # the first colours of the PASCAL-VOC devkit's colour map
    assert pal[:8].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128], [128, 0, 128], [0, 128, 128],
                                [128, 128, 128]]
    assert pal[8].tolist() == [64, 0, 0] and pal[15].tolist() == [192, 128, 128] and pal[20].tolist() == [0, 64, 128]
    assert len({tuple(c) for c in pal.tolist()}) == 255                   # 255 different colours
    assert np.array_equal(voc_palette(11), pal[:11])                      # a prefix: deterministic, no file


def test_build_vocabulary_offsets():
    from openess_amd.models.clip_text import build_prompts, build_vocabulary, parse_classes
    classes = ["road", ["car", "a cab", "vehicle"], "person"]
    templates = ["a photo of a {}.", "{} on the road"]
    prompts, name_offsets, class_offsets, names = build_vocabulary(classes, templates)
    assert names == [["road"], ["car", "a cab", "vehicle"], ["person"]]
    assert class_offsets.tolist() == [0, 1, 4, 5] and class_offsets.dtype == torch.int64
    assert name_offsets.tolist() == [0, 2, 4, 6, 8, 10] and len(prompts) == 10
    assert prompts[2] == "a photo of a car." and prompts[5] == "a cab on the road"
    # the same prompts, in the same order, as K29's pooled form: only the grouping differs
    assert prompts == build_prompts(classes, templates)[0]
    assert parse_classes("road, car|a cab|vehicle ,person") == classes
    for bad in ([], [[]], ["road", ""], [["car", 3]]):
        with pytest.raises(ValueError):
            build_vocabulary(bad, templates)
