"""GPU tests of the open vocabulary: Segmenter.set_vocabulary / set_vocabulary_embeddings / reset_vocabulary,
SemSegE2VID.head_features / compose_vocabulary, deeplabv3_resnet50.logits_at_stride(text_embeddings=...) and tools/segment.py
--classes, on the synthetic fine-tune YAML (64 x 96, batch 2) with seeded weights.

frame2recon runs the kernels and operands of the path without a vocabulary: equalities.  The event student's fused head forms its
logits by an fmaf chain where forward_fp32 runs a convolution kernel: its labels are compared wherever the float64 top-2 class
margin of the composed head exceeds the pixel's value bound (tests/vocab_render_cases.py VALUE_BOUND times the scale of the terms),
and the share of pixels left out is capped."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import yaml

from tests import clip_text_reference as cr
from tests import vocab_render_cases as vc
from tests import vocab_render_reference as vr
from tests.synth import damp_residual, fill_by_name

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CFG = os.path.join(HERE, "configs", "finetune_dsec_synthetic.yaml")
SEEDS = {'front_sensor_b': 11, 'back_end': 12, 'model_recon': 16}
H, W, NWIN, BINS, K = 64, 96, 3, 5, 11
GROUPS = [0, 2, 3, 7]                            # 7 names, 3 classes
SKIP_CAP = vc.SKIP_CAP                           # share of pixels whose margin may lie within the value bound: the kernel tests' 1 %


def _segmenter(option, precision, tmp_path, linear_probing=False, settings=CFG):
    from openess_amd.inference import Segmenter
    seg = Segmenter(settings, option, precision=precision, linear_probing=linear_probing, ckpt_dir=str(tmp_path))
    for name, m in seg.trainer.models_dict.items():
        fill_by_name(m, SEEDS[name])
        if name != 'model_recon':
            damp_residual(m)
    return seg


def _events(B=2, seed=4):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, NWIN * BINS, H, W, generator=g) * (torch.rand(B, NWIN * BINS, H, W, generator=g) > 0.7)).contiguous().cuda()


def _unit_rows(P, seed):
    t = torch.randn(P, 512, generator=torch.Generator().manual_seed(seed))
    return (t / t.norm(dim=1, keepdim=True)).cuda()


def _same(a, b, keys=('labels', 'conf', 'rgb')):
    return all(torch.equal(a[k], b[k]) for k in keys)


def _group_amax(v, offs):
    return torch.stack([v[:, a:b].amax(1) for a, b in zip(offs[:-1], offs[1:])], 1)


def _sure_pixels(seg, ev, T, offs):
    """(bool [B, H, W] numpy: the float64 top-2 class margin of the composed head on the student's own head operand exceeds the
    pixel's value bound, the float64 labels there)"""
    back = seg.trainer.models_dict['back_end']
    with torch.no_grad():
        x, _ = seg._event_logits(ev, False, False, head_operand=True)
    w, b = back.compose_vocabulary(T)
    ref = vr.head_render(x.float().cpu().numpy(), w.cpu().numpy(), b.cpu().numpy(), offs)
    return ref['margin'] > vc.pixel_bound(ref['scale']), ref['argmax']


# ------------------------------------------------------------------------------------------- the checkpoint's own embeddings
def test_frame2recon_with_its_own_embeddings_is_the_plain_prediction(tmp_path):
    for precision in ('bf16', 'fp32'):
        seg = _segmenter('frame2recon', precision, tmp_path)
        model = seg.trainer.models_dict['model_recon']
        batch = (None, None, torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(4)).cuda())
        plain = seg.predict(batch)
        own = model.classifier.text_embeddings.detach().clone()
        version = model.classifier.text_embeddings._version
        seg.set_vocabulary_embeddings(own, palette=seg.palette)
        assert seg.num_classes == K
        assert _same(seg.predict(batch), plain)                          # same kernels, same operands
        assert torch.equal(model.logits_at_stride(batch[2], precision, text_embeddings=own), model.logits_at_stride(batch[2], precision))
        assert model.classifier.text_embeddings._version == version and torch.equal(model.classifier.text_embeddings, own)
        seg.reset_vocabulary()
        assert _same(seg.predict(batch), plain)


def test_event_student_with_its_own_embeddings_agrees_outside_the_margin(tmp_path):
    seg = _segmenter('frame2voxel', 'fp32', tmp_path)
    back = seg.trainer.models_dict['back_end']
    ev = _events()
    plain = seg.predict((ev, None, None))
    own = back.text_embeddings.detach().clone()
    seg.set_vocabulary_embeddings(own, palette=seg.palette)
    got = seg.predict((ev, None, None))
    sure, labels64 = _sure_pixels(seg, ev, own, list(range(K + 1)))
    skipped = 1.0 - float(sure.mean())
    print(f"[open vocabulary] event student, own embeddings: skipped share {skipped:.4f}", flush=True)
    assert skipped <= SKIP_CAP and len(np.unique(labels64)) > 1
    assert np.array_equal(got['labels'].cpu().numpy()[sure], plain['labels'].cpu().numpy()[sure])
    assert np.array_equal(got['labels'].cpu().numpy()[sure], labels64[sure])
    assert torch.equal(got['rgb'], seg.palette[got['labels'].long()])
    assert torch.equal(back.text_embeddings, own)


# ------------------------------------------------------------------------------------------------- 7 names in 3 classes
def test_frame2recon_seven_names_three_classes(tmp_path):
    from openess_amd import hip
    from openess_amd.inference import voc_palette
    seg = _segmenter('frame2recon', 'bf16', tmp_path)
    model = seg.trainer.models_dict['model_recon']
    img = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(4)).cuda()
    batch = (None, None, img)
    plain = seg.predict(batch)
    T = _unit_rows(7, seed=21)
    seg.set_vocabulary_embeddings(T, GROUPS, names=[["road", "street"], "car", ["person", "man", "woman", "child"]])
    assert seg.num_classes == 3 and np.array_equal(seg.palette.cpu().numpy(), voc_palette(3))
    assert [c['names'] for c in seg.vocabulary] == [["road", "street"], ["car"], ["person", "man", "woman", "child"]]
    got = seg.predict(batch)
    # the explicit composition: forward against the stacked matrix, amax per group, argmax
    own = model.classifier.text_embeddings
    model.classifier.text_embeddings = T
    model.classifier._pw_text.key = None                                  # (the cached operand is keyed by the buffer's version alone)
    try:
        with torch.no_grad():
            full = model(img)[0]
    finally:
        model.classifier.text_embeddings = own
        model.classifier._pw_text.key = None
    assert full.shape == (2, 7, H, W)
    want = _group_amax(full, GROUPS).argmax(1)
    assert torch.equal(got['labels'].long(), want) and len(torch.unique(want)) > 1
    assert torch.equal(got['rgb'], seg.palette[got['labels'].long()])
    # merged by the maximum, not by K29's mean of the embeddings
    low = model.logits_at_stride(img, 'bf16', text_embeddings=T)
    assert low.shape == (2, 7, H // 16, W // 16)
    assert torch.equal(got['labels'], hip.segment_render(low, size=(H, W), class_offsets=GROUPS, want=('labels',))['labels'])
    seg.reset_vocabulary()
    assert seg.num_classes == K and _same(seg.predict(batch), plain)


def test_event_student_seven_names_three_classes_and_the_states(tmp_path):
    seg = _segmenter('frame2voxel', 'fp32', tmp_path)
    back = seg.trainer.models_dict['back_end']
    ev = _events()
    plain = seg.predict((ev, None, None))
    T = _unit_rows(7, seed=22) * 8.0                                       # (any rows: a larger scale spreads the classes)
    seg.set_vocabulary_embeddings(T, GROUPS)
    got = seg.predict((ev, None, None))
    assert seg.num_classes == 3 and got['labels'].shape == (2, H, W) and int(got['labels'].max()) <= 2
    # the explicit composition: forward_fp32 against the stacked matrix, amax per group, argmax
    own = back.text_embeddings
    back.text_embeddings = T
    back._pw32_head.key = None                                            # (the cached operand is keyed by version counters alone)
    try:
        with torch.no_grad():
            full, _ = seg._event_logits(ev, False, False)
    finally:
        back.text_embeddings = own
        back._pw32_head.key = None
    assert full.shape == (2, 7, H, W)
    want = _group_amax(full, GROUPS).argmax(1).cpu().numpy()
    sure, labels64 = _sure_pixels(seg, ev, T, GROUPS)
    skipped = 1.0 - float(sure.mean())
    print(f"[open vocabulary] event student, 7 names: skipped share {skipped:.4f}", flush=True)
    assert skipped <= SKIP_CAP and len(np.unique(want)) > 1
    assert np.array_equal(got['labels'].cpu().numpy()[sure], want[sure]) and np.array_equal(want[sure], labels64[sure])
    # the stateful path carries its states across a vocabulary change
    one = ev[:1].contiguous()
    seg.reset()
    for i in range(NWIN):
        under_vocab = seg.predict_events(one[:, i * BINS:(i + 1) * BINS].contiguous(), stateful=True)
    assert _same(under_vocab, seg.predict_events(one))
    seg.reset()
    seg.predict_events(one[:, :BINS].contiguous(), stateful=True)
    seg.reset_vocabulary()                                                 # 11 classes from here on, the same recording
    seg.predict_events(one[:, BINS:2 * BINS].contiguous(), stateful=True)
    last = seg.predict_events(one[:, 2 * BINS:].contiguous(), stateful=True)
    seg.reset()
    assert seg.num_classes == K and _same(last, seg.predict_events(one))
    assert _same(seg.predict((ev, None, None)), plain)                     # the earlier bits


def test_event_student_above_the_lds_budget_takes_the_head_conv(tmp_path):
    """400 names at 32 channels exceed vocab_render's 372: the composed head runs as a convolution, the grouped render follows"""
    from openess_amd import hip
    seg = _segmenter('frame2voxel', 'fp32', tmp_path)
    assert hip.vocab_render_max_names(32) == 372
    ev = _events()
    T = _unit_rows(400, seed=23) * 8.0
    offs = list(range(0, 401, 2))                                          # 200 classes of two names
    seg.set_vocabulary_embeddings(T, offs)
    assert not seg._vocab.fused and seg.num_classes == 200
    got = seg.predict((ev, None, None))
    sure, labels64 = _sure_pixels(seg, ev, T, offs)
    assert 1.0 - float(sure.mean()) <= SKIP_CAP
    assert np.array_equal(got['labels'].cpu().numpy()[sure], labels64[sure])
    seg.set_vocabulary_embeddings(T[:372], offs[:187])                     # at the budget: the fused pass
    assert seg._vocab.fused and seg.num_classes == 186


# ---------------------------------------------------------------------------------------------------------- CLIP end to end
def _clip_files(tmp_path):
    return cr.write_synthetic_checkpoint(tmp_path / "clip.pt"), cr.write_merges(tmp_path / "merges.txt")


def test_set_vocabulary_end_to_end(tmp_path):
    from openess_amd.models.clip_text import compute_text_embeddings
    ckpt, bpe = _clip_files(tmp_path)
    classes = ["road", ["car", "a cab"], "broad road"]
    seg = _segmenter('frame2recon', 'bf16', tmp_path)
    batch = (None, None, torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(4)).cuda())
    with pytest.raises(ValueError, match="clip_text_checkpoint"):
        seg.set_vocabulary(classes)                                       # the YAML names no CLIP files
    seg.set_vocabulary(classes, merge='mean', clip_text_checkpoint=ckpt, clip_bpe_path=bpe)
    mean = seg.predict(batch)
    assert seg.num_classes == 3 and seg._vocab.P == 3
    assert [c['names'] for c in seg.vocabulary] == [["road"], ["car", "a cab"], ["broad road"]]
    rows = compute_text_embeddings(ckpt, bpe, classes, 'single', 'cuda')
    assert torch.equal(seg._vocab.T.cpu(), rows)
    seg.set_vocabulary_embeddings(rows)
    assert _same(seg.predict(batch), mean)
    seg.set_vocabulary(classes, merge='max', clip_text_checkpoint=ckpt, clip_bpe_path=bpe)
    assert seg.num_classes == 3 and seg._vocab.P == 4 and seg._vocab.offsets == [0, 1, 3, 4]
    # one unit row per name: the singleton classes keep K29's rows, the two names of `car` stay apart
    T = seg._vocab.T.cpu()
    assert torch.allclose(T[0], rows[0], atol=1e-6) and torch.allclose(T[3], rows[2], atol=1e-6) and float((T[1] - T[2]).abs().max()) > 1e-3
    assert torch.allclose(T.norm(dim=1), torch.ones(4), atol=1e-5)
    out = seg.predict(batch)
    assert out['labels'].shape == (2, H, W) and int(out['labels'].max()) <= 2


# ----------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_classes_writes_the_vocabulary_and_labels_in_it(tmp_path, capsys):
    from PIL import Image
    spec = importlib.util.spec_from_file_location("segment_tool", os.path.join(ROOT, "tools", "segment.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ckpt, bpe = _clip_files(tmp_path)
    out = tmp_path / "out"
    res = tool.main(["-o", str(out), "--classes", "road,car|a cab,broad road", "--clip-text-checkpoint", ckpt, "--bpe", bpe,
                     "--min-conf", "0.34", "--max-frames", "2"])
    rec = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    assert rec == json.loads(json.dumps(res)) and rec['frames'] == 2 and rec['classes'] == 3
    assert 'miou' not in rec and 'acc' not in rec and rec['vocabulary'] == {"merge": "max", "templates": "single"}
    vocab = json.load(open(out / "vocabulary.json"))
    assert [c['id'] for c in vocab] == [0, 1, 2] and [c['names'] for c in vocab] == [["road"], ["car", "a cab"], ["broad road"]]
    assert [c['color'] for c in vocab] == [[0, 0, 0], [128, 0, 0], [0, 128, 0]]
    files = sorted(os.listdir(out / "labels"))
    assert len(files) == 2
    for f in files:
        with Image.open(out / "labels" / f) as im:
            lab = np.asarray(im)
        assert lab.shape == (H, W) and bool(np.isin(lab, [0, 1, 2, 255]).all())
    # the YAML's keys serve as the defaults of the two paths
    cfg = yaml.load(open(CFG), yaml.Loader)
    cfg['clip'].update(clip_text_checkpoint=ckpt, clip_bpe_path=bpe)
    (tmp_path / "with_clip.yaml").write_text(yaml.dump(cfg))
    (tmp_path / "classes.txt").write_text("road\ncar|a cab\n")
    tool.main(["-o", str(tmp_path / "again"), "--settings", str(tmp_path / "with_clip.yaml"), "--classes", str(tmp_path / "classes.txt"),
               "--merge", "mean", "--max-frames", "1"])
    rec = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    assert rec['classes'] == 2 and rec['vocabulary']['merge'] == "mean" and 'miou' not in rec
