"""GPU tests of flip and multi-scale inference: Segmenter.predict / predict_events with flip= and scales=, and
tools/segment.py --tta / --tta-scales, on the geometry of tests/test_hip_inference.py (2 x 64 x 96, three sub-windows, seeded
weights).  Everything here is an equality: a prediction under flip / scales is hip.ensemble_render of the logits the plain path's
own calls give on the mirrored / rescaled input, bit for bit, and the defaults are the plain prediction."""
import json
import os

import pytest
import torch

from tests import test_hip_inference as ti

pytestmark = pytest.mark.gpu
H, W, NWIN, BINS, K = ti.H, ti.W, ti.NWIN, ti.BINS, ti.K
SCALES = (0.75, 1.0, 1.25)


def _image(seed=4):
    return torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(seed)).cuda()


# --------------------------------------------------------------------------------------------------------------- frame2recon
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_frame2recon_is_the_ensemble_of_its_views(precision, tmp_path):
    from openess_amd import hip
    from openess_amd.inference import tta_views
    seg = ti._segmenter('frame2recon', precision, tmp_path)
    model = seg.trainer.models_dict['model_recon']
    img = _image()
    batch = (None, None, img)
    grey = torch.randint(0, 256, (2, H, W), generator=torch.Generator().manual_seed(6), dtype=torch.int64).to(torch.uint8).cuda()
    kw = dict(min_conf=0.125, background=grey, alpha=0.25)                 # seeded weights: confidences of 0.12 ... 0.14 over 11 classes
    rkw = dict(size=(H, W), palette=seg.palette, ignore_label=seg.ignore_label, **kw)
    # the defaults are today's prediction
    plain = seg.predict(batch, **kw)
    assert ti._same(plain, hip.segment_render(model.logits_at_stride(img, precision), **rkw))
    assert ti._same(seg.predict(batch, flip=False, scales=(1.0,), **kw), plain)
    # flip
    low = [model.logits_at_stride(img, precision), model.logits_at_stride(img.flip(-1), precision)]
    assert torch.equal(low[0], model.logits_at_stride(img, precision))                 # view 0's logits are the plain path's
    flipped = seg.predict(batch, flip=True, **kw)
    assert ti._same(flipped, hip.ensemble_render(low, flips=[False, True], **rkw))
    assert not torch.equal(flipped['conf'], plain['conf']) and len(torch.unique(flipped['labels'])) > 1
    # three scales, each with its mirror image
    views = tta_views(True, SCALES)
    assert len(views) == 6 and views[0] == (1.0, False)
    lows = []
    for scale, mirrored in views:
        x = img if scale == 1.0 else hip.bilinear_resize(img, size=(int(H * scale + 0.5), int(W * scale + 0.5)))
        lows.append(model.logits_at_stride(x.flip(-1) if mirrored else x, precision))
    assert len({tuple(v.shape[-2:]) for v in lows}) == 3
    multi = seg.predict(batch, flip=True, scales=SCALES, **kw)
    assert ti._same(multi, hip.ensemble_render(lows, flips=[m for _, m in views], **rkw))
    assert not torch.equal(multi['conf'], flipped['conf'])
    assert ti._same(seg.predict(batch, **kw), plain)                                    # and the plain path is left as it was


def test_frame2recon_flip_needs_less_memory_than_the_composed_form(tmp_path):
    from openess_amd import hip
    seg = ti._segmenter('frame2recon', 'bf16', tmp_path)
    model = seg.trainer.models_dict['model_recon']
    img = _image(7)
    batch = (None, None, img)

    def composed():
        p = 0
        for mirrored in (False, True):
            low = model.logits_at_stride(img.flip(-1) if mirrored else img, 'bf16')
            q = hip.bilinear_resize(low.float(), size=(H, W)).softmax(1)
            p = p + (q.flip(-1) if mirrored else q)
        conf, labels = (p / 2).max(1)
        return labels.to(torch.uint8), conf, seg.palette[labels]

    got, want = seg.predict(batch, flip=True), composed()                  # (both ran once: workspaces and operands exist)
    assert float((got['conf'] - want[1]).abs().max()) <= 1e-5               # the two forms compute the same thing
    peak_composed = ti._peak(composed)
    peak_predict = ti._peak(lambda: seg.predict(batch, flip=True))
    print(f"[tta] frame2recon bf16 2 x {H} x {W} flip: peak bytes predict {peak_predict}, composed form {peak_composed}", flush=True)
    assert peak_predict < peak_composed


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_linear_probe_flips_its_full_resolution_logits_and_refuses_scales(precision, tmp_path):
    from openess_amd import hip
    seg = ti._segmenter('frame2recon', precision, tmp_path, linear_probing=True)
    img = _image(5)
    batch = (None, None, img)
    with torch.no_grad():
        full = [seg.trainer.val_logits(batch, precision), seg.trainer.val_logits((None, None, img.flip(-1)), precision)]
    assert full[0].shape == (2, K, H, W)
    want = hip.ensemble_render(full, flips=[False, True], palette=seg.palette, ignore_label=seg.ignore_label)
    assert ti._same(seg.predict(batch, flip=True), want)
    with pytest.raises(ValueError, match="linear probe"):
        seg.predict(batch, scales=SCALES)
    with pytest.raises(ValueError, match="linear probe"):
        seg.predict(batch, flip=True, scales=(1.0, 0.5))


# ------------------------------------------------------------------------------------------------------------ event students
@pytest.mark.parametrize("front,precision", [("convlstm", "bf16"), ("convlstm", "fp32"), ("convgru", "bf16")])
def test_event_student_flip_is_the_ensemble_of_the_tensor_and_its_mirror_image(front, precision, tmp_path):
    from openess_amd import hip
    from tests.synth import damp_residual, fill_by_name
    gru = front == "convgru"
    seg = ti._segmenter('frame2voxel', precision, tmp_path, settings=ti._gru_settings(tmp_path) if gru else ti.CFG, fill=not gru)
    if gru:
        fill_by_name(seg.trainer.models_dict['back_end'], ti.SEEDS['back_end'])
        damp_residual(seg.trainer.models_dict['back_end'])
    ev = ti._events()
    rkw = dict(palette=seg.palette, ignore_label=seg.ignore_label)
    with torch.no_grad():
        logits = [seg.trainer.val_logits((e, None, None), precision).float() for e in (ev, ev.flip(-1).contiguous())]
    plain = seg.predict((ev, None, None))
    assert ti._same(plain, hip.segment_render(logits[0], **rkw))
    want = hip.ensemble_render(logits, flips=[False, True], **rkw)
    got = seg.predict((ev, None, None), flip=True)
    assert ti._same(got, want) and ti._same(seg.predict_events(ev, flip=True), want)
    assert not torch.equal(got['conf'], plain['conf']) and len(torch.unique(got['labels'])) > 1
    assert ti._same(seg.predict_events(ev, flip=False, scales=(1.0,)), plain)
    with pytest.raises(ValueError, match="flip only"):
        seg.predict_events(ev, scales=SCALES)
    # one recording under flip: a state set per view
    one = ev[:1].contiguous()
    stateless = seg.predict_events(one, flip=True)
    first = seg.predict_events(one, stateful=True, flip=True)
    assert ti._same(first, stateless) and seg._states is not None and seg._mirror_states is not None
    second = seg.predict_events(one, stateful=True, flip=True)
    assert not torch.equal(second['conf'], stateless['conf'])
    seg.reset()
    assert seg._states is None and seg._mirror_states is None
    assert ti._same(seg.predict_events(one, stateful=True, flip=True), stateless)
    seg.reset()
    # the overlay and the reconstruction come from view 0
    recon = seg.predict_events(one, want_recon=True)['recon']
    over = seg.predict_events(one, background='recon', alpha=0.25, flip=True, want_recon=True)
    assert torch.equal(over['recon'], recon) and torch.equal(over['labels'], stateless['labels'])
    c = seg.palette[over['labels'].long()].int()
    assert torch.equal(over['rgb'].int(), (64 * c + 192 * recon[..., None].int() + 128) >> 8)


def test_flip_inference_disturbs_no_trainer(tmp_path):
    """two train steps of a fine-tune trainer, with and without flip predictions of a Segmenter between them"""
    import train
    from openess_amd.config.settings import Settings

    def run(with_tta):
        train.seed_everything()
        s = Settings(ti.CFG, generate_log=False)
        s.ckpt_dir, s.config_option = str(tmp_path), "frame2voxel"
        s.if_finetuning, s.if_linear_probing, s.if_supervised_only = True, False, False
        trainer, _ = train.build_trainer(s)
        ti._fill(trainer.models_dict)
        ev = ti._events()
        gt = torch.randint(0, K, (2, H // 4, W // 4), generator=torch.Generator().manual_seed(8)).repeat_interleave(4, 1).repeat_interleave(4, 2).cuda()
        b = (ev, gt, None, gt, gt, None)
        losses = [trainer.train_step(b)[2].clone()]
        if with_tta:
            seg = ti._segmenter('frame2voxel', 'bf16', tmp_path)
            seg.predict(b, flip=True)
            seg.predict_events(ev[:1].contiguous(), stateful=True, want_recon=True, flip=True)
            assert all(len(opt.state) == 0 for opt in seg.trainer.optimizers_dict.values())
        losses.append(trainer.train_step(b)[2].clone())
        return losses, [p.detach().clone() for p in trainer.task_backend.parameters()]

    plain, with_tta = run(False), run(True)
    assert all(torch.equal(a, b) for a, b in zip(plain[0], with_tta[0]))
    assert all(torch.equal(a, b) for a, b in zip(plain[1], with_tta[1]))


# ----------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_scores_the_ensembles_labels_on_the_validation_split(tmp_path, capsys):
    from openess_amd.evaluation.metrics import MetricsSemseg
    out_dir = tmp_path / "out"
    res = ti._tool().main(["-o", str(out_dir), "--tta", "flip"])
    rec = ti._json_line(capsys)
    assert rec == json.loads(json.dumps(res)) and rec['tta'] == {"flip": True, "scales": [1.0], "views": 2} and rec['frames'] > 0
    seg = ti._segmenter('frame2voxel', 'bf16', tmp_path, fill=False)
    tr, s = seg.trainer, seg.settings
    met = MetricsSemseg(s.semseg_num_classes, s.semseg_ignore_label, s.semseg_class_names)
    stems, differs = [], False
    for sample in tr.val_loader_sensor_b:
        batch = tr.prepare_batch(sample, 'val')[:-4]
        stems += [os.path.splitext(os.path.basename(str(p)))[0] for p in sample[-1]]
        labels = seg.predict(batch, flip=True)['labels']
        differs = differs or not torch.equal(labels, seg.predict(batch)['labels'])
        met.update_batch(labels, batch[1])
    assert differs                                                         # the ensemble is not the plain prediction
    for sub in ('labels', 'color'):                                        # the stems of the plain run (test_hip_inference.py)
        assert sorted(os.listdir(out_dir / sub)) == sorted(st + '.png' for st in stems)
    summary = met.get_metrics_summary()
    assert float(summary['miou']) == rec['miou'] and float(summary['acc']) == rec['acc']
    assert summary['cm'].tolist() == rec['confusion']


def test_cli_segments_a_recording_statefully_under_flip(tmp_path, capsys):
    tool = ti._tool()
    n_per, windows = 700, 4
    path = ti._events_file(tmp_path, n_per * windows)
    runs = {}
    for name, flags in (("plain", []), ("flip", ["--tta", "flip"])):
        out = tmp_path / name
        tool.main(["-o", str(out), "-i", path, "-N", str(n_per), "--stateful"] + flags)
        runs[name] = (ti._json_line(capsys), out)
    assert runs["plain"][0]['tta'] == {"flip": False, "scales": [1.0], "views": 1}
    assert runs["flip"][0]['tta'] == {"flip": True, "scales": [1.0], "views": 2}
    assert runs["flip"][0]['frames'] == runs["plain"][0]['frames'] == windows
    want = ['frame_{:010d}.png'.format(k) for k in range(windows)]
    for name, (_, out) in runs.items():
        assert sorted(os.listdir(out / 'labels')) == want and sorted(os.listdir(out / 'color')) == want
    files = {name: [open(out / 'labels' / f, 'rb').read() for f in want] for name, (_, out) in runs.items()}
    assert files["plain"] != files["flip"]                                 # the ensemble is not the plain prediction
