"""GPU tests of the inference path: deeplabv3_resnet50.logits_at_stride, openess_amd.inference.Segmenter and
tools/segment.py on the synthetic fine-tune YAML (64 x 96, three sub-windows), with seeded weights.  Everything here is an equality:
the render's labels are the argmax of the logits the trainers validate with, bit for bit."""
import importlib.util
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml

from tests import pretrained_cases as pc
from tests.synth import damp_residual, fill_by_name

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CFG = os.path.join(HERE, "configs", "finetune_dsec_synthetic.yaml")
SEEDS = {'front_sensor_b': 11, 'back_end': 12, 'model_recon': 16}
H, W, NWIN, BINS, K = 64, 96, 3, 5, 11


def _fill(models):
    for name, m in models.items():
        fill_by_name(m, SEEDS[name])
        if name != 'model_recon':
            damp_residual(m)


def _segmenter(option, precision, tmp_path, linear_probing=False, settings=CFG, fill=True):
    from openess_amd.inference import Segmenter
    seg = Segmenter(settings, option, precision=precision, linear_probing=linear_probing, ckpt_dir=str(tmp_path))
    if fill:
        _fill(seg.trainer.models_dict)
    return seg


def _events(B=2, seed=4):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, NWIN * BINS, H, W, generator=g) * (torch.rand(B, NWIN * BINS, H, W, generator=g) > 0.7)).contiguous().cuda()


def _same(a, b, keys=('labels', 'conf', 'rgb')):
    return all(torch.equal(a[k], b[k]) for k in keys)


def _peak(fn):
    """peak bytes allocated by fn() above what is allocated before it (fn already ran once: workspaces and operands exist)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


# --------------------------------------------------------------------------------------------------------------- frame2recon
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_frame2recon_renders_the_argmax_of_forward_from_the_stride_level_logits(precision, tmp_path):
    from openess_amd import hip
    seg = _segmenter('frame2recon', precision, tmp_path)
    model = seg.trainer.models_dict['model_recon']
    assert not model.training and not any(m.training for m in model.modules())
    img = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(4)).cuda()
    batch = (None, None, img)
    with torch.no_grad():
        full = (model(img) if precision == 'bf16' else model.forward_fp32(img))[0]
        val = seg.trainer.val_logits(batch, precision)
    low = model.logits_at_stride(img, precision)
    # output_stride: 32 dilates layer4 only: the network's stride is 16
    assert low.dtype == torch.float32 and low.shape == (2, K, H // 16, W // 16) and not low.requires_grad
    labels = hip.segment_render(low, size=(H, W), want=('labels',))['labels']
    assert torch.equal(labels.long(), full.argmax(1)) and torch.equal(labels.long(), val.argmax(1))
    assert len(torch.unique(labels)) > 1
    out = seg.predict(batch)
    assert torch.equal(out['labels'], labels) and out['rgb'].shape == (2, H, W, 3) and out['conf'].shape == (2, H, W)
    assert torch.equal(out['rgb'], seg.palette[out['labels'].long()])
    # nothing of the full resolution but the outputs: less memory than the validation forward
    with torch.no_grad():
        peak_val = _peak(lambda: seg.trainer.val_logits(batch, precision).argmax(1))
    peak_predict = _peak(lambda: seg.predict(batch))
    print(f"[inference] frame2recon {precision} 2 x {H} x {W}: peak bytes predict {peak_predict}, val_logits + argmax {peak_val}", flush=True)
    assert peak_predict < peak_val


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_frame2recon_linear_probe_takes_the_full_resolution_path(precision, tmp_path):
    seg = _segmenter('frame2recon', precision, tmp_path, linear_probing=True)
    model = seg.trainer.models_dict['model_recon']
    assert model.if_linear_probing
    img = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(5)).cuda()
    batch = (None, None, img)
    with torch.no_grad():
        want = seg.trainer.val_logits(batch, precision).argmax(1)
    assert torch.equal(seg.predict(batch)['labels'].long(), want)
    with pytest.raises(NotImplementedError, match="linear probe"):
        model.logits_at_stride(img, precision)
    with pytest.raises(ValueError, match="event students"):
        seg.predict_events(_events())


# --------------------------------------------------------------------------------------------------------------- frame2voxel
def _gru_settings(tmp_path):
    path = str(tmp_path / "gru.pth.tar")
    pc.write_e2vid(path, pc.GRU, seed=45)
    cfg = yaml.load(open(CFG), yaml.Loader)
    cfg['clip'].update(e2vid_checkpoint=path)
    out = tmp_path / "gru.yaml"
    out.write_text(yaml.dump(cfg))
    return str(out)


@pytest.mark.parametrize("front,precision", [("convlstm", "bf16"), ("convlstm", "fp32"), ("convgru", "bf16")])
def test_event_student_predicts_the_argmax_of_val_logits_and_carries_state(front, precision, tmp_path):
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor, PostProcessor
    gru = front == "convgru"
    seg = _segmenter('frame2voxel', precision, tmp_path, settings=_gru_settings(tmp_path) if gru else CFG, fill=not gru)
    if gru:
        fill_by_name(seg.trainer.models_dict['back_end'], SEEDS['back_end'])
        damp_residual(seg.trainer.models_dict['back_end'])
    front_end = seg.trainer.models_dict['front_sensor_b']
    assert getattr(front_end, 'recurrent_block_type', 'convlstm') == front
    ev = _events()
    batch = (ev, None, None)
    with torch.no_grad():
        want = seg.trainer.val_logits(batch, precision).argmax(1)
    out = seg.predict(batch)
    assert torch.equal(out['labels'].long(), want) and len(torch.unique(want)) > 1
    assert _same(out, seg.predict_events(ev))
    # one recording: the first stateful call is the stateless one, the second is not, reset() starts over
    one = ev[:1].contiguous()
    stateless = seg.predict_events(one)                 # (not compared with out[:1]: another batch size may take other conv routes)
    first = seg.predict_events(one, stateful=True)
    assert _same(first, stateless)
    second = seg.predict_events(one, stateful=True)
    assert not torch.equal(second['conf'], stateless['conf'])
    assert _same(seg.predict_events(one), stateless)                      # a stateless call in between starts from empty states
    third = seg.predict_events(one, stateful=True)                         # ... and leaves the recording's states alone
    assert not torch.equal(third['conf'], stateless['conf']) and not torch.equal(third['conf'], second['conf'])
    seg.reset()
    assert _same(seg.predict_events(one, stateful=True), stateless)
    seg.reset()
    # one window per call through the stateful path = the sub-windows of one tensor
    for i in range(NWIN):
        last = seg.predict_events(one[:, i * BINS:(i + 1) * BINS].contiguous(), stateful=True)
    assert _same(last, stateless)
    seg.reset()
    with pytest.raises(ValueError, match="batch size 1"):
        seg.predict_events(ev, stateful=True)
    with pytest.raises(ValueError, match="sub-windows"):
        seg.predict_events(one[:, :BINS].contiguous())
    # the E2VID image of the last sub-window, as reconstruct() / process_u8 give it for the same windows
    with_recon = seg.predict_events(one, want_recon=True)
    assert _same(with_recon, stateless)
    opts = SimpleNamespace(**dict(vars(seg.settings.e2vid_config), precision=precision))
    rec = ImageReconstructor(front_end, H, W, BINS, seg.device, opts)
    for i in range(NWIN):
        img, _, _ = rec.update_reconstruction(one[:, i * BINS:(i + 1) * BINS].contiguous(), reconstruct=True)
    grey = PostProcessor(seg.device).process_u8(img[:, :1])
    assert with_recon['recon'].dtype == torch.uint8 and with_recon['recon'].shape == (1, H, W)
    assert torch.equal(with_recon['recon'], grey) and len(torch.unique(grey)) > 4
    over = seg.predict_events(one, background='recon', alpha=0.25)
    assert torch.equal(over['labels'], stateless['labels']) and not torch.equal(over['rgb'], stateless['rgb'])
    c = seg.palette[over['labels'].long()].int()
    assert torch.equal(over['rgb'].int(), (64 * c + 192 * grey[..., None].int() + 128) >> 8)


def test_a_segmenter_disturbs_no_trainer(tmp_path):
    """two train steps of a fine-tune trainer, with and without a Segmenter built and used between them: the same losses and weights"""
    import train
    from openess_amd.config.settings import Settings

    def run(with_segmenter):
        train.seed_everything()
        s = Settings(CFG, generate_log=False)
        s.ckpt_dir, s.config_option = str(tmp_path), "frame2voxel"
        s.if_finetuning, s.if_linear_probing, s.if_supervised_only = True, False, False
        trainer, _ = train.build_trainer(s)
        _fill(trainer.models_dict)
        ev = _events()
        gt = torch.randint(0, K, (2, H // 4, W // 4), generator=torch.Generator().manual_seed(8)).repeat_interleave(4, 1).repeat_interleave(4, 2).cuda()
        b = (ev, gt, None, gt, gt, None)
        losses = [trainer.train_step(b)[2].clone()]
        modes = [m.training for net in trainer.models_dict.values() for m in net.modules()]
        if with_segmenter:
            seg = _segmenter('frame2voxel', 'bf16', tmp_path)
            seg.predict(b)
            seg.predict_events(ev[:1].contiguous(), stateful=True, want_recon=True)
            assert all(len(opt.state) == 0 for opt in seg.trainer.optimizers_dict.values())
            assert not any(m.training for net in seg.trainer.models_dict.values() for m in net.modules())
        assert [m.training for net in trainer.models_dict.values() for m in net.modules()] == modes
        losses.append(trainer.train_step(b)[2].clone())
        return losses, [p.detach().clone() for p in trainer.task_backend.parameters()]

    plain, with_seg = run(False), run(True)
    assert all(torch.equal(a, b) for a, b in zip(plain[0], with_seg[0]))
    assert all(torch.equal(a, b) for a, b in zip(plain[1], with_seg[1]))
    assert not torch.equal(plain[0][0], plain[0][1])


# ----------------------------------------------------------------------------------------------------------------------- CLI
def _tool():
    spec = importlib.util.spec_from_file_location("segment_tool", os.path.join(ROOT, "tools", "segment.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _json_line(capsys):
    return json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])


def test_cli_writes_the_validation_split_and_reports_the_trainers_miou(tmp_path, capsys):
    from PIL import Image
    from openess_amd import hip
    out_dir = tmp_path / "out"
    res = _tool().main(["-o", str(out_dir), "--save-confidence"])
    rec = _json_line(capsys)
    assert rec == json.loads(json.dumps(res)) and rec['source'] == 'val' and rec['frames'] > 0
    assert set(rec['ms_per_frame']) == {'network', 'render', 'write'} and all(v > 0 for v in rec['ms_per_frame'].values())
    print("[inference] segment.py --split val:", json.dumps({k: v for k, v in rec.items() if k != 'confusion'}), flush=True)
    # the same split through a Segmenter of the same settings: stems, labels and the trainer's own validation
    seg = _segmenter('frame2voxel', 'bf16', tmp_path, fill=False)
    tr = seg.trainer
    stems, labels = [], []
    for sample in tr.val_loader_sensor_b:
        batch = tr.prepare_batch(sample, 'val')[:-4]
        stems += [os.path.splitext(os.path.basename(str(p)))[0] for p in sample[-1]]
        labels.append(seg.predict(batch)['labels'])
    labels = torch.cat(labels)
    assert len(set(stems)) == len(stems) == rec['frames']
    for sub, ext in (('labels', '.png'), ('color', '.png'), ('confidence', '.npy')):
        assert sorted(os.listdir(out_dir / sub)) == sorted(s + ext for s in stems)
    datas = [open(out_dir / 'labels' / (s + '.png'), 'rb').read() for s in stems]
    blob = torch.from_numpy(np.frombuffer(b"".join(datas), np.uint8).copy()).cuda()
    maps, status = hip.png_decode_gray8_batch(blob, [len(d) for d in datas], H, W)
    assert not bool(status.any()) and torch.equal(maps, labels.long())
    with Image.open(out_dir / 'labels' / (stems[0] + '.png')) as im:
        assert im.mode == 'L' and im.size == (W, H)
    with Image.open(out_dir / 'color' / (stems[0] + '.png')) as im:
        assert im.mode == 'RGB' and im.size == (W, H)
        assert np.array_equal(np.asarray(im), seg.palette[labels[0].long()].cpu().numpy())
    conf = np.load(out_dir / 'confidence' / (stems[0] + '.npy'))
    assert conf.dtype == np.float32 and conf.shape == (H, W) and 0 < conf.min() and conf.max() <= 1
    summary = tr.valEpochs()
    assert float(summary['miou']) == rec['miou'] and float(summary['acc']) == rec['acc']
    assert summary['cm'].tolist() == rec['confusion']


def _events_file(tmp_path, n, seed=5):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0.0, 0.2, n))
    ev = np.stack([t, rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n)], 1)
    path = str(tmp_path / "events.txt")
    with open(path, "w") as f:
        f.write(f"{W} {H}\n")
        for r in ev:
            f.write("%.9f %d %d %d\n" % (r[0], r[1], r[2], r[3]))
    return path


def test_cli_segments_an_event_recording(tmp_path, capsys):
    tool = _tool()
    n_per, windows = 700, 7                                                # 7 windows of 700 events: two groups of three, one left over
    path = _events_file(tmp_path, n_per * windows)
    runs = {}
    for name, flags in (("plain", []), ("stateful", ["--stateful"]), ("overlay", ["--overlay", "recon"])):
        out = tmp_path / name
        tool.main(["-o", str(out), "-i", path, "-N", str(n_per)] + flags)
        runs[name] = (_json_line(capsys), out)
    rec = runs["plain"][0]
    assert rec['source'] == path and rec['frames'] == windows // NWIN and rec['events_per_window'] == n_per
    assert runs["stateful"][0]['frames'] == windows and runs["stateful"][0]['windows_per_frame'] == 1
    assert runs["overlay"][0]['frames'] == rec['frames']
    for name, (r, out) in runs.items():
        want = ['frame_{:010d}.png'.format(k) for k in range(r['frames'])]
        assert sorted(os.listdir(out / 'labels')) == want and sorted(os.listdir(out / 'color')) == want
        assert not (out / 'confidence').exists()
    for k in range(rec['frames']):
        f = 'frame_{:010d}.png'.format(k)
        same = [open(runs[name][1] / sub / f, 'rb').read() for name in ("plain", "overlay") for sub in ('labels', 'color')]
        assert same[0] == same[2] and same[1] != same[3]                   # the overlay changes color/, not labels/
    limited = tmp_path / "limited"
    tool.main(["-o", str(limited), "-i", path, "-N", str(n_per), "--stateful", "--max-frames", "2", "--skipevents", "100"])
    assert _json_line(capsys)['frames'] == 2 and len(os.listdir(limited / 'labels')) == 2
