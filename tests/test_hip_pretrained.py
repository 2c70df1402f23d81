"""GPU tests of the pretrained-weight loading (K33): the weights a YAML names reach every kernel that reads them -- the bf16 packed
operands (engine.PackedWeight, its grouped repack included), the fp32 operands with BatchNorm folded in float64
(engine.PackedWeightF32), the fp32 reconstructor that shares the front-end module, the ConvGRU schedule.  Loading adds no kernel:
every comparison is between the same kernels on the same operands, so the same bits are required (torch.equal), never a tolerance.
Files are seeded checkpoints in the reference's layouts, written into tmp_path (tests/pretrained_cases.py).  Size of the synthetic
configs: 64 x 96, batch 2."""
import logging
from types import SimpleNamespace

import pytest
import torch

from tests import pretrained_cases as pc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def _trainer(s):
    import train
    train.seed_everything()
    return train.build_trainer(s)


def _standalone_latents(state, config, precision, ev):
    """The latents of the last sub-window from a stand-alone ImageReconstructor over a manually loaded module, by the trainers'
    own loop (three sub-windows from empty states)."""
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor
    from openess_amd.e2vid.model.model import E2VIDRecurrent
    model = E2VIDRecurrent(config)
    model.load_state_dict(state)
    model.to(DEV).eval()
    rec = ImageReconstructor(model, pc.H, pc.W, pc.BINS, DEV, SimpleNamespace(precision=precision))
    return _sequence(rec, ev)


def _sequence(rec, ev):
    rec.last_states_for_each_channel = {'grayscale': None}
    for i in range(pc.NWIN):
        kw = {'latents_only': True} if rec.precision == 'fp32' else {'need_latents': i == pc.NWIN - 1}
        _, _, latent = rec.update_reconstruction(ev, channel_slice=(i * pc.BINS, pc.BINS), **kw)
    rec.last_states_for_each_channel = {'grayscale': None}
    torch.cuda.synchronize()
    return {k: v.detach().float().clone() for k, v in latent.items()}


def _trainer_latents(trainer, ev, precision):
    if type(trainer).__name__ == 'OpenESSPretrainModel':
        st = trainer.step
        st._set_modes()
        rec = st.reconstructor_fp32 if precision == 'fp32' else st.reconstructor
        if precision == 'fp32':
            latent = st._latents_fp32(ev)
        else:
            ev_, frame, labels, sp, S = pc.make_batch()
            latent = st.front((ev, None, frame.to(DEV), labels.to(DEV), sp.to(DEV), S)).content
        assert rec.model is st.front_end_sensor_b
    else:
        trainer._set_modes()
        latent = trainer._train_latents(ev, precision)
    torch.cuda.synchronize()
    return {k: v.detach().float().clone() for k, v in latent.items()}


def _same(a, b):
    assert sorted(a) == sorted(b) == [1, 2, 4, 8]
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ E2VID into the trainers
@pytest.mark.parametrize("precision", ['bf16', 'fp32'])
@pytest.mark.parametrize("base", ["pretrain_dsec_synthetic.yaml", "finetune_dsec_synthetic.yaml"])
def test_e2vid_checkpoint_reaches_the_trainer(tmp_path, base, precision):
    path = str(tmp_path / "e2vid.pth.tar")
    state = pc.write_e2vid(path, pc.LIGHT, seed=41)
    keys = dict(config_option='frame2voxel', train_precision=precision)
    trainer, _ = _trainer(pc.settings(tmp_path, base, e2vid_checkpoint=path, **keys))
    front = trainer.models_dict['front_sensor_b']
    got = front.state_dict()
    assert list(got) == list(state) and not front.training and not any(p.requires_grad for p in front.parameters())
    for k, v in state.items():
        assert got[k].is_cuda and torch.equal(got[k].cpu(), v), k
    # one module behind both reconstructors
    rec32 = getattr(trainer.step if base.startswith('pretrain') else trainer, 'reconstructor_fp32', None)
    assert trainer.reconstructor.model is front and (precision == 'bf16' or rec32.model is front)
    ev = pc.make_batch()[0].to(DEV)
    latents = _trainer_latents(trainer, ev, precision)
    assert latents[8].shape == (pc.B, 256, pc.H // 8, pc.W // 8)
    _same(latents, _standalone_latents(state, pc.LIGHT, precision, ev))
    other, _ = _trainer(pc.settings(tmp_path, base, **keys))                  # no key, no file: the seeded front end
    unloaded = _trainer_latents(other, ev, precision)
    assert all(not torch.equal(latents[k], unloaded[k]) for k in latents)


def test_convgru_checkpoint_as_the_front_end_of_a_fine_tune_trainer(tmp_path):
    path = str(tmp_path / "gru.pth.tar")
    state = pc.write_e2vid(path, pc.GRU, seed=45, spelling='config', module_prefix=True)
    trainer, _ = _trainer(pc.settings(tmp_path, "finetune_dsec_synthetic.yaml", config_option='frame2voxel', e2vid_checkpoint=path))
    front = trainer.models_dict['front_sensor_b']
    assert front.recurrent_block_type == 'convgru'
    assert all(torch.equal(front.state_dict()[k].cpu(), v) for k, v in state.items())
    ev, frame, labels, sp, S = pc.make_batch()
    ev = ev.to(DEV)
    _same(_trainer_latents(trainer, ev, 'bf16'), _standalone_latents(state, pc.GRU, 'bf16', ev))
    losses, _, total = trainer.train_step((ev, labels.to(DEV), frame.to(DEV), labels.to(DEV), labels.to(DEV), None))
    assert set(losses) == {'semseg_sensor_b_loss'} and bool(torch.isfinite(total))


# ------------------------------------------------------------------------------------------------------------ teacher
def _teacher_outputs(net, x):
    """One bf16 and one fp32 forward of the train-mode teacher (each moves the running statistics one step), then its statistics."""
    net.train()
    with torch.no_grad():
        y16 = net(x).float().clone()
        y32 = net.forward_fp32(x).clone()
    torch.cuda.synchronize()
    stats = {k: v.detach().clone() for k, v in net.encoder.state_dict().items() if 'running_' in k or 'num_batches' in k}
    return y16, y32, stats


@pytest.fixture(scope="module")
def teacher_state():
    return pc.teacher_state(seed=43)


@pytest.mark.parametrize("name", ['dino', 'moco_v2'])
def test_teacher_weights_reach_both_forwards(tmp_path, teacher_state, name):
    from openess_amd.models.image_model import DilationFeatureExtractor
    from openess_amd.training.pretrain_step import PretrainStep
    path = pc.write_teacher(tmp_path / f"{name}.pt", name, teacher_state)
    kw = dict(img_size=(pc.H, pc.W), nr_events_data=pc.NWIN)
    st = PretrainStep(image_weights=name, image_weights_path=path, **kw)
    enc = st.model_frame.encoder
    assert all(torch.equal(enc.state_dict()[k].cpu(), v) for k, v in teacher_state.items())
    assert not any(p.requires_grad for p in enc.parameters()) and all(p.requires_grad for p in st.model_frame.decoder.parameters())
    manual = DilationFeatureExtractor(None)
    manual.encoder.load_state_dict(dict(teacher_state))
    manual.decoder.load_state_dict({k: v.cpu() for k, v in st.model_frame.decoder.state_dict().items()})
    manual.to(DEV)
    unloaded = PretrainStep(**kw).model_frame                                 # the same seed: the same head, a random encoder
    assert all(torch.equal(a, b) for a, b in zip(unloaded.decoder.state_dict().values(), st.model_frame.decoder.state_dict().values()))
    x = torch.rand(2, 3, 32, 48, generator=torch.Generator().manual_seed(5)).to(DEV)
    st.model_frame.lazy_features = False
    got, want, other = _teacher_outputs(st.model_frame, x), _teacher_outputs(manual, x), _teacher_outputs(unloaded, x)
    assert got[0].shape == got[1].shape == (2, 256, 32, 48)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert sorted(got[2]) == sorted(want[2]) and len(got[2]) == 3 * 53
    for k in got[2]:
        assert torch.equal(got[2][k], want[2][k]), k
    assert not torch.equal(got[2]['bn1.running_mean'].cpu(), teacher_state['bn1.running_mean'])       # the forwards moved them
    assert not torch.equal(got[0], other[0]) and not torch.equal(got[1], other[1])


# --------------------------------------------------------------------------------------------------- load after a forward
def test_weights_loaded_after_a_forward_replace_every_cached_operand(teacher_state):
    """The operand caches follow the parameters' version counters: a load into modules that have already run (bf16 and fp32, so
    every PackedWeight -- the registered plain ones go through the grouped repack -- and every PackedWeightF32 with its folded
    BatchNorm holds operands of the old weights) must give what a fresh module gives."""
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor
    from openess_amd.e2vid.model.model import E2VIDRecurrent
    from openess_amd.models.image_model import DilationFeatureExtractor
    ev, frame = (t.to(DEV) for t in pc.make_batch()[:2])
    first, second = pc.e2vid_state(pc.LIGHT, 41), pc.e2vid_state(pc.LIGHT, 42)
    model = E2VIDRecurrent(pc.LIGHT)
    model.load_state_dict(first)
    model.to(DEV).eval()
    recs = {p: ImageReconstructor(model, pc.H, pc.W, pc.BINS, DEV, SimpleNamespace(precision=p)) for p in ('bf16', 'fp32')}
    before = {p: _sequence(rec, ev) for p, rec in recs.items()}
    model.load_state_dict(second)
    for p, rec in recs.items():
        after = _sequence(rec, ev)
        _same(after, _standalone_latents(second, pc.LIGHT, p, ev))
        assert not torch.equal(after[8], before[p][8])

    def teacher(state, head_seed):
        net = DilationFeatureExtractor(None)
        net.encoder.load_state_dict(dict(state))
        pc.fill_by_name(net.decoder, head_seed)
        return net.to(DEV)

    def run(net):
        out = []
        with torch.no_grad():
            for mode in (net.eval, net.train):                                # folded BatchNorm, then batch statistics
                mode()
                out += [net(frame).float().clone(), net.forward_fp32(frame).clone()]
        x = net.head(net.encode(frame))                                       # the trainable head under autograd: a registered operand
        out.append(x.float().detach().clone())
        torch.cuda.synchronize()
        return out
    other_state = pc.teacher_state(seed=44)
    net = teacher(teacher_state, 7)
    old = run(net)
    fresh = teacher(other_state, 8)
    net.load_state_dict({k: v.cpu() for k, v in fresh.state_dict().items()})
    new, want = run(net), run(fresh)
    assert len(new) == len(want) == 5
    for i, (a, b, c) in enumerate(zip(new, want, old)):
        assert torch.equal(a, b), i
        assert not torch.equal(a, c), i


# ------------------------------------------------------------------------------------------------ pretrained_backbone, stage 1
def test_pretrained_backbone_reaches_the_frame2recon_student(tmp_path):
    from openess_amd.training.pretrain_step import PretrainStep
    path = str(tmp_path / "backbone.pt")
    state = pc.write_backbone(path)
    torch.manual_seed(0)
    st = PretrainStep(config_option='frame2recon', pretrained_backbone=path, img_size=(pc.H, pc.W), nr_events_data=pc.NWIN,
                      if_spatial_contrastive=True, superpixel_size=pc.SPS, lr=1e-4)
    got = st.model_recon.state_dict()
    assert list(got) == list(state)
    for k, v in state.items():
        assert torch.equal(got[k].cpu(), v), k
    ev, frame, labels, sp, S = pc.make_batch()
    recon = torch.rand(pc.B, 3, pc.H, pc.W, generator=torch.Generator().manual_seed(9))
    losses, _, total = st.train_step((frame.to(DEV), None, recon.to(DEV), labels.to(DEV), sp.to(DEV), S))
    assert set(losses) == {'dense_clip_loss', 'contrastive_nce_loss'} and bool(torch.isfinite(total))
    assert not torch.equal(st.model_recon.state_dict()['classifier.classifier.0.weight'].cpu(), state['classifier.classifier.0.weight'])


# ------------------------------------------------------------------------------------------------------------------ the tool
def test_check_pretrained_reports_each_network(tmp_path, capsys, teacher_state):
    import importlib.util
    import json
    import os
    import yaml
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "check_pretrained.py")
    spec = importlib.util.spec_from_file_location("check_pretrained", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    e2vid = pc.write_e2vid(tmp_path / "gru.pth.tar", pc.GRU)
    pc.write_teacher(tmp_path / "moco.pt", 'moco_v2', teacher_state)
    cfg = yaml.load(open(os.path.join(pc.CFG_DIR, "pretrain_dsec_synthetic.yaml")), yaml.Loader)
    cfg['clip'].update(e2vid_checkpoint=str(tmp_path / "gru.pth.tar"), image_weights='moco_v2', image_weights_path=str(tmp_path / "moco.pt"),
                       pre_trained_backbone=str(tmp_path / "absent.pt"))
    (tmp_path / "s.yaml").write_text(yaml.dump(cfg))
    results = tool.main(["--settings", str(tmp_path / "s.yaml")])
    lines = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith('{')]
    assert lines == json.loads(json.dumps(results)) and [r['network'] for r in results] == ['e2vid', 'teacher', 'deeplabv3']
    for r, key, tensors in zip(results[:2], ('e2vid_checkpoint', 'image_weights_path'), (len(e2vid), 318)):
        assert r['key'] == key and r['found'] and r['missing'] == r['unexpected'] == [] and r['tensors'] == tensors
        assert r['bf16']['finite'] and r['fp32']['finite'] and r['bf16']['std'] > 0 and r['fp32']['std'] > 0
        assert 0 < r['rel_rms'] < 0.5           # two arithmetics of one network: different bits, the same values to first order
    assert results[2] == {'network': 'deeplabv3', 'key': 'pre_trained_backbone', 'file': str(tmp_path / "absent.pt"), 'found': False}
    cfg['clip'].update(require_pretrained=True)
    (tmp_path / "s.yaml").write_text(yaml.dump(cfg))
    with pytest.raises(FileNotFoundError, match="pre_trained_backbone"):
        tool.main(["--settings", str(tmp_path / "s.yaml")])


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("option", ['frame2voxel', 'frame2recon'])
def test_trainer_from_a_yaml_with_every_key_trains_two_steps(tmp_path, caplog, teacher_state, option):
    """One YAML names all three files and sets require_pretrained: True; each config_option loads the networks it builds (the
    E2VID front end or the DeepLabv3 student, and the teacher), says so once per network, and trains its two synthetic batches."""
    files = {'e2vid_checkpoint': str(tmp_path / "e2vid.pth.tar"), 'image_weights_path': str(tmp_path / "dino.pt"),
             'pre_trained_backbone': str(tmp_path / "backbone.pt")}
    e2vid = pc.write_e2vid(files['e2vid_checkpoint'], pc.LIGHT)
    pc.write_teacher(files['image_weights_path'], 'dino', teacher_state)
    backbone = pc.write_backbone(files['pre_trained_backbone'])
    s = pc.settings(tmp_path, "pretrain_dsec_synthetic.yaml", config_option=option, image_weights='dino', require_pretrained=True,
                    **files)
    with caplog.at_level(logging.INFO):
        trainer, loop = _trainer(s)
    assert loop == 'pretraining'
    loaded = [r.getMessage() for r in caplog.records if r.getMessage().startswith('loaded ')]
    first, state, module = (('the E2VID front end', e2vid, 'front_sensor_b') if option == 'frame2voxel' else
                            ('the DeepLabv3 student', backbone, 'model_recon'))
    assert len(loaded) == 2, loaded
    assert first in loaded[0] and files['e2vid_checkpoint' if option == 'frame2voxel' else 'pre_trained_backbone'] in loaded[0]
    assert f"{len(state)} tensors" in loaded[0]
    assert "image teacher" in loaded[1] and files['image_weights_path'] in loaded[1] and "318 tensors" in loaded[1]
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING and 'not found' in r.getMessage()]
    assert all(torch.equal(trainer.models_dict[module].state_dict()[k].cpu(), v) for k, v in state.items())
    enc = trainer.models_dict['model_frame'].encoder.state_dict()
    assert all(torch.equal(enc[k].cpu(), v) for k, v in teacher_state.items())
    trainer.trainEpoch()
    torch.cuda.synchronize()
    assert trainer.step_count == 2
    assert all(bool(torch.isfinite(p).all()) for m in trainer.models_dict.values() for p in m.parameters())
