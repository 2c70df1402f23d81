"""GPU tests of `recon_sources: online_e2vid`: slot 2 of the batch, reconstructed from the sample's events inside
BaseTrainer.prepare_batch.  Synthetic data, 3 sub-windows of 2 000 events, 5 bins, B = 2; 64 x 96 (no padding) and 44 x 60 (the
CropParameters pad-and-crop path).  (a) the public pieces composed by hand, bf16; (b) the CPU oracle, fp32; (c) state isolation;
(d) the ingest schedule; (e) two steps of each shipped YAML through the trainers' own train_step.

Figures of (b) on the MI355X (printed by the test before it asserts) are recorded in DESIGN.md K27."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml

from tests import online_recon_cases as oc

pytestmark = pytest.mark.gpu
PRETRAIN, FINETUNE, OPENESS = ("pretrain_dsec_synthetic_frame2recon_online_recon.yaml",
                               "finetune_dsec_synthetic_frame2recon_online_recon.yaml", "openess_dsec_synthetic_online_recon.yaml")


@pytest.fixture
def filled_e2vid(monkeypatch):
    """`online_recon_model: random` with the weights filled by name (tests/synth.py), as the K14 end-to-end tests do: a
    well-conditioned network whose image spreads over the grey levels, and the oracle's weights."""
    import openess_amd.e2vid.run_reconstruction as mod
    from tests.synth import fill_by_name
    orig = mod.load_model

    def load(path):
        m = orig(path)
        fill_by_name(m, oc.FILL_SEED)
        return m
    monkeypatch.setattr(mod, 'load_model', load)


def _trainer(tmp_path, name=PRETRAIN, hw=(64, 96), augmentation=False, prefetch=True, **clip):
    import train
    from openess_amd.config.settings import Settings
    cfg = yaml.load(open(os.path.join(oc.CFG, name)), yaml.Loader)
    cfg['clip'].update(clip)
    cfg['dataset']['DSEC_events']['shape'] = list(hw)
    cfg['model']['data_augmentation_train'] = bool(augmentation)
    path = tmp_path / f"settings_{hw[0]}x{hw[1]}_{len(os.listdir(tmp_path))}.yaml"
    path.write_text(yaml.dump(cfg))
    train.seed_everything()
    s = Settings(str(path), generate_log=False)
    s.ckpt_dir = str(tmp_path)
    s.ingest_prefetch = prefetch
    assert (s.nr_events_data_b, s.nr_events_window_b, s.nr_temporal_bins_b, s.batch_size_b) == (oc.NWIN, oc.NEV, oc.BINS, oc.B)
    trainer, _ = train.build_trainer(s)
    return trainer


def _host_batch(trainer, split='train', index=0):
    loader = trainer.train_loader_sensor_b if split == 'train' else trainer.val_loader_sensor_b
    torch.manual_seed(77)                                    # the train loader shuffles
    for i, b in enumerate(loader):
        if i == index:
            return b


def _voxels(trainer, ev):
    """The batched voxelizer, called as a public piece (not through the trainer's helper)."""
    from openess_amd.DSEC.dataset.sequence_ov import voxelize_raw_batch
    (H, W), crop = trainer.sensor_geometry
    return voxelize_raw_batch(ev, trainer.device, trainer.rectify_maps, oc.BINS, H, W, crop, oc.NWIN)


@pytest.mark.parametrize("hw", oc.SIZES)
def test_a_slot2_equals_the_public_pieces_composed_by_hand_bf16(hw, tmp_path, filled_e2vid):
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor, PostProcessor
    tr = _trainer(tmp_path, hw=hw)
    host = _host_batch(tr)
    assert isinstance(host[2], dict) and host[2]['aug']['noise_seed'] == [0, 0] and torch.is_tensor(host[0])
    out = tr.prepare_batch(host, 'train')
    got = out[2]
    assert got.shape == (oc.B, 3) + tuple(hw) and got.dtype == torch.float32 and got.is_cuda and len(out) == 8
    vox = _voxels(tr, host[2])
    rec = ImageReconstructor(tr.recon_model, hw[0], hw[1], oc.BINS, tr.device, SimpleNamespace(precision='bf16'))
    assert rec.crop.needs_pad == (hw == (44, 60))
    for i in range(oc.NWIN - 1):
        rec.update_reconstruction(vox, channel_slice=(i * oc.BINS, oc.BINS), need_latents=False)
    img, _, _ = rec.update_reconstruction(vox, channel_slice=((oc.NWIN - 1) * oc.BINS, oc.BINS), reconstruct=True)
    if rec.crop.needs_pad:
        img = img[:, :, rec.crop.iy0:rec.crop.iy1, rec.crop.ix0:rec.crop.ix1]
    post = PostProcessor(tr.device)
    f32 = post.process(img[:, :1])
    u8 = post.process_u8(img[:, :1])
    assert len(torch.unique(u8)) > 64                                    # a real image
    # the grey levels are PostProcessor.process's; their fp32 form is the PNG path's k / 255 (IEEE division), which K13's float
    # output (k times the rounded reciprocal) misses by one ulp on 126 of the 256 levels (tests/test_recon_augment_cases.py)
    want = np.repeat((u8.cpu().numpy() / 255.0).astype(np.float32)[:, None], 3, axis=1)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(oc.levels(got.cpu().numpy()), np.repeat(oc.levels(f32.cpu().numpy()), 3, axis=1))
    assert float((got - f32.expand(-1, 3, -1, -1)).abs().max()) <= 2.0 ** -24
    # every other slot is what the default path gives
    assert torch.equal(out[0].cpu(), host[0]) and torch.equal(out[1].cpu(), host[1]) and torch.equal(out[3].cpu(), host[3])


@pytest.mark.parametrize("hw", oc.SIZES)
def test_b_fp32_source_against_the_cpu_oracle(hw, tmp_path, filled_e2vid):
    """Every pixel within one grey level of the oracle (torch fp32 E2VID on the same voxels, then the reference's PostProcessor
    as torch ops on the device, the K13 tests' yardstick); the share that differs at all at most four times what torch fp32
    shows against float64 on the same case (oc.share_bound: measured 0, so every grey level has to be the oracle's)."""
    from tests.test_hip_e2vid_postprocess import TorchPost, _opts
    tr = _trainer(tmp_path, hw=hw, online_recon_precision='fp32')
    assert tr.recon_reconstructor.precision == 'fp32'
    host = _host_batch(tr)
    got = oc.levels(tr.prepare_batch(host, 'train')[2].cpu().numpy())
    assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 0], got[:, 2])
    vox = _voxels(tr, host[2]).cpu()
    ref = oc.oracle_model(tr.recon_model.state_dict())
    img = oc.oracle_image(vox, ref, hw, torch.float32)
    want = TorchPost(_opts())(img.cuda())[0].cpu().numpy().astype(np.int64)
    d = np.abs(got[:, 0] - want)
    share = float((d != 0).mean())
    print(f"online_e2vid fp32 {hw}: max |grey level - oracle| = {int(d.max())}, share differing = {share:.3e} "
          f"({int((d != 0).sum())} of {d.size} pixels; bound {oc.share_bound(hw):.3e})")
    assert d.max() <= 1
    assert share <= oc.share_bound(hw)


def test_c_states_are_left_empty_and_validation_does_not_see_training(tmp_path, filled_e2vid):
    tr = _trainer(tmp_path, augmentation=True)
    empty = {'grayscale': None}
    assert tr.recon_reconstructor.last_states_for_each_channel == empty
    tr.prepare_batch(_host_batch(tr), 'train')
    assert tr.recon_reconstructor.last_states_for_each_channel == empty
    val = tr.prepare_batch(_host_batch(tr, 'val'), 'val')[2]
    assert tr.recon_reconstructor.last_states_for_each_channel == empty
    fresh = _trainer(tmp_path, augmentation=True)
    assert torch.equal(val, fresh.prepare_batch(_host_batch(fresh, 'val'), 'val')[2])
    assert float(val.min()) >= 0.0 and float(val.max()) <= 1.0          # validation: every augmentation off
    assert 'recon_model' not in tr.models_dict and all(m is not tr.recon_model for m in tr.models_dict.values())
    assert not any(p.requires_grad for p in tr.recon_model.parameters())


def test_d_ingest_prefetch_on_and_off_give_the_same_bits(tmp_path, filled_e2vid):
    runs = []
    for prefetch in (True, False):
        tr = _trainer(tmp_path, augmentation=True, prefetch=prefetch)
        torch.manual_seed(5)
        slots = []
        for batch in tr.device_batches(tr.train_loader_sensor_b):
            slots.append((batch[2].clone(), batch[0].clone()))
        torch.cuda.synchronize()
        assert len(slots) == 2
        runs.append(slots)
    for (a2, a0), (b2, b0) in zip(*runs):
        assert torch.equal(a2, b2) and torch.equal(a0, b0)
    assert not torch.equal(runs[0][0][0], runs[0][1][0])                 # two different batches


def test_f_real_dsec_layout_without_a_reconstructions_tree(tmp_path):
    """train.py's route over an on-disk DSEC tree in the reference's layout that has NO reconstructions/ directory: DSECEvents ->
    collate -> prepare_batch (one rectify map per sequence, selected per sub-window) at 440 x 640 -> one epoch of frame2recon
    pre-training -> checkpoint -> validation."""
    import glob
    import shutil
    import train
    from openess_amd.config.settings import Settings
    from tests import synth_datasets as sd
    root = sd.make_dsec_tree(str(tmp_path / "dsec"))
    for d in glob.glob(os.path.join(root, "**", "reconstructions"), recursive=True):
        shutil.rmtree(d)
    assert not glob.glob(os.path.join(root, "**", "reconstructions*"), recursive=True)
    cfg = yaml.load(open(os.path.join(oc.CFG, PRETRAIN)), yaml.Loader)
    cfg['dataset']['DSEC_events'].update(dataset_path=root, shape=[440, 640], nr_events_data=2, nr_events_window=3000)
    cfg['clip']['superpixel_size'] = 100
    path = tmp_path / "settings.yaml"
    path.write_text(yaml.dump(cfg))
    train.seed_everything()
    s = Settings(str(path), generate_log=False)
    s.ckpt_dir = str(tmp_path)
    assert not s.synthetic_data and s.recon_sources == 'online_e2vid'
    trainer, which = train.build_trainer(s)
    assert which == 'pretraining' and len(trainer.train_loader_sensor_b.dataset) == 6          # 2 train sequences x 3 frames
    host = next(iter(trainer.train_loader_sensor_b))
    assert isinstance(host[2], dict) and len(host[2]['sequence']) == 2 and len(host[2]['aug']['flip']) == 2
    slot2 = trainer.prepare_batch(host, 'train')[2]
    assert slot2.shape == (2, 3, 440, 640) and slot2.dtype == torch.float32 and bool(torch.isfinite(slot2).all())
    trainer.pretraining()
    assert trainer.step_count == 3 and 'Epoch_0.pt' in os.listdir(str(tmp_path))
    trainer.valEpochs()
    assert 0.0 <= float(trainer.last_val_metrics['miou']) <= 100.0


@pytest.mark.parametrize("name,cls", [(PRETRAIN, 'OpenESSPretrainModel'), (FINETUNE, 'OpenESSFineTuneModel'), (OPENESS, 'OpenESSModel')])
def test_e_two_steps_of_each_shipped_yaml(name, cls, tmp_path):
    """The YAML as shipped (online_recon_model: random, augmentation on) through the trainer's own train_step."""
    tr = _trainer(tmp_path, name, augmentation=True)
    assert type(tr).__name__ == cls and tr.online_recon == {'precision': 'bf16', 'model': 'random'}
    for m in tr.models_dict.values():
        m.train()
    steps = 0
    for batch in tr.device_batches(tr.train_loader_sensor_b):
        assert batch[2].shape == (oc.B, 3, 64, 96) and batch[2].dtype == torch.float32 and batch[2].is_cuda
        assert bool(torch.isfinite(batch[2]).all())
        losses = tr.train_step(batch)[0]
        assert losses and all(np.isfinite(float(v)) for v in losses.values()), losses
        steps += 1
    assert steps == 2
    off = _trainer(tmp_path, name, augmentation=False)
    slot2 = off.prepare_batch(_host_batch(off), 'train')[2]
    assert slot2.shape == (oc.B, 3, 64, 96) and float(slot2.min()) >= 0.0 and float(slot2.max()) <= 1.0
