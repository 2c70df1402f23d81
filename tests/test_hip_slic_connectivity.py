"""GPU tests of SLIC's connectivity pass (K24): hip.slic_enforce_connectivity against the sequential loop of
tests/slic_connectivity_reference.py (run without skimage's max_size cut) on every map of tests/slic_connectivity_cases.py, the
pass inside hip.slic_superpixels, and `online_slic_connectivity: True` through the pre-training trainer.

Integer labels in, integer labels out: every comparison is torch.equal, there is no tolerance anywhere.  That the loop with the
cut gives the same on the (a) and (b) maps is checked on the CPU (tests/test_slic_connectivity_host.py)."""
import os

import numpy as np
import pytest
import torch

from tests import slic_cases as sc
from tests import slic_connectivity_cases as cc
from tests import slic_connectivity_reference as cref

pytestmark = pytest.mark.gpu
CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")


def _gpu(a):
    return torch.from_numpy(np.array(a)).cuda()                  # a copy: the shared maps and references are read-only


@pytest.mark.parametrize("name", cc.ALL_NAMES)
def test_pass_equals_the_sequential_loop(name):
    from openess_amd import hip
    c = cc.get(name)
    want, counts = cc.reference(name)
    maps = _gpu(c.maps)
    keep = maps.clone()
    got, n = hip.slic_enforce_connectivity(maps, c.min_size, return_counts=True)
    assert got.dtype == torch.int64 and got.shape == maps.shape and got.is_contiguous() and got.data_ptr() != maps.data_ptr()
    assert n.dtype == torch.int32 and tuple(n.shape) == (2,)
    assert torch.equal(got, _gpu(want))
    assert n.tolist() == list(counts)
    assert int(got.min()) >= 0 and int(got.max()) < c.bound and max(counts) <= c.bound
    assert torch.equal(maps, keep)                               # the input is unchanged
    if c.expected is not None:
        assert torch.equal(got, _gpu(c.expected))                # the answer written down by hand
    # again, into a given tensor and without the counts: the same bits
    out = torch.full_like(maps, -7)
    assert hip.slic_enforce_connectivity(maps, c.min_size, out=out) is out and torch.equal(out, got)
    # on a side stream, with a workspace of its own
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = hip.slic_enforce_connectivity(maps, c.min_size)
    side.synchronize()
    assert torch.equal(other, got)
    # each sample alone: nothing leaks between the samples of a batch
    for b in range(2):
        alone, k = hip.slic_enforce_connectivity(maps[b:b + 1].contiguous(), c.min_size, return_counts=True)
        assert torch.equal(alone[0], got[b]) and k.tolist() == [counts[b]]


def test_min_size_zero_and_one_only_renumber():
    from openess_amd import hip
    c = cc.get("random4-37x53")
    want = np.stack([cref.enforce_sequential(m, 1, None)[0] for m in c.maps])
    maps = _gpu(c.maps)
    for min_size in (0, 1):
        got, n = hip.slic_enforce_connectivity(maps, min_size, return_counts=True)
        assert torch.equal(got, _gpu(want)) and n.tolist() == [int(w.max()) + 1 for w in want]


@pytest.mark.parametrize("H,W", [(1, 1), (1, 300), (300, 1), (3, 257), (2, 128)])
def test_degenerate_extents(H, W):
    """One row, one column, one pixel, a row that ends one pixel into a second chunk of 256, rows that are whole waves."""
    from openess_amd import hip
    rng = np.random.default_rng(H * 1000 + W)
    maps = rng.integers(0, 2, (2, H, W))
    for min_size in (1, 3):
        want = [cref.enforce_sequential(m, min_size, None) for m in maps]
        got, n = hip.slic_enforce_connectivity(_gpu(maps), min_size, return_counts=True)
        assert torch.equal(got, _gpu(np.stack([w[0] for w in want]))) and n.tolist() == [w[1] for w in want]


def test_phase_timer_runs_the_same_pass():
    from openess_amd import hip
    c = cc.get("checker-110x160-n100-it10")
    ms = hip.slic_connectivity_phase_ms(_gpu(c.maps), c.min_size)
    assert list(ms) == ["components", "sizes", "ranks", "donors", "write"] and all(v >= 0.0 for v in ms.values())


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "{}x{}-n{}".format(*s))
def test_superpixels_with_the_pass(shape):
    from openess_amd import hip
    H, W, n = shape
    x = _gpu(sc.frames('checker', H, W, n))
    ny, nx, _ = hip.slic_lattice(H, W, n)
    min_size, _, bound = hip.slic_connectivity_sizes(H, W, ny * nx)
    plain = hip.slic_superpixels(x, n)
    assert torch.equal(hip.slic_superpixels(x, n, enforce_connectivity=False), plain)        # the default: today's bits
    assert torch.equal(plain, hip.slic_superpixels(x, n, sc.COMPACTNESS, sc.SIGMA, iters=10))
    want = hip.slic_enforce_connectivity(plain, min_size)
    got, cen = hip.slic_superpixels(x, n, enforce_connectivity=True, return_centers=True)
    assert torch.equal(got, want) and int(got.min()) >= 0 and int(got.max()) < bound
    assert torch.equal(cen, hip.slic_superpixels(x, n, return_centers=True)[1])              # the centres are those of the rounds
    assert torch.equal(hip.slic_superpixels(x, n, enforce_connectivity=True), got)


# --------------------------------------------------------------------------------------------------------------- trainer
def test_trainer_runs_the_pass_online(tmp_path):
    import train
    from openess_amd import hip
    from openess_amd.config.settings import Settings
    from tests import pretrain_fp32_cases as pc
    train.seed_everything()
    s = Settings(os.path.join(CFG, "pretrain_dsec_synthetic_online_slic_connected.yaml"), generate_log=False)
    s.ckpt_dir = str(tmp_path)
    trainer, loop = train.build_trainer(s)
    assert loop == 'pretraining' and trainer.online_slic_segments == 12 and s.online_slic_connectivity is True
    pc.fill_models(trainer.models_dict)
    batch = trainer.prepare_batch(next(iter(trainer.train_loader_sensor_b)), 'train')
    B = s.batch_size_b
    ny, nx, _ = hip.slic_lattice(64, 96, 12)
    min_size, _, bound = hip.slic_connectivity_sizes(64, 96, ny * nx)
    assert (ny * nx, min_size, bound) == (8, 384, 16)
    assert torch.equal(batch[4], hip.slic_superpixels(batch[2], 12, enforce_connectivity=True)) and batch[4].dtype == torch.int64
    assert torch.equal(batch[4], hip.slic_enforce_connectivity(hip.slic_superpixels(batch[2], 12), min_size))
    assert int(batch[4].max()) < bound and batch[-1] == (B - 1) * 25 + bound                  # S from the shapes alone
    assert len(torch.unique(batch[4])) > 2                       # a segmentation, not the ones-map
    for _ in range(2):
        losses = trainer.train_step(batch)[0]
        assert bool(torch.isfinite(losses['contrastive_nce_loss'])) and bool(torch.isfinite(losses['dense_clip_loss']))


# ------------------------------------------------------------------------------------------------------------------ tool
def test_offline_writer_with_the_pass(tmp_path, capsys):
    import importlib.util
    from PIL import Image
    from openess_amd import hip
    path = os.path.join(os.path.dirname(CFG), os.pardir, "tools", "write_slic_superpixels.py")
    spec = importlib.util.spec_from_file_location("write_slic_superpixels", os.path.abspath(path))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    u8 = sc.frames_u8('checker', 40, 56, 7)
    seq = tmp_path / "train" / "zurich_city_00_a" / "images_aligned" / "left"
    seq.mkdir(parents=True)
    Image.fromarray(np.ascontiguousarray(u8[0].transpose(1, 2, 0))).save(seq / "000000.png")
    assert tool.main(["--root", str(tmp_path), "--num_segments", "12", "--enforce-connectivity"]) == 0
    assert "wrote 1 superpixel maps" in capsys.readouterr().out
    got = np.asarray(Image.open(tmp_path / "train" / "zurich_city_00_a" / "sp_slic_rgb" / "left" / "000000_slic_12.png"))
    want = hip.slic_superpixels(torch.from_numpy(u8[:1]).cuda().float() * (1.0 / 255.0), 12, enforce_connectivity=True)
    assert got.dtype == np.uint8 and np.array_equal(got, want[0].cpu().numpy().astype(np.uint8))
    # 64 x 64 with 256 segments: up to 512 labels, more than a uint8 map holds -- refused before anything is written
    big = tmp_path / "big" / "seq" / "images_aligned" / "left"
    big.mkdir(parents=True)
    Image.fromarray(np.zeros((64, 64, 3), np.uint8)).save(big / "000000.png")
    with pytest.raises(SystemExit, match="512 labels"):
        tool.main(["--root", str(tmp_path / "big"), "--num_segments", "256", "--enforce-connectivity"])
    assert not (tmp_path / "big" / "seq" / "sp_slic_rgb").exists()
