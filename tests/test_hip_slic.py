"""GPU tests of the SLIC superpixel kernels (K24) against the float64 reference of tests/slic_reference.py on the cases of
tests/slic_cases.py, and of `superpixel_sources: online_slic` through the pre-training trainer.

Bounds (the rule of K19 - K23): the two float bounds are four times what the same algorithm in numpy fp32 shows against float64
on the same cases (tools/exp_slic_bounds.py, CPU_FP32 below).  Labels are compared where the float64 reference itself is
decided: one assignment at every pixel whose two lowest distances differ by more than MARGIN of the lowest (fp32 rounding of
the operands moves a distance d by about 2e-6 / sqrt(d) of itself: below 1e-3 for every d >= 4e-6), the whole run by the share of
differing pixels.

    figure                                  numpy fp32 CPU    bound       MI355X
    Lab map, max abs                        1.73e-05          6.91e-05    1.40e-05
    one update, colours, max abs            7.08e-07          2.83e-06    4.77e-07 (7.08e-07 against the float64 map)
    one assignment, pixels left out         <= 0.18 %         < 1 %       (the reference's own figure)
    one assignment, labels inside margin    0                 0           0
    whole run, differing pixels             <= 0.009 %        <= 1 %      0 on all 12 cases at 1, 2 and 10 rounds
"""
import os

import numpy as np
import pytest
import torch

from tests import slic_cases as sc
from tests import slic_reference as ref

pytestmark = pytest.mark.gpu
CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")

CPU_FP32 = {'lab': 1.727e-5, 'colour': 7.077e-7}
BOUND = {k: 4.0 * v for k, v in CPU_FP32.items()}
MARGIN = 1e-3                      # top-two distance margin, as a fraction of the best distance
MAX_LEFT_OUT = 0.01                # pixels the margin may leave out of the assignment test
MAX_DIFFERING = 0.01               # pixels whose label may differ from the float64 run


def _report(name, value, bound=None):
    print(f"[slic] {name}: {value:.3e}" + (f" (bound {bound:.2e})" if bound is not None else ""), flush=True)
    return value


def _gpu(a, dtype=None):
    t = torch.from_numpy(np.array(a))                            # a copy: the shared references are read-only
    return (t.to(dtype) if dtype is not None else t).cuda()


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_lab_map_matches_float64(case):
    from openess_amd import hip
    r = sc.reference(*case)
    ny, nx, _ = r['lattice']
    lab, cen = hip.slic_lab(_gpu(sc.frames(*case)), sc.SIGMA, sc.COMPACTNESS, lattice=(ny, nx))
    assert lab.dtype == torch.float32 and lab.is_contiguous() and tuple(lab.shape) == r['lab'].shape
    err = _report(f"lab {sc.case_id(case)}", float(np.abs(lab.cpu().numpy().astype(np.float64) - r['lab']).max()), BOUND['lab'])
    assert err <= BOUND['lab']
    # the starting centres: the lattice pixels exactly, the map's own values there
    c, c64 = cen.cpu().numpy(), r['centers'][0]
    assert c.shape == c64.shape and np.array_equal(c[..., :2], c64[..., :2].astype(np.float32))
    ys, xs = c64[0, :, 0].astype(int), c64[0, :, 1].astype(int)
    assert torch.equal(cen[..., 2:], lab[:, ys, xs])
    assert torch.equal(hip.slic_lab(_gpu(sc.frames(*case)), sc.SIGMA, sc.COMPACTNESS), lab)


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_one_assignment_from_the_reference_centres(case):
    from openess_amd import hip
    r = sc.reference(*case)
    ny, nx, step = r['lattice']
    l64, c64, p64 = r['lab'], r['centers'][0], r['labels'][0]
    want, best, second = ref.assign(l64, c64, p64, step, with_margin=True)
    keep = (second - best) > MARGIN * best
    left = _report(f"assign {sc.case_id(case)} left out", 1.0 - float(keep.mean()), MAX_LEFT_OUT)
    assert left < MAX_LEFT_OUT                                   # the float64 reference is decided on these inputs
    lab, cen = _gpu(l64, torch.float32), _gpu(c64, torch.float32)
    got = hip.slic_assign(lab, cen, _gpu(p64), step)
    assert got.dtype == torch.int64 and int(got.min()) >= 0 and int(got.max()) < ny * nx
    g = got.cpu().numpy()
    bad = _report(f"assign {sc.case_id(case)} wrong inside the margin", float(((g != want) & keep).sum()))
    assert bad == 0
    # without previous labels every pixel starts in its lattice cell: the same result
    assert torch.equal(hip.slic_assign(lab, cen, None, step, lattice=(ny, nx)), got)
    # in place
    prev = _gpu(p64)
    assert hip.slic_assign(lab, cen, prev, step, out=prev) is prev and torch.equal(prev, got)


def test_a_pixel_eligible_for_no_centre_keeps_its_label():
    from openess_amd import hip
    case = ('blobs', 40, 56, 12)
    r = sc.reference(*case)
    l64, c64 = r['lab'], r['centers'][0]
    yy, xx = np.meshgrid(np.arange(40), np.arange(56), indexing='ij')
    prev = np.broadcast_to((yy * 3 + xx) % 8, (sc.B, 40, 56)).astype(np.int64).copy()
    want, best, second = ref.assign(l64, c64, prev, 3, with_margin=True)       # step 3: windows of 13 x 13 around 8 centres
    none = np.isinf(best)
    assert 0.3 < none.mean() < 0.9 and np.array_equal(want[none], prev[none])
    got = hip.slic_assign(_gpu(l64, torch.float32), _gpu(c64, torch.float32), _gpu(prev), 3).cpu().numpy()
    assert np.array_equal(got[none], prev[none])
    with np.errstate(invalid='ignore'):                           # inf - inf where no centre is eligible
        keep = ~none & ((second - best) > MARGIN * best)
    assert np.array_equal(got[keep], want[keep]) and keep.sum() > 0.95 * (~none).sum()


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_one_update_from_the_reference_labels(case):
    from openess_amd import hip
    r = sc.reference(*case)
    l64, c64, lbl = r['lab'], r['centers'][0], r['labels'][1].copy()
    K = c64.shape[1]
    lbl[lbl == K - 1] = 0                                        # the last centre is empty: it must stay where it is
    lab = _gpu(l64, torch.float32)
    want, counts = ref.update(lab.cpu().numpy().astype(np.float64), lbl, c64.astype(np.float32).astype(np.float64))
    got, cnt = hip.slic_update(lab, _gpu(lbl), _gpu(c64, torch.float32), return_counts=True)
    assert np.array_equal(cnt.cpu().numpy(), counts) and int(counts.sum()) == lbl.size and not counts[:, K - 1].any()
    g = got.cpu().numpy()
    assert np.array_equal(g[..., :2], want[..., :2].astype(np.float32))        # the float64 quotient of an exact sum, rounded to fp32
    assert np.array_equal(g[:, K - 1], c64[:, K - 1].astype(np.float32))
    err = _report(f"update {sc.case_id(case)} colours", float(np.abs(g[..., 2:].astype(np.float64) - want[..., 2:]).max()), BOUND['colour'])
    assert err <= BOUND['colour']
    # against the float64 map itself (the fp32 rounding of the map included): the same bound
    want64, _ = ref.update(l64, lbl, c64)
    err = _report(f"update {sc.case_id(case)} colours, float64 map", float(np.abs(g[..., 2:].astype(np.float64) - want64[..., 2:]).max()),
                  BOUND['colour'])
    assert err <= BOUND['colour']
    again = hip.slic_update(lab, _gpu(lbl), _gpu(c64, torch.float32))
    assert torch.equal(again, got)


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_whole_run_matches_float64(case):
    from openess_amd import hip
    kind, H, W, n = case
    r = sc.reference(*case)
    ny, nx, _ = r['lattice']
    K = ny * nx
    assert K == sc.EXPECTED_K[(H, W, n)]
    x = _gpu(sc.frames(*case))
    for it in sc.ITERS:
        got = hip.slic_superpixels(x, n, sc.COMPACTNESS, sc.SIGMA, iters=it)
        assert got.dtype == torch.int64 and tuple(got.shape) == (sc.B, H, W) and int(got.min()) >= 0 and int(got.max()) < K
        share = _report(f"run {sc.case_id(case)} iters {it} differing", float((got.cpu().numpy() != r['labels'][it]).mean()), MAX_DIFFERING)
        assert share <= MAX_DIFFERING
    # default arguments are the reference's; two runs and a channels-last input give the same bits
    again, cen = hip.slic_superpixels(x, n, return_centers=True)
    assert torch.equal(again, got) and tuple(cen.shape) == (sc.B, K, 5) and bool(torch.isfinite(cen).all())
    cl = x.contiguous(memory_format=torch.channels_last)
    assert cl.stride() != x.stride() and torch.equal(hip.slic_superpixels(cl, n), got)
    crop = torch.zeros(sc.B, 4, H + 2, W + 3, device=x.device)
    crop[:, 1:, 1:-1, 2:-1] = x
    assert torch.equal(hip.slic_superpixels(crop[:, 1:, 1:-1, 2:-1], n), got)      # a channel and crop view: any strides


def test_frames_outside_the_unit_range_give_no_nan():
    from openess_amd import hip
    case = ('noise', 37, 53, 6)
    x = _gpu(sc.frames(*case)) * 1.6 - 0.3                        # brightness / contrast / noise augmentation leaves [0, 1]
    lab = hip.slic_lab(x)
    assert bool(torch.isfinite(lab).all())
    want = ref.lab_map(x.cpu().numpy())
    assert float(np.abs(lab.cpu().numpy() - want).max()) <= 4 * BOUND['lab']        # larger values, the same relative error
    labels, cen = hip.slic_superpixels(x, 6, return_centers=True)
    assert int(labels.min()) >= 0 and int(labels.max()) < 4 and bool(torch.isfinite(cen).all())


# --------------------------------------------------------------------------------------------------------------- trainer
def _trainer(tmp_path):
    import train
    from openess_amd.config.settings import Settings
    from tests import pretrain_fp32_cases as pc
    train.seed_everything()
    s = Settings(os.path.join(CFG, "pretrain_dsec_synthetic_online_slic.yaml"), generate_log=False)
    s.ckpt_dir = str(tmp_path)
    trainer, loop = train.build_trainer(s)
    assert loop == 'pretraining' and type(trainer).__name__ == 'OpenESSPretrainModel' and trainer.online_slic_segments == 25
    pc.fill_models(trainer.models_dict)
    return trainer, s


def test_trainer_computes_the_superpixels_online(tmp_path):
    from openess_amd import hip
    first = None
    for _ in range(2):                                            # two fresh trainers
        trainer, s = _trainer(tmp_path)
        ds = trainer._voxel_ds['train']
        assert ds.superpixel_sources == '' and torch.equal(ds[0][4], torch.ones(64, 96, dtype=torch.int64))
        host = next(iter(trainer.train_loader_sensor_b))
        batch = trainer.prepare_batch(host, 'train')
        B = s.batch_size_b
        ny, nx, _ = hip.slic_lattice(64, 96, 25)
        assert (ny, nx) == (4, 6)
        assert torch.equal(batch[4], hip.slic_superpixels(batch[2], 25)) and batch[4].dtype == torch.int64
        assert int(batch[4].max()) < 24 and batch[-1] == (B - 1) * 25 + 24
        assert len(torch.unique(batch[4])) > 12                  # a segmentation, not the ones-map
        val = trainer.prepare_batch(next(iter(trainer.val_loader_sensor_b)), 'val')
        assert val[4].shape[0] >= 1 and int(val[4].max()) == 24 and val[-1] == (val[4].shape[0] - 1) * 25 + 25     # untouched: the grid
        losses = [trainer.train_step(batch)[0], trainer.train_step(batch)[0]]
        for l in losses:
            assert set(l) >= {'contrastive_nce_loss', 'dense_clip_loss'}
            assert all(bool(torch.isfinite(l[k])) for k in ('contrastive_nce_loss', 'dense_clip_loss'))
        if first is None:
            first = losses[0]
        else:
            assert all(torch.equal(first[k], losses[0][k]) for k in first)


# ------------------------------------------------------------------------------------------------------------------ tool
def test_offline_writer_writes_the_reference_layout(tmp_path, capsys):
    import importlib.util
    from PIL import Image
    from openess_amd import hip
    path = os.path.join(os.path.dirname(CFG), os.pardir, "tools", "write_slic_superpixels.py")
    spec = importlib.util.spec_from_file_location("write_slic_superpixels", os.path.abspath(path))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    u8 = sc.frames_u8('blobs', 40, 56, 7)                                   # [2, 3, 40, 56] uint8
    seq = tmp_path / "train" / "zurich_city_00_a" / "images_aligned" / "left"
    seq.mkdir(parents=True)
    for i in range(2):
        Image.fromarray(np.ascontiguousarray(u8[i].transpose(1, 2, 0))).save(seq / f"{i:06d}.png")
    other = tmp_path / "train" / "zurich_city_00_a" / "sp_slic_rgb" / "left"
    other.mkdir(parents=True)
    Image.fromarray(np.full((40, 56), 7, np.uint8)).save(other / "000001_slic_12.png")      # exists: skipped
    assert tool.main(["--root", str(tmp_path), "--num_segments", "12"]) == 0
    assert "wrote 1 superpixel maps" in capsys.readouterr().out
    got = np.asarray(Image.open(other / "000000_slic_12.png"))
    assert got.dtype == np.uint8 and got.shape == (40, 56)
    want = hip.slic_superpixels(torch.from_numpy(u8[:1]).cuda().float() * (1.0 / 255.0), 12)
    assert np.array_equal(got, want[0].cpu().numpy().astype(np.uint8)) and got.max() < 8
    assert (np.asarray(Image.open(other / "000001_slic_12.png")) == 7).all()
    assert tool.main(["--root", str(tmp_path), "--num_segments", "12"]) == 0
    assert "No images to process" in capsys.readouterr().out
    # DDD17 layout
    d17 = tmp_path / "ddd" / "dir0" / "images_aligned"
    d17.mkdir(parents=True)
    Image.fromarray(np.ascontiguousarray(u8[1].transpose(1, 2, 0))).save(d17 / "img_00000001.png")
    assert tool.main(["--root", str(tmp_path / "ddd"), "--num_segments", "12", "--dataset", "DDD17"]) == 0
    assert os.path.isfile(tmp_path / "ddd" / "dir0" / "sp_slic_rgb" / "img_00000001_slic_12.png")
