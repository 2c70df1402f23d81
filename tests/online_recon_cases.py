"""Cases of the `recon_sources: online_e2vid` tests: the synthetic batches, the CPU oracle of the reconstruction
(oracle/ E2VID in torch, fp32 or float64, followed by the reference's PostProcessor as torch ops in the same type), and the
measured share bound.  Shared by tests/test_online_recon_host.py, tests/test_hip_online_recon.py and
tools/exp_recon_augment_bounds.py.  Nothing here needs a GPU."""
import os

import numpy as np
import torch
import torch.nn.functional as F

CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")
SIZES = ((64, 96), (44, 60))              # network input: no padding | CropParameters pads to 48 x 64 and crops back
B, NWIN, NEV, BINS, CROP = 2, 3, 2000, 5, 40
FILL_SEED = 11                            # tests.synth.fill_by_name seed of the E2VID weights (as the K14 end-to-end tests)

# Share of pixels whose grey level differs between the oracle in torch fp32 and the same oracle in float64 on these cases
# (tools/exp_recon_augment_bounds.py, CPU, printed as `oracle_fp32_vs_f64_share`).  Measured: 0 of 12 288 and 0 of 5 280 pixels
# (the fp32 oracle's image is within 1.3e-7 of the float64 one, and no grey level's truncation boundary lies that close).  The
# GPU path is allowed four times the share, so on these cases it has to give the oracle's grey level at every pixel.
ORACLE_DIFF_SHARE = {(64, 96): 0.0, (44, 60): 0.0}


def share_bound(hw):
    return 4.0 * ORACLE_DIFF_SHARE[tuple(hw)]


def dataset(hw, mode='train', augmentation=False, length=4):
    from openess_amd.datasets.synthetic_events import SyntheticEvents
    return SyntheticEvents(length=length, sensor_hw=(hw[0] + CROP, hw[1]), crop_rows=CROP, nr_events_data=NWIN, nr_events_window=NEV,
                           nr_bins=BINS, config_option='frame2recon', superpixel_size=25, mode=mode,
                           recon_sources='online_e2vid', recon_augmentation=augmentation)


def host_batch(hw, mode='train', augmentation=False):
    from openess_amd.datasets.synthetic_events import collate
    ds = dataset(hw, mode, augmentation)
    return collate([ds[i] for i in range(B)]), ds


def oracle_voxels(batch2, ds):
    """The collated slot-2 events through the CPU oracle's voxelizer: fp32 [B, NWIN * BINS, H, W]."""
    from oracle import events as oe
    H, W = ds.sensor_hw
    counts = batch2['events_per_sample'].tolist()
    out, base = [], 0
    for n in counts:
        sl = slice(base, base + n)
        out.append(oe.dsec_event_tensor(batch2['x'][sl].numpy(), batch2['y'][sl].numpy(), batch2['t'][sl].numpy(),
                                        batch2['p'][sl].numpy(), ds.rectify_map, NWIN, BINS, H, W, CROP))
        base += n
    return torch.from_numpy(np.stack(out))


def oracle_model(state_dict):
    from oracle import nets as on
    from oracle.step import E2VID_LIGHTWEIGHT_CONFIG
    ref = on.E2VIDRecurrent(E2VID_LIGHTWEIGHT_CONFIG, full=True).eval()
    ref.load_state_dict({k: v.detach().cpu().float() for k, v in state_dict.items()})
    return ref


def filled_state_dict():
    """The weights every test of this feature gives the frozen E2VID: E2VID_lightweight filled by name (well conditioned)."""
    from openess_amd.e2vid.model.model import E2VID_LIGHTWEIGHT_CONFIG, E2VIDRecurrent
    from tests.synth import fill_by_name
    m = E2VIDRecurrent(E2VID_LIGHTWEIGHT_CONFIG).eval()
    fill_by_name(m, FILL_SEED)
    return m.state_dict()


def oracle_image(vox, ref, hw, dtype=torch.float32):
    """The reference's reconstruction loop on the oracle: per sub-window EventPreprocessor -> reflection pad -> E2VIDRecurrent
    from empty states; the last image, cropped back.  dtype float64 runs the same modules in double."""
    from oracle import nets as on
    from openess_amd.e2vid.utils.inference_utils import CropParameters
    crop = CropParameters(hw[1], hw[0], ref.num_encoders)
    ref = ref.to(dtype)
    st = None
    with torch.no_grad():
        for i in range(NWIN):
            x = on.event_preprocess(vox[:, i * BINS:(i + 1) * BINS].to(dtype)).to(dtype)
            if crop.needs_pad:
                x = crop.pad(x)
            img, st, _ = ref(x, st)
    ref.float()
    return img[:, :, crop.iy0:crop.iy1, crop.ix0:crop.ix1].contiguous()


def post_cpu(img, amount=0.3, sigma=1.0, imin=0.0, imax=1.0):
    """UnsharpMaskFilter + IntensityRescaler (e2vid/utils/inference_utils.py:90-129, 234-252) as the reference's torch ops, on
    the CPU in img's own dtype: uint8 [B, H, W]."""
    from openess_amd.e2vid.utils.inference_utils import gkern
    k = gkern(5, sigma).to(img.dtype)[None, None]
    blurred = F.conv2d(img, k, padding=2)
    img = (1 + amount) * img - amount * blurred
    img = 255.0 * (img - imin) / (imax - imin)
    return img.clamp(0.0, 255.0).byte()[:, 0]


def levels(x):
    """fp32 image of grey levels k / 255 -> the integers k."""
    return np.rint(np.asarray(x, dtype=np.float64) * 255.0).astype(np.int64)
