#!/usr/bin/env python3
"""Offline E2VID reconstruction (e2vid/run_reconstruction.py:14-116): events text file -> event windows ->
voxel grids (events_to_voxel_grid_pytorch on the HIP voxelizer) -> recurrent E2VID on the MI355X -> one grayscale PNG per
window (what the frame2recon stage reads back as `reconstructions/`).  Same flags as the reference for the path it
executes; `-o/--output_folder` + `--dataset_name` follow e2vid/options/inference_options.py.

    python -m openess_amd.e2vid.run_reconstruction -c E2VID_lightweight.pth.tar -i events.txt -o out/

`--postprocess` runs the reference's PostProcessor (unsharp mask + intensity rescaling, optionally auto-HDR; image_reconstructor.py
:126-140) on each cropped frame and writes its bytes; its tuning flags (`--unsharp_mask_amount`, `--Imin`, `--auto_hdr`, ...) keep
the reference's defaults and are refused without it.  Without `--postprocess` a frame is round(clamp(img, 0, 1) * 255).
`--precision fp32` runs the network in fp32 as the reference does (f32-input MFMA kernels); the default `bf16`
runs it on the training path's bf16-storage kernels.  Both precisions run every recurrent checkpoint with `norm` None or `BN` and
`skip_type: sum`: ConvLSTM or ConvGRU blocks (K28), transposed-convolution decoders (`use_upsample_conv: False`) or the
reference's default bilinear upsample + convolution decoders (K30: the skip sum and the x2 interpolation are one HIP kernel).

Checkpoint format: the reference's (`{'arch': 'E2VIDRecurrent', 'model' | 'config.model': {...}, 'state_dict': ...}`,
e2vid/utils/loading_utils.py:5-16); `-c random` builds E2VID_lightweight with seeded random weights (no checkpoint
ships with either repository)."""
import argparse
import os

import numpy as np
import torch

from types import SimpleNamespace

from .image_reconstructor import ImageReconstructor, PostProcessor
from .model.model import E2VID_LIGHTWEIGHT_CONFIG, E2VIDRecurrent
from .utils.event_readers import FixedDurationEventReader, FixedSizeEventReader
from .utils.inference_utils import events_to_voxel_grid_pytorch


def load_model(path_to_model):
    if path_to_model == 'random':
        torch.manual_seed(1205)
        return E2VIDRecurrent(E2VID_LIGHTWEIGHT_CONFIG)
    from .utils.loading_utils import load_model as load_checkpoint       # the one checkpoint reader (returns (model, None))
    return load_checkpoint(path_to_model)[0]


def reconstruct(path_to_events, model, output_folder=None, window_size=None, fixed_duration=False, window_duration=33.33,
                num_events_per_pixel=0.35, skipevents=0, suboffset=0, device='cuda', max_windows=None, postprocessor=None,
                options=None, precision='bf16', hot_pixels_file=None, flip=False):
    """Returns the list of reconstructed images (uint8 [H, W]); writes frame_%010d.png + timestamps.txt when a folder is given.
    postprocessor: a PostProcessor applied to each cropped frame (its bytes are the image); None = round(clamp(img, 0, 1) * 255).
    options: passed to ImageReconstructor (no_normalize, no_recurrent).  precision: 'bf16' (default) or 'fp32' (the whole network
    in fp32, UNetRecurrent.forward_fp32); it overrides options.precision.  hot_pixels_file (comma-separated `x,y` rows) / flip:
    EventPreprocessor's event-side options (e2vid/options/inference_options.py); when given they override the options' own."""
    if precision not in ('bf16', 'fp32'):
        raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
    with open(path_to_events) as f:
        width, height = (int(v) for v in f.readline().split())
    print('Sensor size: {} x {}'.format(width, height))
    device = torch.device(device)
    model = model.to(device).eval()
    opts = SimpleNamespace(**dict(vars(options) if options is not None else {}, precision=precision))
    if hot_pixels_file:
        opts.hot_pixels_file = hot_pixels_file
    if flip:
        opts.flip = True
    rec = ImageReconstructor(model, height, width, model.num_bins, device, opts)
    N = window_size
    if not fixed_duration and N is None:
        N = int(width * height * num_events_per_pixel)
        print('Will use {} events per tensor (automatically estimated with num_events_per_pixel={:0.2f}).'.format(N, num_events_per_pixel))
    start_index = skipevents + suboffset
    it = (FixedDurationEventReader(path_to_events, duration_ms=window_duration, start_index=start_index) if fixed_duration
          else FixedSizeEventReader(path_to_events, num_events=N, start_index=start_index))
    if output_folder:
        os.makedirs(output_folder, exist_ok=True)
    frames, stamps = [], []
    for k, window in enumerate(it):
        if max_windows is not None and k >= max_windows:
            break
        grid = events_to_voxel_grid_pytorch(window, num_bins=model.num_bins, width=width, height=height, device=device)
        img, _, _ = rec.update_reconstruction(grid.unsqueeze(0), start_index + window.shape[0], window[-1, 0], reconstruct=True)
        if rec.crop.needs_pad:
            img = img[:, :, rec.crop.iy0:rec.crop.iy1, rec.crop.ix0:rec.crop.ix1]
        if postprocessor is None:
            frame = (img[0, 0].clamp(0, 1) * 255.0).round().to(torch.uint8).cpu().numpy()
        else:
            frame = postprocessor.process_u8(img[:, :1])[0].cpu().numpy()       # the crop view goes in as it is (no copy)
        frames.append(frame)
        stamps.append(float(window[-1, 0]))
        if output_folder:
            from PIL import Image
            Image.fromarray(frame).save(os.path.join(output_folder, 'frame_{:010d}.png'.format(k)))
        start_index += window.shape[0]
    if output_folder:
        np.savetxt(os.path.join(output_folder, 'timestamps.txt'), np.asarray(stamps), fmt='%.9f')
    return frames


# (flag, reference default, type) of the PostProcessor options (e2vid/options/inference_options.py:31-46)
POSTPROCESS_FLAGS = (('unsharp_mask_amount', 0.3, float), ('unsharp_mask_sigma', 1.0, float), ('Imin', 0.0, float),
                     ('Imax', 1.0, float), ('auto_hdr', False, bool), ('auto_hdr_median_filter_size', 10, int),
                     ('bilateral_filter_sigma', 0.0, float))


def build_parser():
    p = argparse.ArgumentParser(description='Evaluating a trained network')
    p.add_argument('-c', '--path_to_model', required=True, type=str)
    p.add_argument('-i', '--input_file', required=True, type=str)
    p.add_argument('--fixed_duration', dest='fixed_duration', action='store_true')
    p.set_defaults(fixed_duration=False)
    p.add_argument('-N', '--window_size', default=None, type=int)
    p.add_argument('-T', '--window_duration', default=33.33, type=float)
    p.add_argument('--num_events_per_pixel', default=0.35, type=float)
    p.add_argument('--skipevents', default=0, type=int)
    p.add_argument('--suboffset', default=0, type=int)
    p.add_argument('--compute_voxel_grid_on_cpu', action='store_true', help='accepted for compatibility; the grid is always built on the GPU')
    p.add_argument('-o', '--output_folder', default=None, type=str)
    p.add_argument('--dataset_name', default='reconstruction', type=str)
    p.add_argument('--no-normalize', dest='no_normalize', action='store_true')
    p.add_argument('--no-recurrent', dest='no_recurrent', action='store_true')
    p.add_argument('--hot_pixels_file', default=None, type=str, help='comma-separated x,y rows: pixels zeroed in every event tensor')
    p.add_argument('--flip', dest='flip', action='store_true', help='mirror the event tensors (H and W) before the network')
    p.add_argument('--precision', choices=('bf16', 'fp32'), default='bf16',
                   help="network arithmetic: bf16 (default, the training path's kernels) or fp32 (as the reference)")
    g = p.add_argument_group('post-processing (e2vid/options/inference_options.py:31-46; only with --postprocess)')
    g.add_argument('--postprocess', action='store_true', help="run the reference's PostProcessor (unsharp mask + intensity rescaling)")
    for name, default, typ in POSTPROCESS_FLAGS:
        if typ is bool:
            g.add_argument('--' + name, dest=name, action='store_true', default=None)
        else:
            g.add_argument('--' + name, dest=name, default=None, type=typ, help='default: {}'.format(default))
    return p


def main(argv=None):
    p = build_parser()
    a = p.parse_args(argv)
    given = ['--' + name for name, _, _ in POSTPROCESS_FLAGS if getattr(a, name) is not None]
    if given and not a.postprocess:
        p.error('{} need(s) --postprocess'.format(', '.join(given)))
    opts = SimpleNamespace(no_normalize=a.no_normalize, no_recurrent=a.no_recurrent, hot_pixels_file=a.hot_pixels_file, flip=a.flip,
                           **{name: default if getattr(a, name) is None else getattr(a, name) for name, default, _ in POSTPROCESS_FLAGS})
    post = PostProcessor(torch.device('cuda'), opts) if a.postprocess else None
    out = os.path.join(a.output_folder, a.dataset_name) if a.output_folder else None
    return reconstruct(a.input_file, load_model(a.path_to_model), out, a.window_size, a.fixed_duration, a.window_duration,
                       a.num_events_per_pixel, a.skipevents, a.suboffset, postprocessor=post, options=opts, precision=a.precision)


if __name__ == "__main__":
    main()
