"""Mirror of the pieces of e2vid/utils/inference_utils.py that are on the training path:
EventPreprocessor (:49-87) and CropParameters (:284-311); and gkern (:38-46) of the offline post-processing."""
from math import ceil, erfc, floor, sqrt

import torch

from ... import hip


def gkern(kernlen=5, nsig=1.0):
    """e2vid/utils/inference_utils.py:38-46: 2-D Gaussian kernel (fp32 [kernlen x kernlen]) from the differences of the normal CDF
    at kernlen + 1 points, computed in float64 and cast at the end.  scipy.stats.norm.cdf(x) is restated as
    0.5 * erfc(-x / sqrt(2)) (the same function; the weights equal the reference's bit for bit, tests/test_e2vid_postprocess.py)."""
    import numpy as np
    interval = (2 * nsig + 1.) / kernlen
    x = np.linspace(-nsig - interval / 2., nsig + interval / 2., kernlen + 1)
    kern1d = np.diff(np.array([0.5 * erfc(-v / sqrt(2.0)) for v in x], dtype=np.float64))
    kernel_raw = np.sqrt(np.outer(kern1d, kern1d))
    kernel = kernel_raw / kernel_raw.sum()
    return torch.from_numpy(kernel).float()


def optimal_crop_size(max_size, max_subsample_factor):
    return int(pow(2, max_subsample_factor) * ceil(max_size / pow(2, max_subsample_factor)))


class CropParameters:
    def __init__(self, width, height, num_encoders):
        self.height, self.width, self.num_encoders = height, width, num_encoders
        self.width_crop_size = optimal_crop_size(width, num_encoders)
        self.height_crop_size = optimal_crop_size(height, num_encoders)
        self.padding_top = ceil(0.5 * (self.height_crop_size - height))
        self.padding_bottom = floor(0.5 * (self.height_crop_size - height))
        self.padding_left = ceil(0.5 * (self.width_crop_size - width))
        self.padding_right = floor(0.5 * (self.width_crop_size - width))
        self.needs_pad = any((self.padding_top, self.padding_bottom, self.padding_left, self.padding_right))
        self.pad = torch.nn.ReflectionPad2d((self.padding_left, self.padding_right, self.padding_top, self.padding_bottom))
        self.cx, self.cy = floor(self.width_crop_size / 2), floor(self.height_crop_size / 2)
        self.ix0, self.ix1 = self.cx - floor(width / 2), self.cx + ceil(width / 2)
        self.iy0, self.iy1 = self.cy - floor(height / 2), self.cy + ceil(height / 2)


def load_hot_pixels(path):
    """The reference's hot-pixel file (e2vid/utils/inference_utils.py:59-64): comma-separated `x,y` rows -> int64 [n, 2].  A file
    that cannot be opened prints the reference's warning and lists nothing.  A single row is one pixel (np.loadtxt returns a
    1-D pair for it, on which the reference's `for x, y in ...` loop breaks)."""
    import numpy as np
    try:
        rows = np.loadtxt(path, delimiter=',', ndmin=2)
    except IOError:
        print('WARNING: could not load hot pixels file: {}'.format(path))
        return np.zeros((0, 2), np.int64)
    if rows.size and rows.shape[1] != 2:
        raise ValueError(f"hot pixels file {path}: rows must be `x,y`, got {rows.shape[1]} columns")
    rows = rows.reshape(-1, 2).astype(np.int64)             # .astype(np.int) there: truncation towards zero
    print('Will remove {} hot pixels'.format(rows.shape[0]))
    return rows


class EventPreprocessor:
    """Hot-pixel removal, flip and the whole-tensor non-zero mean/std normalisation, in the reference's order
    (e2vid/utils/inference_utils.py:70-87): events[:, :, y, x] = 0 for every `x,y` row of options.hot_pixels_file, then
    torch.flip(events, dims=[2, 3]) with options.flip, then the normalisation unless options.no_normalize.  `__call__` keeps the
    reference contract (tensor in, tensor out); `slice_to_nhwc8` is the fused form used by ImageReconstructor.  Both options
    run inside the event kernels (hip.EventPre).  Difference from the reference, documented: the caller's tensor
    is NOT mutated (the reference zeroes the hot pixels of its argument in place)."""

    def __init__(self, options=None):
        self.no_normalize = bool(getattr(options, 'no_normalize', False))
        self.hot_pixels_file = getattr(options, 'hot_pixels_file', None) or None
        self.hot_pixel_locations = load_hot_pixels(self.hot_pixels_file) if self.hot_pixels_file else []
        self.flip = bool(getattr(options, 'flip', False))
        if self.flip:
            print('Will flip event tensors.')
        self._pre = {}                                     # (H, W, device) -> hip.EventPre, built at the first tensor of that size

    def pre_for(self, events):
        """The hip.EventPre of this preprocessor for a [B, C, H, W] tensor (None without options).  The mask is built once per
        (H, W, device); a row outside H x W is a ValueError naming it (the reference raises IndexError, or wraps a negative one)."""
        if not self.flip and len(self.hot_pixel_locations) == 0:
            return None
        if events.ndim != 4:
            raise ValueError(f"hot-pixel removal / flip need a [B, C, H, W] event tensor, got {tuple(events.shape)}")
        H, W = int(events.shape[2]), int(events.shape[3])
        key = (H, W, events.device)
        pre = self._pre.get(key)
        if pre is None:
            mask = None
            if len(self.hot_pixel_locations):
                import numpy as np
                m = np.zeros((H, W), np.uint8)
                for i, (x, y) in enumerate(self.hot_pixel_locations):
                    if not (0 <= x < W and 0 <= y < H):
                        raise ValueError(f"hot pixels file {self.hot_pixels_file}: row {i + 1} (x={x}, y={y}) is outside the "
                                         f"{W} x {H} (W x H) event tensor")
                    m[y, x] = 1
                mask = torch.from_numpy(m).to(events.device)
            pre = self._pre[key] = hip.EventPre(mask, self.flip)
        return pre

    def __call__(self, events):
        pre = self.pre_for(events)
        if pre is None:
            if self.no_normalize:
                return events
            return hip.masked_normalize(events.contiguous())
        events = events.contiguous()
        return hip.masked_normalize_slice(events, 0, events.shape[1], pre=pre, normalize=not self.no_normalize)

    def slice_to_nhwc8(self, events, c0, cs):
        return hip.event_slice_to_nhwc8(events, c0, cs, normalize=not self.no_normalize, pre=self.pre_for(events))


def _e2vid_grid_hip(events, num_bins, width, height, device):
    """Shared body of the two reference entry points below: one HIP launch sequence of the nearest-xy / linear-t
    voxelizer (oess_voxelize_nearest_f64, signed single grid) over the [N x 4] (t, x, y, p) float64 rows."""
    import numpy as np
    import torch
    from ... import hip
    assert events.shape[1] == 4
    assert num_bins > 0 and width > 0 and height > 0
    ev = torch.as_tensor(np.ascontiguousarray(events) if isinstance(events, np.ndarray) else events)
    ev = ev.to(device=device, dtype=torch.float64)
    xytp = ev[:, [1, 2, 0, 3]].contiguous()              # the kernel's row order is (x, y, t, p)
    seg = torch.tensor([0, ev.shape[0]], dtype=torch.int64)
    return hip.voxelize_nearest(xytp, seg, num_bins, height, width, crop_rows=0, separate_pol=False)


def events_to_voxel_grid(events, num_bins, width, height):
    """e2vid/utils/inference_utils.py:405-449 (NumPy in, NumPy out).  [N x 4] rows (timestamp, x, y, polarity);
    polarity 0 counts as -1; bilinear in time, nearest in space, ONE signed grid.  Runs on the HIP voxelizer of the
    current CUDA device.  Difference from the reference, documented: events outside the grid are dropped (the
    reference lets NumPy wrap negative flat indices / raise IndexError), and the caller's array is not mutated
    (the reference rescales column 0 and rewrites polarity 0 -> -1 in place)."""
    import torch
    return _e2vid_grid_hip(events, num_bins, width, height, torch.device('cuda')).cpu().numpy()


def events_to_voxel_grid_pytorch(events, num_bins, width, height, device):
    """e2vid/utils/inference_utils.py:452-515: same grid, returned as a tensor on `device` (must be a GPU: the
    product path has no CPU fallback)."""
    import torch
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError("events_to_voxel_grid_pytorch: the HIP voxelizer needs a GPU device")
    return _e2vid_grid_hip(events, num_bins, width, height, device)
