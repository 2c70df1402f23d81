"""Thin tensor-level wrappers over the liboess C-ABI (include/oess.h).

PyTorch is plumbing only here: device memory (tensors), the current HIP stream and autograd
bookkeeping.  Every function enqueues hand-written HIP kernels on the CURRENT torch stream and
raises if the library is missing or a tensor is not on the GPU -- there is no CPU/eager fallback.
"""
import ctypes
import operator
from typing import NamedTuple

import torch

from . import _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("openess_amd HIP path needs CUDA/HIP tensors (no CPU fallback)")


def h2d_async(t, device):
    """Host tensor -> device; small ones without a device synchronisation: an upload from PAGEABLE memory blocks the host until the
    stream has drained (a full synchronisation per call -- one at the top of every training step for the segment offsets of
    the voxelizer); staged through pinned memory it is an ordinary stream-ordered copy."""
    if t.is_cuda:
        return t
    if not t.is_pinned() and t.numel() * t.element_size() <= (1 << 20):
        t = t.pin_memory()            # large pageable tensors (a loader without pin_memory=True) keep the runtime's own staging
    return t.to(device, non_blocking=True)


def _bump(t):
    """A kernel wrote `t` through its raw pointer: tell autograd / version-keyed caches."""
    torch.autograd.graph.increment_version(t)


_WS_CACHE = {}


def _workspace(nbytes, device, tag="ws"):
    # stream-ordered reuse of one buffer is only safe on ONE stream: the current stream is always part of the key (the teacher
    # forward / backward runs on its own stream next to the student's, training/pretrain_step.py)
    key = (tag, device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _WS_CACHE.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _WS_CACHE[key] = ws
    return ws


def _seg_info(seg_offsets):
    """seg_offsets: 1-D int64 (CPU or GPU). Returns (device tensor, n_seg, max_len) -- max_len is
    computed on the host copy so that no device sync is needed when offsets come from the loader."""
    if seg_offsets.is_cuda:
        host = seg_offsets.cpu()
        dev = seg_offsets
    else:
        host = seg_offsets
        dev = None
    host = host.to(torch.int64)
    n_seg = host.numel() - 1
    lens = host[1:] - host[:-1]
    if n_seg < 1 or bool((lens < 0).any()):
        raise ValueError("seg_offsets must be non-decreasing with at least 2 entries")
    return host, dev, n_seg, int(lens.max().item()), int(host[-1].item())


# ------------------------------------------------------------------------------------------ K1
def voxelize_trilinear(x, y, p, t, seg_offsets, C, H, W, crop_rows=0, count_mode=False, out=None):
    """Batched VoxelGrid.convert: returns (n_seg*C) x (H-crop_rows) x W float32 on the GPU."""
    lib = _lib.load()
    _need_gpu(x, y, p, t)
    for a in (x, y, p, t):
        if a.dtype != torch.float32 or not a.is_contiguous() or a.ndim != 1:
            raise ValueError("x, y, p, t must be contiguous 1-D float32")
    host, dev, n_seg, max_len, n_ev = _seg_info(seg_offsets)
    if n_ev > x.numel():
        raise ValueError("seg_offsets exceed the event arrays")
    if dev is None:
        dev = h2d_async(host, x.device)
    if out is None:
        out = torch.empty((n_seg * C, H - crop_rows, W), dtype=torch.float32, device=x.device)
    nbytes = lib.oess_voxelize_workspace_bytes(x.numel(), n_seg, max_len, C, H, W, crop_rows)
    ws = _workspace(nbytes, x.device, tag=("vox", torch.cuda.current_stream(x.device).cuda_stream))
    _lib.check(lib.oess_voxelize_trilinear_f32(_ptr(x), _ptr(y), _ptr(p), _ptr(t), _ptr(dev), n_seg, max_len, C, H, W,
                                               crop_rows, int(count_mode), _ptr(out), _ptr(ws), ws.numel(), _stream()),
               "oess_voxelize_trilinear_f32")
    _bump(out)
    return out


def voxelize_dsec_raw(x, y, t_us, p, rectify_maps, seg_map, seg_offsets, C, H, W, crop_rows=0, count_mode=False,
                      out=None):
    """Raw DSEC columns (uint16 x,y; int64 t; uint8 p) + rectify maps [n_maps,H,W,2] -> voxel tensor."""
    lib = _lib.load()
    _need_gpu(x, y, t_us, p, rectify_maps, seg_map)
    if x.dtype != torch.uint16 or y.dtype != torch.uint16 or t_us.dtype != torch.int64 or p.dtype != torch.uint8:
        raise ValueError("raw DSEC dtypes are x,y:uint16  t:int64  p:uint8")
    if rectify_maps.dtype != torch.float32 or rectify_maps.ndim != 4 or tuple(rectify_maps.shape[1:]) != (H, W, 2):
        raise ValueError("rectify_maps must be float32 [n_maps, H, W, 2]")
    host, dev, n_seg, max_len, n_ev = _seg_info(seg_offsets)
    if n_ev > x.numel():
        raise ValueError("seg_offsets exceed the event arrays")
    if dev is None:
        dev = h2d_async(host, x.device)
    seg_map = seg_map.to(torch.int32)
    if seg_map.numel() != n_seg:
        raise ValueError("seg_map needs one entry per segment")
    if out is None:
        out = torch.empty((n_seg * C, H - crop_rows, W), dtype=torch.float32, device=x.device)
    nbytes = lib.oess_voxelize_workspace_bytes(x.numel(), n_seg, max_len, C, H, W, crop_rows)
    ws = _workspace(nbytes, x.device, tag=("vox", torch.cuda.current_stream(x.device).cuda_stream))
    _lib.check(lib.oess_voxelize_dsec_raw(_ptr(x), _ptr(y), _ptr(t_us), _ptr(p), _ptr(rectify_maps.contiguous()),
                                          _ptr(seg_map), rectify_maps.shape[0], _ptr(dev), n_seg, max_len, C, H, W,
                                          crop_rows, int(count_mode), _ptr(out), _ptr(ws), ws.numel(), _stream()),
               "oess_voxelize_dsec_raw")
    _bump(out)
    return out


def voxelize_nearest(events, seg_offsets, nbins, H, W, crop_rows=0, separate_pol=True, count_mode=False, out=None):
    """Batched generate_voxel_grid over [N x 4] (x, y, t, p) int64 or float64 events."""
    lib = _lib.load()
    _need_gpu(events)
    if events.ndim != 2 or events.shape[1] != 4 or not events.is_contiguous():
        raise ValueError("events must be contiguous [N x 4]")
    host, dev, n_seg, max_len, n_ev = _seg_info(seg_offsets)
    if n_ev > events.shape[0]:
        raise ValueError("seg_offsets exceed the event array")
    if dev is None:
        dev = h2d_async(host, events.device)
    ch = 2 * nbins if separate_pol else nbins
    if out is None:
        out = torch.empty((n_seg * ch, H - crop_rows, W), dtype=torch.float32, device=events.device)
    nbytes = lib.oess_voxelize_workspace_bytes(events.shape[0], n_seg, max_len, 2 * nbins, H, W, crop_rows)
    ws = _workspace(nbytes, events.device, tag=("vox", torch.cuda.current_stream(events.device).cuda_stream))
    if events.dtype == torch.int64:
        fn, name = lib.oess_voxelize_nearest_i64, "oess_voxelize_nearest_i64"
    elif events.dtype == torch.float64:
        fn, name = lib.oess_voxelize_nearest_f64, "oess_voxelize_nearest_f64"
    else:
        raise ValueError("events must be int64 or float64")
    _lib.check(fn(_ptr(events), _ptr(dev), n_seg, max_len, nbins, H, W, crop_rows, int(separate_pol), int(count_mode),
                  _ptr(out), _ptr(ws), ws.numel(), _stream()), name)
    return out


def event_histogram(events, seg_offsets, H, W):
    lib = _lib.load()
    _need_gpu(events)
    if events.dtype != torch.int64 or events.ndim != 2 or events.shape[1] != 4 or not events.is_contiguous():
        raise ValueError("events must be contiguous int64 [N x 4]")
    host, dev, n_seg, max_len, _ = _seg_info(seg_offsets)
    if dev is None:
        dev = h2d_async(host, events.device)
    out = torch.empty((n_seg * 2, H, W), dtype=torch.float32, device=events.device)
    _lib.check(lib.oess_event_histogram_i64(_ptr(events), _ptr(dev), n_seg, max_len, H, W, _ptr(out), _stream()),
               "oess_event_histogram_i64")
    return out


# ------------------------------------------------------------------------------------------ f3: PNG maps
def png_decode_gray8_batch(files, lengths, H, W, flips=None, out=None):
    """Decode a batch of 8-bit single-channel PNG files on the GPU.  files: uint8 1-D (device) = the files back to back;
    lengths: host sequence of their byte lengths; flips: optional host sequence of bools (horizontal mirror per image).
    Returns (maps int64 [n, H, W], status int32 [n] on the device: 0 = ok, else the map is all 255)."""
    lib = _lib.load()
    _need_gpu(files)
    if files.dtype != torch.uint8 or files.ndim != 1 or not files.is_contiguous():
        raise ValueError("files must be a contiguous 1-D uint8 tensor")
    n = len(lengths)
    if n == 0 or int(sum(lengths)) > files.numel():
        raise ValueError("lengths do not match the byte tensor")
    offs, scr, a, b = [0], [], 0, 0
    for L in lengths:
        a += int(L)
        offs.append(a)
        scr.append(b)
        b += ((int(L) + 15) // 16) * 16 + H * (W + 1) + 16
    meta = h2d_async(torch.tensor(offs + scr, dtype=torch.int64), files.device)
    need = lib.oess_png_decode_scratch_bytes(a, n, H, W)
    ws = _workspace(max(need, b + 256), files.device, tag=("png", torch.cuda.current_stream(files.device).cuda_stream))
    fl = None
    if flips is not None and any(flips):
        fl = h2d_async(torch.tensor([1 if f else 0 for f in flips], dtype=torch.uint8), files.device)
    if out is None:
        out = torch.empty((n, H, W), dtype=torch.int64, device=files.device)
    status = torch.empty(n, dtype=torch.int32, device=files.device)
    _lib.check(lib.oess_png_decode_gray8_batch(_ptr(files), _ptr(meta), a, n, H, W, _ptr(fl), _ptr(out), _ptr(ws), ws.numel(),
                                               meta[n + 1:].data_ptr(), _ptr(status), _stream()), "oess_png_decode_gray8_batch")
    return out, status


PNG_ENCODE_SEGMENT = 16384              # OESS_PNG_ENCODE_SEGMENT of include/oess.h


def png_encode_bound(H, W, channels):
    """The largest file png_encode_batch writes for an H x W map of 1 or 3 channels: the slot size it allocates."""
    n = int(_lib.load().oess_png_encode_bound(int(H), int(W), int(channels)))
    if n <= 0:
        raise ValueError(f"png_encode handles 1 <= H, W <= 16384 and 1 or 3 channels, got {(H, W, channels)}")
    return n


def _png_encode_geom(images):
    if (not torch.is_tensor(images) or not images.is_cuda or images.dtype != torch.uint8 or not images.is_contiguous()
            or images.ndim not in (3, 4) or (images.ndim == 4 and images.shape[3] != 3)):
        raise ValueError("png_encode needs a contiguous CUDA/HIP uint8 tensor [n, H, W] or [n, H, W, 3] (no CPU fallback)")
    n, H, W = images.shape[:3]
    ch = 1 if images.ndim == 3 else 3
    if n < 1:
        raise ValueError("png_encode needs at least one image")
    return n, H, W, ch, png_encode_bound(H, W, ch)


def png_encode_batch(images, out=None):
    """Encode a batch of 8-bit maps as PNG files on the GPU.  images: contiguous u8 [n, H, W] (grey) or
    [n, H, W, 3] (RGB) on the device, e.g. segment_render's 'labels' and 'rgb'.  Returns (files u8 [n, slot], sizes int32 [n]),
    both on the device: image i's file is files[i, :sizes[i]], the rest of a slot is unspecified.  out: a (files, sizes) pair
    of an earlier call on the same shape to write into."""
    lib = _lib.load()
    n, H, W, ch, bound = _png_encode_geom(images)
    if out is None:
        files = torch.empty((n, bound), dtype=torch.uint8, device=images.device)
        sizes = torch.empty(n, dtype=torch.int32, device=images.device)
    else:
        files, sizes = out
        if (not torch.is_tensor(files) or files.dtype != torch.uint8 or files.device != images.device or files.ndim != 2
                or files.shape[0] != n or files.shape[1] < bound or not files.is_contiguous()):
            raise ValueError(f"out[0] must be a contiguous uint8 tensor [{n}, >= {bound}] on {images.device}")
        if (not torch.is_tensor(sizes) or sizes.dtype != torch.int32 or sizes.device != images.device or tuple(sizes.shape) != (n,)
                or not sizes.is_contiguous()):
            raise ValueError(f"out[1] must be a contiguous int32 tensor [{n}] on {images.device}")
    need = lib.oess_png_encode_scratch_bytes(n, H, W, ch)
    if need == 0:
        raise ValueError(f"png_encode: a batch of {n} maps of {H} x {W} x {ch} has too many segments for one call")
    ws = _workspace(need, images.device, tag="png_encode")
    _lib.check(lib.oess_png_encode_batch(_ptr(images), n, H, W, ch, _ptr(files), files.shape[1], _ptr(sizes), _ptr(ws), ws.numel(),
                                         _stream()), "oess_png_encode_batch")
    _bump(files)
    _bump(sizes)
    return files, sizes


def png_encode_files(images):
    """png_encode_batch, then the files as a list of bytes.  The sizes cross first (pinned memory, the call's one wait on the
    stream); then only the first max(sizes) columns of the slots follow, in one blocking copy into pinned memory."""
    files, sizes = png_encode_batch(images)
    host_sizes = torch.empty(sizes.shape, dtype=torch.int32, pin_memory=True)
    host_sizes.copy_(sizes, non_blocking=True)
    torch.cuda.current_stream(images.device).synchronize()
    lens = host_sizes.tolist()
    host = torch.empty((files.shape[0], max(lens)), dtype=torch.uint8, pin_memory=True)
    host.copy_(files[:, :max(lens)])
    rows = host.numpy()
    return [rows[i, :n].tobytes() for i, n in enumerate(lens)]


# ------------------------------------------------------------------------------------------ K2
class EventPre:
    """EventPreprocessor's event-side options (e2vid/utils/inference_utils.py:71-75) for the kernels that read the raw event
    tensor: hot_mask = uint8 [H, W] device tensor, non-zero = hot pixel, in SOURCE coordinates (None: no list); flip mirrors H and
    W.  Order as in the reference: zero the hot pixels, then flip, then normalise.  With `pre=` a wrapper computes what it
    computes without on torch.flip(zeroed copy, [2, 3]); the caller's tensor is only read."""

    def __init__(self, hot_mask=None, flip=False):
        if hot_mask is not None:
            if not isinstance(hot_mask, torch.Tensor) or hot_mask.dtype != torch.uint8:
                raise ValueError("EventPre: hot_mask must be a uint8 tensor")
            if hot_mask.ndim != 2 or not hot_mask.is_contiguous():
                raise ValueError("EventPre: hot_mask must be a contiguous [H, W] tensor")
        self.hot_mask, self.flip = hot_mask, bool(flip)

    def tag(self):
        """What a statistics cache has to compare: the flip does not change statistics, the mask does."""
        m = self.hot_mask
        return None if m is None else (m.data_ptr(), m._version)

    def bind(self, events):
        """Host-side checks against the [B, C, H, W] event tensor -> the oess_event_pre_t to pass (keep it alive over the call)."""
        if events.ndim != 4:
            raise ValueError("pre= needs a [B, C, H, W] event tensor")
        m = self.hot_mask
        if m is not None:
            if tuple(m.shape) != tuple(events.shape[2:]):
                raise ValueError(f"EventPre: hot_mask is {tuple(m.shape)}, the event tensor is H x W = {tuple(events.shape[2:])}")
            if not m.is_cuda or m.device != events.device:
                raise ValueError(f"EventPre: hot_mask is on {m.device}, the event tensor on {events.device}")
        return _lib.EventPre(None if m is None else m.data_ptr(), int(self.flip))


def _bind_pre(pre, events):
    if not isinstance(pre, EventPre):
        raise ValueError("pre must be a hip.EventPre")
    return pre.bind(events)


def masked_normalize(x, out=None, pre=None):
    """EventPreprocessor / normalize_voxel_grid on a dense float32 tensor (whole-tensor statistics).  pre (EventPre; x is then
    [B, C, H, W]): hot pixels zeroed and H, W mirrored first."""
    if pre is not None:
        if x.ndim != 4:
            raise ValueError("pre= needs a [B, C, H, W] event tensor")
        return masked_normalize_slice(x, 0, x.shape[1], out=out, pre=pre)
    lib = _lib.load()
    _need_gpu(x)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("masked_normalize needs a contiguous float32 tensor")
    if out is None:
        out = torch.empty_like(x)
    stats = torch.empty(lib.oess_masked_stats_doubles(1), dtype=torch.float64, device=x.device)
    _lib.check(lib.oess_masked_normalize_f32(_ptr(x), _ptr(out), x.numel(), _ptr(stats), _stream()),
               "oess_masked_normalize_f32")
    return out


def masked_normalize_slice(x, c0, cs, out=None, pre=None, normalize=True):
    """Normalise the channel slice x[:, c0:c0+cs] of a contiguous [B, C, H, W] float32 tensor.  pre (EventPre): hot pixels
    zeroed and H, W mirrored first; normalize=False (with pre only) stops after that."""
    cpre = None if pre is None else _bind_pre(pre, x)
    if pre is None and not normalize:
        raise ValueError("normalize=False without pre= is a plain slice")
    lib = _lib.load()
    _need_gpu(x)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.ndim != 4:
        raise ValueError("needs contiguous float32 [B, C, H, W]")
    B, Ct, H, W = x.shape
    if out is None:
        out = torch.empty((B, cs, H, W), dtype=torch.float32, device=x.device)
    stats = torch.empty(lib.oess_masked_stats_doubles(1), dtype=torch.float64, device=x.device)
    if cpre is not None:
        if out.data_ptr() == x.data_ptr():
            raise ValueError("pre=: out must not alias the input")
        _lib.check(lib.oess_masked_normalize_slice_pre_f32(_ptr(x), _ptr(out), B, Ct, c0, cs, H, W, ctypes.byref(cpre),
                                                           int(bool(normalize)), _ptr(stats), _stream()),
                   "oess_masked_normalize_slice_pre_f32")
        return out
    _lib.check(lib.oess_masked_normalize_slice_f32(_ptr(x), _ptr(out), B, Ct, c0, cs, H * W, _ptr(stats), _stream()),
               "oess_masked_normalize_slice_f32")
    return out


# ------------------------------------------------------------------------------------------ K7
class _SegmentMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat_pm, ids, pps, sps, S):
        lib = _lib.load()
        P, Cf = feat_pm.shape
        k = torch.empty((S, Cf), dtype=torch.float32, device=feat_pm.device)
        cnt = torch.empty((S,), dtype=torch.float32, device=feat_pm.device)
        is_bf16 = int(feat_pm.dtype == torch.bfloat16)
        ws_bytes = lib.oess_segment_mean_fwd_workspace_bytes(S, Cf)           # 96-bit fixed-point accumulators (deterministic sums)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=feat_pm.device)
        _lib.check(lib.oess_segment_mean_fwd(_ptr(feat_pm), is_bf16, _ptr(ids), P, pps, sps, Cf, S, _ptr(k), _ptr(cnt),
                                             _ptr(ws), ws_bytes, _stream()), "oess_segment_mean_fwd")
        ctx.save_for_backward(ids, cnt)
        ctx.meta = (P, Cf, pps, sps, S, feat_pm.dtype)
        ctx.mark_non_differentiable(cnt)
        return k, cnt

    @staticmethod
    def backward(ctx, gk, _gcnt):
        lib = _lib.load()
        ids, cnt = ctx.saved_tensors
        P, Cf, pps, sps, S, dtype = ctx.meta
        gk = gk.contiguous().float()
        gfeat = torch.empty((P, Cf), dtype=dtype, device=gk.device)
        table = torch.empty((S, Cf), dtype=dtype, device=gk.device)          # gk / (count + 1e-6), formed once per call
        _lib.check(lib.oess_segment_mean_bwd(_ptr(gk), _ptr(cnt), _ptr(ids), P, pps, sps, Cf, S, _ptr(gfeat),
                                             int(dtype == torch.bfloat16), _ptr(table), table.numel() * table.element_size(),
                                             _stream()), "oess_segment_mean_bwd")
        return gfeat, None, None, None, None


def segment_mean(feat_pm, ids, pixels_per_sample, superpixel_size, S):
    """Superpixel scatter-mean.  feat_pm: pixel-major [P, Cf] (fp32/bf16); ids: [P] int64 raw ids."""
    _need_gpu(feat_pm, ids)
    if feat_pm.dtype not in (torch.float32, torch.bfloat16) or not feat_pm.is_contiguous() or feat_pm.ndim != 2:
        raise ValueError("feat must be contiguous [P, Cf] float32/bfloat16")
    if feat_pm.shape[1] % 4:
        raise ValueError("channel count must be a multiple of 4")
    ids = ids.reshape(-1).contiguous().to(torch.int64)
    return _SegmentMean.apply(feat_pm, ids, int(pixels_per_sample), int(superpixel_size), int(S))[0]


def superpixel_pool(feat_nchw, superpixels, superpixel_size, S=None, with_count=False):
    """Drop-in for the inline block of training/pretrain_trainer.py:445-465.  feat_nchw is logically
    B x C x H x W (any memory format; channels_last is free), superpixels B x H x W int64.
    with_count: also the fp32 pixel count of every row (not differentiable)."""
    if hasattr(feat_nchw, 'pool') and hasattr(feat_nchw, 'materialize'):      # PointwiseFeature / UpsampledNormalizedFeature
        return feat_nchw.pool(superpixels, superpixel_size, S)
    B, C, H, W = feat_nchw.shape
    if S is None:   # data-dependent size exactly like sparse_coo_tensor (costs one device sync)
        off = torch.arange(0, B * superpixel_size, superpixel_size, device=superpixels.device)[:, None, None]
        S = int((superpixels + off).max().item()) + 1
    pm = feat_nchw.permute(0, 2, 3, 1).contiguous().view(B * H * W, C)
    if not with_count:
        return segment_mean(pm, superpixels, H * W, superpixel_size, S)
    _need_gpu(pm, superpixels)
    ids = superpixels.reshape(-1).contiguous().to(torch.int64)
    return _SegmentMean.apply(pm, ids, H * W, int(superpixel_size), int(S))


class PointwiseFeature:
    """A full-resolution feature map that is a 1x1 convolution of `x` (SemSegE2VID's 256-channel `x_ch256 = decoder_ch256(x)`,
    models/style_networks.py:166), kept as the pair (x, conv) because its only consumer in the pre-training step is the
    superpixel mean of training/pretrain_trainer.py:445-465 -- and the mean commutes with the per-pixel affine map:
        sum_p (W x_p + b) / (n + 1e-6)  =  W (sum_p x_p / (n + 1e-6)) + b n / (n + 1e-6).
    Pooling the 32 input channels and applying the convolution to the S pooled rows gives the reference's result without the
    8 x 256 x 440 x 640 tensor (1.15 GB in bf16), its convolution forward / input- / weight-gradient passes and the 256-channel
    scatter / gather -- and without that tensor's bf16 rounding.  `materialize()` is the tensor itself for any other consumer."""

    def __init__(self, x, conv):
        self.x, self.conv = x, conv

    @property
    def shape(self):
        B, _, H, W = self.x.shape
        return torch.Size((B, self.conv.weight.shape[0], H, W))

    def materialize(self):
        if self.x.dtype == torch.float32:           # fp32 training (K20): the conv's fp32 autograd form, not its bf16 forward
            return self.conv.forward_f32_train(self.x)
        if self.x.dtype != torch.bfloat16:
            raise ValueError(f"PointwiseFeature holds a bfloat16 or float32 map, not {self.x.dtype}")
        return self.conv(self.x)

    def pool(self, superpixels, superpixel_size, S=None):
        if self.x.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"PointwiseFeature holds a bfloat16 or float32 map, not {self.x.dtype}")
        k_in, cnt = superpixel_pool(self.x, superpixels, superpixel_size, S, with_count=True)
        w = self.conv.weight.flatten(1).float()                                   # Cout x Cin
        k = k_in @ w.t()
        if self.conv.bias is not None:
            k = k + (cnt / (cnt + 1e-6)).unsqueeze(1) * self.conv.bias.float()
        return k


# ------------------------------------------------------------------------------------------ K9
class _TaskLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, K, ignore_index, flags, strides):
        lib = _lib.load()
        P, pps, sb, sp, sc = strides
        sums = torch.empty(lib.oess_task_loss_sums_doubles(K), dtype=torch.float64, device=logits.device)   # totals + partial rows
        loss = torch.empty(3, dtype=torch.float32, device=logits.device)
        is_bf16 = int(logits.dtype == torch.bfloat16)
        _lib.check(lib.oess_task_loss_fwd(_ptr(logits), is_bf16, _ptr(target), P, pps, sb, sp, sc, K, ignore_index,
                                          flags, _ptr(sums), _ptr(loss), _stream()), "oess_task_loss_fwd")
        ctx.save_for_backward(logits, target, sums)
        ctx.meta = (K, ignore_index, flags, strides)
        return loss[0], loss[1:].clone()

    @staticmethod
    def backward(ctx, g_total, _g_parts):
        lib = _lib.load()
        logits, target, sums = ctx.saved_tensors
        K, ignore_index, flags, (P, pps, sb, sp, sc) = ctx.meta
        grad = torch.empty_like(logits)
        gdev = g_total.reshape(1).float().contiguous()          # device scalar: no host sync
        _lib.check(lib.oess_task_loss_bwd(_ptr(logits), int(logits.dtype == torch.bfloat16), _ptr(target), P, pps, sb,
                                          sp, sc, K, ignore_index, flags, _ptr(sums), 1.0, _ptr(gdev), _ptr(grad),
                                          int(grad.dtype == torch.bfloat16), _stream()), "oess_task_loss_bwd")
        return grad, None, None, None, None, None


def task_loss(logits, target, num_classes, ignore_index=255, losses=("dice", "cross_entropy")):
    """TaskLoss (Dice + CE).  logits: logically B x K x H x W, contiguous either as NCHW or as
    channels_last (NHWC); float32 or bfloat16.  Returns (total, [dice, ce])."""
    _need_gpu(logits, target)
    B, K, H, W = logits.shape
    if K != num_classes:
        raise ValueError("logits channel count != num_classes")
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("logits must be float32 or bfloat16")
    if logits.is_contiguous():
        strides = (B * H * W, H * W, K * H * W, 1, H * W)
    elif logits.is_contiguous(memory_format=torch.channels_last):
        strides = (B * H * W, H * W, H * W * K, K, 1)
    else:
        logits = logits.contiguous()
        strides = (B * H * W, H * W, K * H * W, 1, H * W)
    target = target.reshape(-1).contiguous().to(torch.int64)
    flags = (1 if "dice" in losses else 0) | (2 if "cross_entropy" in losses else 0)
    return _TaskLoss.apply(logits, target, K, int(ignore_index), flags, strides)


# ------------------------------------------------------------------------------------------ a16 consistency losses
def _loss_scratch(device):
    lib = _lib.load()
    return torch.empty(lib.oess_loss_partials_bytes() // 8, dtype=torch.float64, device=device)


class _L1Mean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        lib = _lib.load()
        loss = torch.empty(1, dtype=torch.float32, device=a.device)
        _lib.check(lib.oess_l1_mean_fwd(_ptr(a), _ptr(b), a.numel(), int(a.dtype == torch.bfloat16), _ptr(_loss_scratch(a.device)),
                                        _ptr(loss), _stream()), "oess_l1_mean_fwd")
        ctx.save_for_backward(a, b)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        a, b = ctx.saved_tensors
        ga = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        gb = torch.empty_like(b) if b is not None and ctx.needs_input_grad[1] else None
        if ga is None and gb is None:
            return None, None
        gdev = g.reshape(1).float().contiguous()
        _lib.check(lib.oess_l1_mean_bwd(_ptr(a), _ptr(b), a.numel(), int(a.dtype == torch.bfloat16), _ptr(gdev),
                                        None if ga is None else _ptr(ga), None if gb is None else _ptr(gb), _stream()),
                   "oess_l1_mean_bwd")
        return ga, gb


def l1_mean(a, b):
    """nn.L1Loss()(a, b) (training/openess_trainer.py:497).  a, b: same shape, dtype (fp32 / bf16) and memory layout.
    Two UpsampledFeature operands of the same geometry (DeepLabV3.lazy_feats): bilinear upsampling is linear, so
    |up(a) - up(b)| = |up(a - b)| -- the difference is formed on the low-resolution maps in fp32 and ONE full-resolution tensor
    is written, read, and differentiated instead of two."""
    if isinstance(a, UpsampledFeature) and isinstance(b, UpsampledFeature):
        if a.size != b.size or a.align_corners != b.align_corners or a.x.shape != b.x.shape:
            raise ValueError("l1_mean: upsampled operands differ in geometry")
        d = (a.x.float() - b.x.float()).to(a.x.dtype)
        u = bilinear_resize(d, size=a.size, align_corners=a.align_corners)
        return _L1Mean.apply(u if (u.is_contiguous() or u.is_contiguous(memory_format=torch.channels_last)) else u.contiguous(), None)
    if isinstance(a, UpsampledFeature):
        a = a.materialize()
    if isinstance(b, UpsampledFeature):
        b = b.materialize()
    _need_gpu(a, b)
    if a.shape != b.shape or a.dtype != b.dtype or a.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("l1_mean: operands must share shape and dtype (float32 or bfloat16)")
    if a.stride() != b.stride() or not (a.is_contiguous() or a.is_contiguous(memory_format=torch.channels_last)):
        a, b = a.contiguous(), b.contiguous()
    return _L1Mean.apply(a, b)


class _CosMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, eps):
        lib = _lib.load()
        (B, H, W, C), sa, sb = a.shape, _pix_stride(a), _pix_stride(b)
        loss = torch.empty(1, dtype=torch.float32, device=a.device)
        _lib.check(lib.oess_cosine_mean_fwd(_ptr(a), sa, _ptr(b), sb, B * H * W, C, int(a.dtype == torch.bfloat16), eps,
                                            _ptr(_loss_scratch(a.device)), _ptr(loss), _stream()), "oess_cosine_mean_fwd")
        ctx.save_for_backward(a, b)
        ctx.eps = eps
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        a, b = ctx.saved_tensors
        (B, H, W, C), sa, sb = a.shape, _pix_stride(a), _pix_stride(b)
        ga = torch.empty((B, H, W, C), dtype=a.dtype, device=a.device) if ctx.needs_input_grad[0] else None
        gb = torch.empty((B, H, W, C), dtype=b.dtype, device=b.device) if ctx.needs_input_grad[1] else None
        gdev = g.reshape(1).float().contiguous()
        _lib.check(lib.oess_cosine_mean_bwd(_ptr(a), sa, _ptr(b), sb, B * H * W, C, int(a.dtype == torch.bfloat16), ctx.eps,
                                            _ptr(gdev), None if ga is None else _ptr(ga), C, None if gb is None else _ptr(gb), C,
                                            _stream()), "oess_cosine_mean_bwd")
        return ga, gb, None


def cosine_mean_loss(a, b, eps=1e-8):
    """mean(1 - F.cosine_similarity(a, b, dim=1)) (training/openess_trainer.py:501) for logical B x C x H x W tensors;
    computed on NHWC views (a channels_last input is used in place, an NCHW one is re-laid out once)."""
    _need_gpu(a, b)
    if a.shape != b.shape or a.dtype != b.dtype or a.dtype not in (torch.float32, torch.bfloat16) or a.ndim != 4:
        raise ValueError("cosine_mean_loss: operands must be 4-D with the same shape and dtype (float32 or bfloat16)")
    an, bn = a.permute(0, 2, 3, 1), b.permute(0, 2, 3, 1)
    if an.stride(3) != 1 or not _uniform_pix_stride(an):
        an = an.contiguous()
    if bn.stride(3) != 1 or not _uniform_pix_stride(bn):
        bn = bn.contiguous()
    return _CosMean.apply(an, bn, float(eps))


def _pix_stride(x):
    """Pixel stride (elements) of an NHWC view; size-1 dims carry arbitrary strides in torch, so skip them."""
    B, H, W, C = x.shape
    if W > 1:
        return x.stride(2)
    if H > 1:
        return x.stride(1)
    if B > 1:
        return x.stride(0)
    return C


def _uniform_pix_stride(x):
    B, H, W, C = x.shape
    ps = _pix_stride(x)
    return (H == 1 or W == 1 or x.stride(1) == W * ps) and (B == 1 or x.stride(0) == H * W * ps) and ps >= C


class _NCELoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, k, q, temperature):
        lib = _lib.load()
        S, C = k.shape
        G = torch.empty((S, S), dtype=torch.float32, device=k.device)
        part = torch.empty(S, dtype=torch.float64, device=k.device)
        loss = torch.empty(1, dtype=torch.float32, device=k.device)
        _lib.check(lib.oess_nce_loss_fwd(_ptr(k), _ptr(q), S, C, temperature, _ptr(G), _ptr(part), part.numel() * 8, _ptr(loss),
                                         _stream()), "oess_nce_loss_fwd")
        ctx.save_for_backward(G, k, q)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        G, k, q = ctx.saved_tensors
        S, C = k.shape
        gk = torch.empty_like(k) if ctx.needs_input_grad[0] else None
        gq = torch.empty_like(q) if ctx.needs_input_grad[1] else None
        gdev = g.reshape(1).float().contiguous()
        _lib.check(lib.oess_nce_loss_bwd(_ptr(G), _ptr(k), _ptr(q), S, C, _ptr(gdev), None if gk is None else _ptr(gk),
                                         None if gq is None else _ptr(gq), _stream()), "oess_nce_loss_bwd")
        return gk, gq, None


def nce_loss(k, q, temperature=0.07):
    """NCELoss.forward (utils/loss_functions.py:147-154) on fp32 [S x C] superpixel means."""
    _need_gpu(k, q)
    if k.shape != q.shape or k.ndim != 2:
        raise ValueError("nce_loss: k and q must both be [S, C]")
    return _NCELoss.apply(k.float().contiguous(), q.float().contiguous(), float(temperature))


# ------------------------------------------------------------------------------------------ K11
def confusion_accumulate(pred, label, num_classes, ignore_label, conf):
    lib = _lib.load()
    _need_gpu(pred, label, conf)
    pred = pred.reshape(-1).contiguous().to(torch.int64)
    label = label.reshape(-1).contiguous().to(torch.int64)
    if conf.dtype != torch.int64 or conf.numel() != num_classes * num_classes or not conf.is_contiguous():
        raise ValueError("conf must be contiguous int64 K*K")
    _lib.check(lib.oess_confusion_accumulate(_ptr(pred), _ptr(label), pred.numel(), num_classes, ignore_label,
                                             _ptr(conf), _stream()), "oess_confusion_accumulate")
    return conf


# ------------------------------------------------------------------------------------------ conv
def _nhwc_geom(x):
    """x: bf16 [B, H, W, C] view whose last dim is dense and whose pixels are equally spaced."""
    if x.dtype != torch.bfloat16 or x.ndim != 4 or x.stride(3) != 1:
        raise ValueError("expected bf16 NHWC tensor with dense channels")
    B, H, W, C = x.shape
    ps = x.stride(2)
    if x.stride(1) != W * ps or (B > 1 and x.stride(0) != H * W * ps):
        raise ValueError("NHWC tensor must have uniformly strided pixels")
    return B, H, W, C, ps


_CONV_WS_NEED = {}


def conv_packed_bytes(Cout, Cin, R, S, flip=False):
    return _lib.load().oess_conv2d_packed_bytes(Cout, Cin, R, S, int(flip))


def pack_conv_weight(w, flip=False):
    """Conv2d.weight (OIHW, any float dtype) -> packed bf16 operand for conv2d_nhwc.
    flip=True (1) packs the data-gradient operator of a stride-1 convolution; flip=2 packs the forward operator with
    ConvLSTM gate-interleaved rows (convlstm_fused)."""
    lib = _lib.load()
    _need_gpu(w)
    w = w.detach().float().contiguous()
    Cout, Cin, R, S = w.shape
    nbytes = lib.oess_conv2d_packed_bytes(Cout, Cin, R, S, int(flip))
    packed = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=w.device)
    _lib.check(lib.oess_conv2d_pack_weight(_ptr(w), Cout, Cin, R, S, int(flip), _ptr(packed), nbytes, _stream()),
               "oess_conv2d_pack_weight")
    return packed


def _conv_marshal(x, Cout, R, S, stride, pad, dil, residual, out, out_f32, tile_stats, allow_splitk, alloc):
    """The arguments of oess_conv2d_fwd_bf16 that conv2d_nhwc derives from its tensors, shared with conv2d_route so that the
    query describes the call exactly: (B, H, W, Cin, ps_in, out, is_f32, ps_out, ps_res, workspace bytes to offer).
    alloc=False (the query) leaves a missing output unallocated: it would be dense and 16-byte aligned."""
    B, H, W, Cin, ps_in = _nhwc_geom(x)
    Ho = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (S - 1) - 1) // stride + 1
    if out is None and alloc:
        out = torch.empty((B, Ho, Wo, Cout), dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
    if out is None:
        is_f32, ps_out = bool(out_f32), Cout
    else:
        is_f32 = out.dtype == torch.float32
        if is_f32:
            if out.stride(3) != 1:
                raise ValueError("fp32 output must have dense channels")
            ps_out = out.stride(2)
        else:
            ps_out = _nhwc_geom(out)[4]
        if tuple(out.shape) != (B, Ho, Wo, Cout):
            raise ValueError(f"bad output shape {tuple(out.shape)} != {(B, Ho, Wo, Cout)}")
    ps_res = 0
    if residual is not None:
        ps_res = _nhwc_geom(residual)[4]
    key = (B, H, W, Cin, Cout, R, S, stride, pad, dil, tile_stats is not None, is_f32)
    need = _CONV_WS_NEED.get(key)
    if need is None:       # host-only query of the dispatch rules (split-K layers want fp32 slice scratch), cached per geometry
        need = _CONV_WS_NEED[key] = _lib.load().oess_conv2d_fwd_workspace_bytes(*key[:10], int(key[10]), int(key[11]))
    return B, H, W, Cin, ps_in, out, is_f32, ps_out, ps_res, (need if allow_splitk else 0)


def conv2d_nhwc(x, packed, bias, Cout, R, S, stride=1, pad=0, dil=1, relu=False, residual=None, out=None,
                out_f32=False, tile_stats=None, allow_splitk=True):
    """out = act(conv(x, w) + bias [+ residual]) on NHWC bf16 views (channel slices of wider buffers are fine).
    x's channel count must be a multiple of 8 (zero-padded channels; packed weights are zero there).
    allow_splitk=False withholds the scratch of the split-K form (small-M / long-K layers): one pass, for A/B tests."""
    lib = _lib.load()
    e0 = None if _CONV_TIMING is None or Cout <= 64 else _timing_start(lstm=False)
    _need_gpu(x, packed)
    B, H, W, Cin, ps_in, out, is_f32, ps_out, ps_res, need = _conv_marshal(x, Cout, R, S, stride, pad, dil, residual, out, out_f32,
                                                                           tile_stats, allow_splitk, True)
    o_bf16, o_f32 = (None, _ptr(out)) if is_f32 else (_ptr(out), None)
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous()):
        bias = bias.float().contiguous()
    ws, wsn = None, 0
    if need:
        ws = _workspace(need, x.device, tag=("conv_splitk", torch.cuda.current_stream(x.device).cuda_stream))
        wsn = ws.numel()
    _lib.check(lib.oess_conv2d_fwd_bf16(_ptr(x), ps_in, B, H, W, Cin, _ptr(packed), _ptr(bias), Cout, R, S, stride, pad,
                                        dil, int(relu), _ptr(residual), ps_res, o_bf16, o_f32, ps_out, _ptr(tile_stats),
                                        _ptr(ws), wsn, _stream()),
               "oess_conv2d_fwd_bf16")
    if e0 is not None:
        _timing_stop(e0, (H, W, Cin, Cout, R, stride, dil), 2.0 * B * out.shape[1] * out.shape[2] * Cout * Cin * R * S)
    return out


def conv2d_route(x, packed, bias, Cout, R, S, stride=1, pad=0, dil=1, relu=False, residual=None, out=None,
                 out_f32=False, tile_stats=None, allow_splitk=True, in_pix_stride=None, out_pix_stride=None,
                 res_pix_stride=None, out_aligned16=True):
    """The kernel conv2d_nhwc would launch for these arguments: an OESS_ROUTE_* value of include/oess.h (split-K carries its
    slice count: route & 0xff is the kernel, route >> 8 is ks); raises where the call would.  Host only, needs no GPU.
    With x a tensor the arguments are conv2d_nhwc's own and go through the same marshalling (_conv_marshal): strides, output
    type, alignment and workspace are those of the call.  With x a (B, H, W, Cin) shape, bias / residual / tile_stats are
    booleans and the *_pix_stride / out_aligned16 keywords stand in for the views (default: dense, aligned).
    `packed` is not looked at."""
    lib = _lib.load()
    if torch.is_tensor(x):
        B, H, W, Cin, ps_in, out, f32, ps_out, ps_res, need = _conv_marshal(x, Cout, R, S, stride, pad, dil, residual, out, out_f32,
                                                                            tile_stats, allow_splitk, False)
        has_bias, has_res, stats = bias is not None, residual is not None, tile_stats is not None
        if out is not None:
            out_aligned16 = out.data_ptr() % 16 == 0
    else:
        B, H, W, Cin = x
        has_bias, has_res, stats, f32 = bool(bias), bool(residual), bool(tile_stats), bool(out_f32)
        ps_in = Cin if in_pix_stride is None else in_pix_stride
        ps_out = Cout if out_pix_stride is None else out_pix_stride
        ps_res = (Cout if res_pix_stride is None else res_pix_stride) if has_res else 0
        need = lib.oess_conv2d_fwd_workspace_bytes(B, H, W, Cin, Cout, R, S, stride, pad, dil, int(stats), int(f32)) if allow_splitk else 0
    r = lib.oess_conv2d_fwd_route(B, H, W, Cin, Cout, R, S, stride, pad, dil, int(has_bias), int(relu), int(has_res), int(f32),
                                  int(stats), ps_in, ps_out, ps_res, int(bool(out_aligned16)), need)
    if r < 0:
        _lib.check(r, "oess_conv2d_fwd_route")
    return r


def convlstm_route(xh, C, k, pad, hidden_pix_stride=None, in_pix_stride=None):
    """conv2d_route for convlstm_fused: xh is the cat(x, h) tensor of the call or its (B, H, W, Cin) shape."""
    lib = _lib.load()
    if torch.is_tensor(xh):
        B, H, W, Cin, ps = _nhwc_geom(xh)
    else:
        B, H, W, Cin = xh
        ps = Cin if in_pix_stride is None else in_pix_stride
    r = lib.oess_convlstm_fused_route(B, H, W, Cin, ps, C, k, k, pad, C if hidden_pix_stride is None else hidden_pix_stride)
    if r < 0:
        _lib.check(r, "oess_convlstm_fused_route")
    return r


def conv2d_route_name(route):
    return _lib.load().oess_conv2d_route_name(int(route)).decode()


def e2vid_head_enc0(x8, head_packed, head_bias, head_relu, enc_packed, enc_bias, enc_relu, out=None):
    """E2VID head (5x5, bins -> 32) + encoder 0's conv (5x5 stride 2, 32 -> 64) in one kernel; the head output stays in LDS.
    x8: NHWC bf16 [B, H, W, 8]; out: NHWC bf16 [B, Ho, Wo, 64] view (may be a channel slice)."""
    lib = _lib.load()
    _need_gpu(x8, head_packed, enc_packed)
    B, H, W, C, ps = _nhwc_geom(x8)
    if C != 8:
        raise ValueError("e2vid_head_enc0: x8 must have 8 channels")
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        out = torch.empty((B, Ho, Wo, 64), dtype=torch.bfloat16, device=x8.device)
    _, _, _, Co, ops = _nhwc_geom(out)
    if tuple(out.shape) != (B, Ho, Wo, 64):
        raise ValueError(f"bad output shape {tuple(out.shape)} != {(B, Ho, Wo, 64)}")
    for b_ in (head_bias, enc_bias):
        if b_ is not None and (b_.dtype != torch.float32 or not b_.is_contiguous()):
            raise ValueError("biases must be contiguous fp32")
    _lib.check(lib.oess_e2vid_head_enc0_bf16(_ptr(x8), ps, B, H, W, _ptr(head_packed), _ptr(head_bias), int(bool(head_relu)),
                                             _ptr(enc_packed), _ptr(enc_bias), int(bool(enc_relu)), _ptr(out), ops, _stream()),
               "oess_e2vid_head_enc0_bf16")
    return out


def e2vid_events_head_enc0(events, c0, cs, normalize, head_packed, head_bias, head_relu, enc_packed, enc_bias, enc_relu, out=None,
                           pre=None):
    """e2vid_head_enc0 fed from the fp32 event tensor [B, Ctot, H, W]: the slice's EventPreprocessor normalisation and the
    NHWC8 bf16 packing happen inside the kernel (no intermediate tensor at all between the voxel grid and encoder 0's output).
    pre (EventPre): the patch loader also zeroes the hot pixels and mirrors H and W (K32)."""
    cpre = None if pre is None else _bind_pre(pre, events)
    lib = _lib.load()
    _need_gpu(events, head_packed, enc_packed)
    if events.dtype != torch.float32 or not events.is_contiguous() or events.ndim != 4:
        raise ValueError("needs contiguous float32 [B, C, H, W]")
    B, Ct, H, W = events.shape
    if cs > 5 or c0 < 0 or c0 + cs > Ct:
        raise ValueError("bad channel slice")
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        out = torch.empty((B, Ho, Wo, 64), dtype=torch.bfloat16, device=events.device)
    _, _, _, _, ops = _nhwc_geom(out)
    if tuple(out.shape) != (B, Ho, Wo, 64):
        raise ValueError(f"bad output shape {tuple(out.shape)} != {(B, Ho, Wo, 64)}")
    stats = _slice_stats(events, c0, cs, pre) if normalize else None
    if cpre is not None:
        _lib.check(lib.oess_e2vid_events_head_enc0_pre_bf16(_ptr(events), B, Ct, c0, cs, H, W, ctypes.byref(cpre), _ptr(stats),
                                                            int(bool(normalize)), _ptr(head_packed), _ptr(head_bias),
                                                            int(bool(head_relu)), _ptr(enc_packed), _ptr(enc_bias),
                                                            int(bool(enc_relu)), _ptr(out), ops, _stream()),
                   "oess_e2vid_events_head_enc0_pre_bf16")
        return out
    _lib.check(lib.oess_e2vid_events_head_enc0_bf16(_ptr(events), B, Ct, c0, cs, H, W, _ptr(stats), int(bool(normalize)),
                                                    _ptr(head_packed), _ptr(head_bias), int(bool(head_relu)), _ptr(enc_packed),
                                                    _ptr(enc_bias), int(bool(enc_relu)), _ptr(out), ops, _stream()),
               "oess_e2vid_events_head_enc0_bf16")
    return out


# ------------------------------------------------------------------------------------------ pointwise
def convlstm_gates(gates, cell, hidden_out, prev_cell_is_zero=False):
    """gates: bf16 NHWC [B,H,W,4C]; cell: fp32 [B,H,W,C] (updated in place); hidden_out: bf16 NHWC view
    [B,H,W,C] (may be a channel slice)."""
    lib = _lib.load()
    _need_gpu(gates, cell, hidden_out)
    B, H, W, C4, gs = _nhwc_geom(gates)
    C = C4 // 4
    _, _, _, Ch, hs = _nhwc_geom(hidden_out)
    if Ch != C or cell.dtype != torch.float32 or not cell.is_contiguous() or cell.numel() != B * H * W * C:
        raise ValueError("convlstm_gates: shape mismatch")
    _lib.check(lib.oess_convlstm_gates_bf16(_ptr(gates), gs, None if prev_cell_is_zero else _ptr(cell), _ptr(cell),
                                            _ptr(hidden_out), hs, B * H * W, C, _stream()), "oess_convlstm_gates_bf16")
    return hidden_out


def convlstm_fused(xh, packed_gates, bias, cell, hidden_out, k, pad, prev_cell_is_zero=False):
    """One ConvLSTM step in one kernel (e2vid/model/submodules.py:199-214): Gates conv over xh = cat(x, h_prev)
    (NHWC bf16) + cell update; `packed_gates` = pack_conv_weight(Gates.weight, flip=2) (gate-interleaved rows).
    cell: fp32 [B,H,W,C] updated in place; hidden_out: bf16 NHWC view [B,H,W,C] that must NOT overlap xh."""
    lib = _lib.load()
    e0 = None if _CONV_TIMING is None else _timing_start(lstm=True)
    _need_gpu(xh, packed_gates, cell, hidden_out)
    B, H, W, Cin, ps = _nhwc_geom(xh)
    _, _, _, C, hs = _nhwc_geom(hidden_out)
    if cell.dtype != torch.float32 or not cell.is_contiguous() or cell.numel() != B * H * W * C:
        raise ValueError("convlstm_fused: cell must be contiguous fp32 [B,H,W,C]")
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous() or bias.numel() != 4 * C):
        raise ValueError("convlstm_fused: bias must be contiguous fp32 [4C]")
    _lib.check(lib.oess_convlstm_fused_bf16(_ptr(xh), ps, B, H, W, Cin, _ptr(packed_gates), None if bias is None else _ptr(bias),
                                            C, k, k, pad, None if prev_cell_is_zero else _ptr(cell), _ptr(cell),
                                            _ptr(hidden_out), hs, _stream()), "oess_convlstm_fused_bf16")
    if e0 is not None:
        _timing_stop(e0, (H, W, Cin, 4 * C, k, 1, "lstm"), 2.0 * B * H * W * 4 * C * Cin * k * k)   # the gate convolution's FLOPs only
    return hidden_out


def _convgru_f32_state(t, shape, what):
    if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape):
        raise ValueError(f"{what} must be a contiguous fp32 [B, H, W, C] = {shape} tensor")


def convgru_gates(win, packed_gates, bias, h_master, u, rh_out, k=3, pad=1, h_is_zero=False, rh_f32=None):
    """ConvGRU gates launch (oess_convgru_gates_bf16, K28): u = sigmoid(conv(win, Wu) + bu) -> `u` (fp32 [B, H, W, C]) and
    bf16(sigmoid(conv(win, Wr) + br) * h) -> `rh_out` (NHWC bf16 [B, H, W, C] view, e.g. a channel window of the buffer `win`
    belongs to, but none it convolves).  win: NHWC bf16 view, the (h | x) window or x alone (then h_is_zero).  h_master: the fp32
    [B, H, W, C] hidden state (not read when h_is_zero).  packed_gates: pack_conv_weight of the [2C, Cin, k, k] weight with rows
    2 hc + (0: update, 1: reset), bias [bu | br].  rh_f32: optional fp32 [B, H, W, C] receiving r * h before its rounding."""
    lib = _lib.load()
    _need_gpu(win, packed_gates, bias, h_master, u, rh_out, rh_f32)
    B, H, W, Cin, ps = _nhwc_geom(win)
    _, _, _, C, rs = _nhwc_geom(rh_out)
    for t, what in ((u, "u"), (rh_f32, "rh_f32"), (None if h_is_zero else h_master, "h_master")):
        _convgru_f32_state(t, (B, H, W, C), "convgru_gates: " + what)
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous() or bias.numel() != 2 * C):
        raise ValueError("convgru_gates: bias must be contiguous fp32 [2C]")
    _lib.check(lib.oess_convgru_gates_bf16(_ptr(win), ps, B, H, W, Cin, _ptr(packed_gates), _ptr(bias), C, k, k, pad,
                                           None if h_is_zero else _ptr(h_master), _ptr(u), _ptr(rh_out), rs, _ptr(rh_f32), _stream()),
               "oess_convgru_gates_bf16")
    return u


def convgru_out(win, packed, bias, u, h_master, h_bf16_out, k=3, pad=1, h_is_zero=False):
    """ConvGRU output launch (oess_convgru_out_bf16, K28): h' = h (1 - u) + tanh(conv(win, Wo) + bo) u, in place in `h_master`
    (fp32 [B, H, W, C]; only written when h_is_zero) and rounded to bf16 into `h_bf16_out` (NHWC bf16 view no part of `win`).
    win: NHWC bf16 view, the (x | r h) window or x alone (then h_is_zero); u from convgru_gates."""
    lib = _lib.load()
    _need_gpu(win, packed, bias, u, h_master, h_bf16_out)
    B, H, W, Cin, ps = _nhwc_geom(win)
    _, _, _, C, hs = _nhwc_geom(h_bf16_out)
    for t, what in ((u, "u"), (h_master, "h_master")):
        if t is None:
            raise ValueError(f"convgru_out: {what} is required")
        _convgru_f32_state(t, (B, H, W, C), "convgru_out: " + what)
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous() or bias.numel() != C):
        raise ValueError("convgru_out: bias must be contiguous fp32 [C]")
    _lib.check(lib.oess_convgru_out_bf16(_ptr(win), ps, B, H, W, Cin, _ptr(packed), _ptr(bias), C, k, k, pad, _ptr(u),
                                         None if h_is_zero else _ptr(h_master), _ptr(h_master), _ptr(h_bf16_out), hs, _stream()),
               "oess_convgru_out_bf16")
    return h_bf16_out


def convlstm_w128_cell_elems(pixels, C):
    """Number of fp32 elements of a w128-tiled cell state for `pixels` = B*H*W pixels and C hidden channels (0: C % 64 != 0)."""
    return int(_lib.load().oess_convlstm_w128_cell_bytes(int(pixels), int(C))) // 4


def convlstm_w128_cell_relayout(src, pixels, C, to_tiled):
    """Cell state between the reference's [pixels, C] fp32 order and the w128-tiled order of oess_convlstm_w128_group_bf16."""
    lib = _lib.load()
    _need_gpu(src)
    n = convlstm_w128_cell_elems(pixels, C)
    if n == 0 or src.dtype != torch.float32 or not src.is_contiguous() or src.numel() != (pixels * C if to_tiled else n):
        raise ValueError("convlstm_w128_cell_relayout: contiguous fp32, C % 64 == 0, matching size")
    dst = torch.empty(n if to_tiled else pixels * C, dtype=torch.float32, device=src.device)
    _lib.check(lib.oess_convlstm_w128_cell_relayout(_ptr(src), _ptr(dst), int(pixels), int(C), int(bool(to_tiled)), _stream()),
               "oess_convlstm_w128_cell_relayout")
    return dst


def _convlstm_descs(problems, name, cell_elems):
    """The descriptor array of a grouped ConvLSTM launch from `problems` (tuples as for convlstm_fused_group), with the by-shape
    keys and the FLOPs of its timing entry: (descs, keys, flops).  cell_elems(pixels, C) = the fp32 elements the launch expects in
    `cell` (None: it does not take that C); None is returned at the first cell that is not such a contiguous fp32 tensor."""
    n = len(problems)
    if not 1 <= n <= 3:
        raise ValueError(f"{name}: 1..3 problems")
    descs = (_lib.ConvLstmDesc * n)()
    flops, keys = 0.0, []
    for d, (xh, packed_gates, bias, cell, hidden_out, k, pad, prev_zero) in zip(descs, problems):
        _need_gpu(xh, packed_gates, cell, hidden_out)
        B, H, W, Cin, ps = _nhwc_geom(xh)
        _, _, _, C, hs = _nhwc_geom(hidden_out)
        if cell.dtype != torch.float32 or not cell.is_contiguous() or cell.numel() != cell_elems(B * H * W, C):
            return None
        if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous() or bias.numel() != 4 * C):
            raise ValueError(f"{name}: bias must be contiguous fp32 [4C]")
        d.in_, d.in_pix_stride, d.B, d.H, d.W, d.Cin = _ptr(xh), ps, B, H, W, Cin
        d.w_packed_gates, d.bias, d.C_hidden, d.R, d.S, d.pad = _ptr(packed_gates), _ptr(bias), C, k, k, pad
        d.prev_cell, d.cell, d.hidden, d.hidden_pix_stride = (None if prev_zero else _ptr(cell)), _ptr(cell), _ptr(hidden_out), hs
        flops += 2.0 * B * H * W * 4 * C * Cin * k * k
        keys.append((H, W, Cin, 4 * C, k, 1, "lstm"))
    return descs, ("group",) + tuple(keys), flops


def convlstm_w128_group(problems):
    """oess_convlstm_w128_group_bf16: `problems` as for convlstm_fused_group, except that `cell` is a flat fp32 tensor of
    convlstm_w128_cell_elems(B*H*W, C) elements in the w128-tiled layout.  Returns False (nothing launched) when the kernel does not
    take one of the problems; the caller then uses convlstm_fused_group on NHWC cells."""
    lib = _lib.load()
    m = _convlstm_descs(problems, "convlstm_w128_group", lambda px, C: None if C % 64 else convlstm_w128_cell_elems(px, C))
    if m is None:
        return False
    e0 = None if _CONV_TIMING is None else _timing_start(lstm=True)
    rc = lib.oess_convlstm_w128_group_bf16(ctypes.addressof(m[0]), len(problems), _stream())
    if rc == -22:                     # OESS_EINVAL: geometry not taken, nothing launched
        return False
    _lib.check(rc, "oess_convlstm_w128_group_bf16")
    if e0 is not None:
        _timing_stop(e0, m[1], m[2])
    return True


def convlstm_fused_group(problems):
    """Up to three INDEPENDENT ConvLSTM steps in one launch (oess_convlstm_fused_group_bf16): `problems` = tuples
    (xh, packed_gates, bias, cell, hidden_out, k, pad, prev_cell_is_zero) as for convlstm_fused.  Same results as calling
    convlstm_fused on each (the levels of E2VID's recurrent encoder on the skewed schedule, e2vid/model/unet.py mirror)."""
    lib = _lib.load()
    m = _convlstm_descs(problems, "convlstm_fused_group", lambda px, C: px * C)
    if m is None:
        raise ValueError("convlstm_fused_group: cell must be contiguous fp32 [B,H,W,C]")
    e0 = None if _CONV_TIMING is None else _timing_start(lstm=True)
    _lib.check(lib.oess_convlstm_fused_group_bf16(ctypes.addressof(m[0]), len(problems), _stream()), "oess_convlstm_fused_group_bf16")
    if e0 is not None:
        _timing_stop(e0, m[1], m[2])
    return [p[4] for p in problems]


def conv5x5s2_group(problems):
    """Up to two INDEPENDENT 5x5 / stride-2 / pad-2 convolutions in one launch (oess_conv5x5s2_group_bf16): `problems` = tuples
    (x NHWC bf16, packed weight, bias | None, Cout, relu, out NHWC bf16 view).  Same results as conv2d_nhwc on each."""
    lib = _lib.load()
    n = len(problems)
    if not 1 <= n <= 2:
        raise ValueError("conv5x5s2_group: 1..2 problems")
    descs = (_lib.ConvS2Desc * n)()
    flops, keys = 0.0, []
    for d, (x, packed, bias, Cout, relu, out) in zip(descs, problems):
        _need_gpu(x, packed, out)
        B, H, W, Cin, ps = _nhwc_geom(x)
        Bo, Ho, Wo, Co, ops = _nhwc_geom(out)
        if (Bo, Ho, Wo, Co) != (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cout):
            raise ValueError("conv5x5s2_group: output view must be [B, (H-1)//2+1, (W-1)//2+1, Cout]")
        if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous() or bias.numel() < Cout):
            raise ValueError("conv5x5s2_group: bias must be contiguous fp32 [Cout]")
        d.in_, d.in_pix_stride, d.B, d.H, d.W, d.Cin = _ptr(x), ps, B, H, W, Cin
        d.w_packed, d.bias, d.Cout, d.relu, d.out, d.out_pix_stride = _ptr(packed), _ptr(bias), Cout, int(bool(relu)), _ptr(out), ops
        fl = 2.0 * B * Ho * Wo * Cout * Cin * 25
        if Cout > 64:
            flops += fl
            keys.append((H, W, Cin, Cout, 5, 2, 1))
    e0 = None if _CONV_TIMING is None or flops <= 0 else _timing_start(lstm=False)
    _lib.check(lib.oess_conv5x5s2_group_bf16(ctypes.addressof(descs), n, _stream()), "oess_conv5x5s2_group_bf16")
    if e0 is not None:
        _timing_stop(e0, ("group",) + tuple(keys), flops)
    return [p[5] for p in problems]


_SLICE_STATS = {}


def masked_stats_slices(events, cs, index=None, pre=None):
    """{sum, sumsq, nnz, -} of every cs-channel slice of a contiguous fp32 [B, Ctot, H, W] tensor in ONE launch -> float64
    [Ctot // cs, 4]; with `index` the row of that slice.  pre (EventPre): its hot pixels add nothing (the flip does not change
    statistics); the mask is part of the cache key below.
    The table is cached ONLY for the access pattern it exists for -- a sub-window loop walking the slices of one tensor in order
    (0, 1, 2, ...): a request is served from the cache iff the tensor's (pointer, version, shape) are unchanged AND `index` is
    exactly the successor of the previous request.  Anything else -- slice 0 (a new loop: the voxelizer rewrites the same
    allocation every batch with the same version), a loop entered in the middle, a repeated or skipped slice, `index=None` --
    recomputes, so stale statistics of a previous batch cannot be served to a caller that does not start at slice 0."""
    cpre = None if pre is None else _bind_pre(pre, events)
    lib = _lib.load()
    B, Ct, H, W = events.shape
    key = (events.device.index, torch.cuda.current_stream(events.device).cuda_stream)
    tag = (events.data_ptr(), events._version, tuple(events.shape), cs)
    if pre is not None and pre.tag() is not None:
        tag = tag + (pre.tag(),)
    hit = _SLICE_STATS.get(key)
    if hit is not None and hit[0] == tag and index is not None and index > 0 and index == hit[2]:
        hit[2] = index + 1
        return hit[1][index]
    n = Ct // cs
    buf = torch.empty(lib.oess_masked_stats_doubles(n), dtype=torch.float64, device=events.device)   # totals + partial rows
    if cpre is not None:
        _need_gpu(events)
        if events.dtype != torch.float32 or not events.is_contiguous():
            raise ValueError("needs contiguous float32 [B, C, H, W]")
        _lib.check(lib.oess_masked_stats_slices_pre_f32(_ptr(events), B, Ct, cs, n, H, W, ctypes.byref(cpre), _ptr(buf), _stream()),
                   "oess_masked_stats_slices_pre_f32")
    else:
        _lib.check(lib.oess_masked_stats_slices_f32(_ptr(events), B, Ct, cs, n, H * W, _ptr(buf), _stream()),
                   "oess_masked_stats_slices_f32")
    stats = buf[:4 * n].view(n, 4)
    _SLICE_STATS[key] = [tag, stats, (index + 1) if index is not None else -1]
    return stats if index is None else stats[index]


def masked_stats_slice(events, c0, cs, pre=None):
    """{sum, sumsq, nnz, -} (float64, on the device) of the one slice events[:, c0:c0+cs] of a contiguous fp32 [B, Ctot, H, W]
    tensor, by a launch of its own.  pre (EventPre): its hot pixels add nothing."""
    cpre = None if pre is None else _bind_pre(pre, events)
    lib = _lib.load()
    _need_gpu(events)
    if events.dtype != torch.float32 or not events.is_contiguous() or events.ndim != 4:
        raise ValueError("needs contiguous float32 [B, C, H, W]")
    B, Ct, H, W = events.shape
    stats = torch.empty(lib.oess_masked_stats_doubles(1), dtype=torch.float64, device=events.device)
    if cpre is not None:
        _lib.check(lib.oess_masked_stats_slice_pre_f32(_ptr(events), B, Ct, c0, cs, H, W, ctypes.byref(cpre), _ptr(stats), _stream()),
                   "oess_masked_stats_slice_pre_f32")
        return stats
    _lib.check(lib.oess_masked_stats_slice_f32(_ptr(events), B, Ct, c0, cs, H * W, _ptr(stats), _stream()),
               "oess_masked_stats_slice_f32")
    return stats


def _slice_stats(events, c0, cs, pre=None):
    """The EventPreprocessor statistics of events[:, c0:c0+cs]: a row of the table of all slices when the tensor is a whole
    number of cs-channel slices (masked_stats_slices), otherwise one launch for this slice alone."""
    B, Ct, H, W = events.shape
    if Ct > cs and Ct % cs == 0 and c0 % cs == 0:
        return masked_stats_slices(events, cs, index=c0 // cs, pre=pre)
    return masked_stats_slice(events, c0, cs, pre=pre)


def event_slice_to_nhwc8(events, c0, cs, normalize=True, out=None, pre=None):
    """events: contiguous fp32 [B, Ctot, H, W]; returns logical [B, 8, H, W] channels_last bf16 holding the
    (optionally EventPreprocessor-normalised) slice events[:, c0:c0+cs], zero padded to 8 channels.
    When the tensor is a whole number of cs-channel slices (the sub-windows of one sample) the statistics of ALL slices are
    formed by one launch at the first request and reused for the others.
    pre (EventPre): hot pixels zeroed and H, W mirrored first, also with normalize=False (K32)."""
    cpre = None if pre is None else _bind_pre(pre, events)
    lib = _lib.load()
    _need_gpu(events)
    if events.dtype != torch.float32 or not events.is_contiguous() or events.ndim != 4:
        raise ValueError("needs contiguous float32 [B, C, H, W]")
    B, Ct, H, W = events.shape
    if out is None:
        out = torch.empty((B, H, W, 8), dtype=torch.bfloat16, device=events.device)
    stats = _slice_stats(events, c0, cs, pre) if normalize else None
    if cpre is not None:
        _lib.check(lib.oess_event_slice_to_nhwc8_pre_bf16(_ptr(events), B, Ct, c0, cs, H, W, ctypes.byref(cpre), _ptr(stats),
                                                          int(normalize), _ptr(out), _stream()), "oess_event_slice_to_nhwc8_pre_bf16")
        return out.permute(0, 3, 1, 2)
    _lib.check(lib.oess_event_slice_to_nhwc8_bf16(_ptr(events), B, Ct, c0, cs, H * W, _ptr(stats), int(normalize),
                                                  _ptr(out), _stream()), "oess_event_slice_to_nhwc8_bf16")
    return out.permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------ timing hooks
_CONV_TIMING = None


def conv_timing_begin(lstm_only=False):
    """bench.py: bracket every launch of the conv family (Cout > 64) with HIP events on the launch stream; resolved after the
    timed region (no sync inside it).  lstm_only: only the fused-ConvLSTM launches (the dominant kernel) -- an event record is a
    barrier packet of its own, ~2.8 us of idle queue each: 2 x 115 of them are 1.3 ms of a one-stream step."""
    global _CONV_TIMING
    _CONV_TIMING = {"events": [], "flops": 0.0, "keys": [], "lstm_only": bool(lstm_only)}


def _timing_start(lstm):
    """First half of the bracket around one launch of the family, for callers that have seen _CONV_TIMING set: the recorded
    start event, or None when only the dominant kernel is bracketed and this is not a ConvLSTM launch."""
    if _CONV_TIMING["lstm_only"] and not lstm:
        return None
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0


def _timing_stop(e0, key, flops):
    """Second half: the end event, and the launch with its by-shape key and FLOPs into the timing record."""
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    t = _CONV_TIMING
    t["events"].append((e0, e1))
    t["flops"] += flops
    t["keys"].append((key, flops))


def conv_timing_end():
    global _CONV_TIMING
    t = _CONV_TIMING
    _CONV_TIMING = None
    if not t:
        return None
    torch.cuda.synchronize()
    times = [a.elapsed_time(b) for a, b in t["events"]]
    ms = sum(times)
    by = {}
    for (k, fl), tm in zip(t["keys"], times):
        e = by.setdefault(k, [0, 0.0, 0.0])
        e[0] += 1; e[1] += tm; e[2] += fl
    return {"ms": ms, "flops": t["flops"], "launches": len(t["events"]), "by_shape": by}


# ------------------------------------------------------------------------------------------ ViT pieces (MaskCLIP tower)
def _check_token_out(what, out, like, shape):
    """A caller's `out` is written through its raw pointer: refuse anything the kernel would write outside of."""
    if not isinstance(out, torch.Tensor) or out.dtype != torch.bfloat16 or out.device != like.device or tuple(out.shape) != tuple(shape) \
            or out.stride(1) != 1 or (shape[0] > 1 and out.stride(0) < shape[1]):
        raise ValueError(f"{what}: out must be bf16 {list(shape)} with dense channels on {like.device}")


def _check_affine(what, name, p, C, like):
    if not isinstance(p, torch.Tensor) or p.dtype != torch.float32 or p.device != like.device or tuple(p.shape) != (C,) \
            or not p.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous fp32 [{C}] on {like.device}")


def layer_norm_tokens(x, gamma, beta, eps=1e-6, out=None):
    """nn.LayerNorm over the last axis of a bf16 token matrix [rows, C] (row-strided views are fine)."""
    lib = _lib.load()
    if x.dtype != torch.bfloat16 or x.ndim != 2 or x.stride(1) != 1:
        raise ValueError("layer_norm_tokens: bf16 [rows, C] with dense channels")
    rows, C = x.shape
    _check_affine("layer_norm_tokens", "gamma", gamma, C, x)
    _check_affine("layer_norm_tokens", "beta", beta, C, x)
    if out is not None:
        _check_token_out("layer_norm_tokens", out, x, (rows, C))
    _need_gpu(x)
    if out is None:
        out = torch.empty((rows, C), dtype=torch.bfloat16, device=x.device)
    _lib.check(lib.oess_layernorm_bf16(_ptr(x), x.stride(0), rows, C, _ptr(gamma), _ptr(beta), float(eps), _ptr(out), out.stride(0),
                                       _stream()), "oess_layernorm_bf16")
    return out


def attention_d64(qkv, B, L, heads, out=None):
    """softmax(Q K^T / 8) V per head (head dim 64) from nn.MultiheadAttention's packed in_proj output [B*L, 3*heads*64]
    (bf16) -> [B*L, heads*64] (bf16), i.e. the attention output before out_proj."""
    lib = _lib.load()
    C = heads * 64
    if qkv.dtype != torch.bfloat16 or qkv.ndim != 2 or qkv.shape != (B * L, 3 * C) or qkv.stride(1) != 1:
        raise ValueError("attention_d64: qkv must be bf16 [B*L, 3*heads*64]")
    if out is not None:
        _check_token_out("attention_d64", out, qkv, (B * L, C))
    _need_gpu(qkv)
    if out is None:
        out = torch.empty((B * L, C), dtype=torch.bfloat16, device=qkv.device)
    _lib.check(lib.oess_attention_d64_bf16(_ptr(qkv), qkv.stride(0), B, L, heads, 0.125, _ptr(out), out.stride(0), _stream()),
               "oess_attention_d64_bf16")
    return out


# ---- K25: the same pieces on fp32 tokens (the tower's forward_fp32)
def _check_tokens_f32(what, name, t, shape=None, like=None):
    """fp32 [rows, C] with dense channels, rows at least C apart and 16-byte aligned (the vector accesses of the kernels)"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.ndim != 2 or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = "[rows, C]" if shape is None else str(list(shape))
        raise ValueError(f"{what}: {name} must be fp32 {want}")
    if like is not None and t.device != like.device:
        raise ValueError(f"{what}: {name} must be on {like.device}")
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what}: {name} must not be empty")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{what}: {name} must have dense channels and a row stride >= {t.shape[1]}")


def _token_stride(t):
    """row stride handed to a kernel: a single row's is its width (torch reports anything for a size-1 axis)"""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def layer_norm_tokens_f32(x, gamma, beta, eps=1e-6, out=None):
    """nn.LayerNorm over the last axis of an fp32 token matrix [rows, C], C <= 2048 (row-strided views are fine; 16-byte
    accesses when C, the strides and the addresses allow, oess_layernorm_f32)."""
    lib = _lib.load()
    _check_tokens_f32("layer_norm_tokens_f32", "x", x)
    rows, C = x.shape
    if C > 2048:
        raise ValueError("layer_norm_tokens_f32: x has more than 2048 channels")
    _check_affine("layer_norm_tokens_f32", "gamma", gamma, C, x)
    _check_affine("layer_norm_tokens_f32", "beta", beta, C, x)
    if not eps > 0:
        raise ValueError("layer_norm_tokens_f32: eps must be positive")
    if out is not None:
        _check_tokens_f32("layer_norm_tokens_f32", "out", out, (rows, C), x)
    _need_gpu(x)
    if out is None:
        out = torch.empty((rows, C), dtype=torch.float32, device=x.device)
    _lib.check(lib.oess_layernorm_f32(_ptr(x), _token_stride(x), rows, C, _ptr(gamma), _ptr(beta), float(eps), _ptr(out),
                                      _token_stride(out), _stream()), "oess_layernorm_f32")
    return out


def attention_d64_f32(qkv, B, L, heads, out=None, causal=False):
    """softmax(Q K^T / 8) V per head (head dim 64) from the packed in_proj output [B*L, 3*heads*64] in fp32 -> [B*L, heads*64]
    fp32 on the f32-input MFMA (oess_attention_d64_f32): fp32 products, fp32 softmax, no rounding in between.  causal (K29):
    query i of a sequence sees keys 0 .. i of it (oess_attention_d64_causal_f32, the text tower's mask)."""
    lib = _lib.load()
    if not all(isinstance(v, int) and v >= 1 for v in (B, L, heads)):
        raise ValueError("attention_d64_f32: B, L and heads must be positive integers")
    if not isinstance(causal, bool):
        raise ValueError("attention_d64_f32: causal must be a bool")
    C = heads * 64
    _check_tokens_f32("attention_d64_f32", "qkv", qkv, (B * L, 3 * C))
    if _token_stride(qkv) % 4 or qkv.data_ptr() % 16:
        raise ValueError("attention_d64_f32: qkv rows must be 16-byte aligned (row stride a multiple of 4 floats)")
    if out is not None:
        _check_tokens_f32("attention_d64_f32", "out", out, (B * L, C), qkv)
        if _token_stride(out) % 4 or out.data_ptr() % 16:
            raise ValueError("attention_d64_f32: out rows must be 16-byte aligned (row stride a multiple of 4 floats)")
    _need_gpu(qkv)
    if out is None:
        out = torch.empty((B * L, C), dtype=torch.float32, device=qkv.device)
    name = "oess_attention_d64_causal_f32" if causal else "oess_attention_d64_f32"
    _lib.check(getattr(lib, name)(_ptr(qkv), _token_stride(qkv), B, L, heads, 0.125, _ptr(out), _token_stride(out), _stream()), name)
    return out


_F32_TOKEN_ACT = {None: 0, 'gelu': 1, 'quick_gelu': None}       # quick_gelu (K29) is an entry of its own, not an `act` code


def linear_tokens_f32(x, packed, bias, Cout, act=None, residual=None, out=None):
    """y = act(x W^T + b [+ residual]) for fp32 tokens x [rows, Cin] on the fp32 conv kernel (oess_linear_tokens_f32).  packed:
    pack_conv_weight_f32(W[:, :, None, None]); act: None or 'gelu' (exact, nn.GELU's default); bias [Cout] and residual
    [rows, Cout] optional; x, residual and out may be row-strided.  act None gives conv2d_f32(..., R=S=1)'s bits.
    act 'quick_gelu': v sigmoid(1.702 v), CLIP's activation (oess_linear_tokens_quick_gelu_f32)."""
    lib = _lib.load()
    _check_tokens_f32("linear_tokens_f32", "x", x)
    rows, Cin = x.shape
    if not isinstance(Cout, int) or Cout < 1:
        raise ValueError("linear_tokens_f32: Cout must be a positive integer")
    need = lib.oess_conv2d_f32_packed_floats(Cout, Cin, 1, 1)
    if not isinstance(packed, torch.Tensor) or packed.dtype != torch.float32 or packed.device != x.device or not packed.is_contiguous() \
            or need == 0 or packed.numel() < need:
        raise ValueError(f"linear_tokens_f32: packed must be a contiguous fp32 tensor of at least {need} floats on {x.device}")
    if bias is not None:
        _check_affine("linear_tokens_f32", "bias", bias, Cout, x)
    if act not in _F32_TOKEN_ACT:
        raise ValueError(f"linear_tokens_f32: act must be one of {list(_F32_TOKEN_ACT)}")
    if residual is not None:
        _check_tokens_f32("linear_tokens_f32", "residual", residual, (rows, Cout), x)
    if out is not None:
        _check_tokens_f32("linear_tokens_f32", "out", out, (rows, Cout), x)
    _need_gpu(x)
    if out is None:
        out = torch.empty((rows, Cout), dtype=torch.float32, device=x.device)
    if act == 'quick_gelu':
        _lib.check(lib.oess_linear_tokens_quick_gelu_f32(_ptr(x), _token_stride(x), rows, Cin, _ptr(packed), _ptr(bias), Cout,
                                                         _ptr(residual), 0 if residual is None else _token_stride(residual),
                                                         _ptr(out), _token_stride(out), _stream()), "oess_linear_tokens_quick_gelu_f32")
        return out
    _lib.check(lib.oess_linear_tokens_f32(_ptr(x), _token_stride(x), rows, Cin, _ptr(packed), _ptr(bias), Cout, _F32_TOKEN_ACT[act],
                                          _ptr(residual), 0 if residual is None else _token_stride(residual), _ptr(out),
                                          _token_stride(out), _stream()), "oess_linear_tokens_f32")
    return out


# ---- K29: what CLIP's text tower needs next to the token kernels above
def _check_ids(what, ids, like=None):
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.ndim != 2 or ids.shape[0] < 1 or ids.shape[1] < 1 \
            or not ids.is_contiguous():
        raise ValueError(f"{what}: ids must be contiguous int64 [N, L]")
    if like is not None and ids.device != like.device:
        raise ValueError(f"{what}: ids must be on {like.device}")


def clip_text_embed(ids, token_embedding, positional_embedding, out=None):
    """x[n L + t, :] = token_embedding[ids[n, t], :] + positional_embedding[t, :]: int64 ids [N, L], fp32 table [V, C] and positions
    [>= L, C] -> fp32 [N L, C] (oess_clip_text_embed_f32; one add per element, exact).  An id outside [0, V) or more tokens than
    positions is a ValueError before the launch (reading the ids back synchronises once)."""
    lib = _lib.load()
    what = "clip_text_embed"
    _check_tokens_f32(what, "token_embedding", token_embedding)
    V, C = token_embedding.shape
    _check_ids(what, ids, token_embedding)
    N, L = ids.shape
    if not isinstance(positional_embedding, torch.Tensor) or positional_embedding.ndim != 2 or positional_embedding.shape[1] != C:
        raise ValueError(f"{what}: positional_embedding must be fp32 [>= L, {C}]")
    _check_tokens_f32(what, "positional_embedding", positional_embedding, like=token_embedding)
    if L > positional_embedding.shape[0]:
        raise ValueError(f"{what}: {L} tokens per text, positional_embedding has {positional_embedding.shape[0]} rows")
    lo, hi = int(ids.min()), int(ids.max())
    if lo < 0 or hi >= V:
        raise ValueError(f"{what}: ids must lie in [0, {V}), got {lo} .. {hi}")
    if out is not None:
        _check_tokens_f32(what, "out", out, (N * L, C), token_embedding)
    _need_gpu(token_embedding)
    if out is None:
        out = torch.empty((N * L, C), dtype=torch.float32, device=ids.device)
    _lib.check(lib.oess_clip_text_embed_f32(_ptr(ids), N, L, _ptr(token_embedding), _token_stride(token_embedding), V, C,
                                            _ptr(positional_embedding), _token_stride(positional_embedding), _ptr(out),
                                            _token_stride(out), _stream()), "oess_clip_text_embed_f32")
    return out


def clip_text_eot_norm(x, ids, gamma, beta, eps=1e-5, out=None):
    """LayerNorm of the end-of-text row of each text: x fp32 [N L, C] (C <= 2048), ids int64 [N, L]; row argmax_t ids[n, t] (the
    first maximum, as torch.argmax) of text n, normalised like layer_norm_tokens_f32 -> fp32 [N, C]
    (oess_clip_text_eot_layernorm_f32; the other N (L - 1) rows are not touched)."""
    lib = _lib.load()
    what = "clip_text_eot_norm"
    _check_tokens_f32(what, "x", x)
    _check_ids(what, ids, x)
    N, L = ids.shape
    C = x.shape[1]
    if x.shape[0] != N * L:
        raise ValueError(f"{what}: x must be fp32 [{N * L}, C] for ids {list(ids.shape)}")
    if C > 2048:
        raise ValueError(f"{what}: x has more than 2048 channels")
    _check_affine(what, "gamma", gamma, C, x)
    _check_affine(what, "beta", beta, C, x)
    if not eps > 0:
        raise ValueError(f"{what}: eps must be positive")
    if out is not None:
        _check_tokens_f32(what, "out", out, (N, C), x)
    _need_gpu(x)
    if out is None:
        out = torch.empty((N, C), dtype=torch.float32, device=x.device)
    _lib.check(lib.oess_clip_text_eot_layernorm_f32(_ptr(x), _token_stride(x), _ptr(ids), N, L, C, _ptr(gamma), _ptr(beta), float(eps),
                                                    _ptr(out), _token_stride(out), _stream()), "oess_clip_text_eot_layernorm_f32")
    return out


def prompt_mean_normalize(e, group_offsets, out=None):
    """out[k] = normalize(sum over the prompts n of class k of normalize(e[n])): e fp32 [N, D] (D <= 2048), group_offsets int64
    [K + 1] (ascending from 0 to N, no empty class; CPU or GPU) -> fp32 [K, D] unit rows (oess_prompt_mean_normalize_f32; a class's
    prompts are added in their order, so the result repeats bit for bit)."""
    lib = _lib.load()
    what = "prompt_mean_normalize"
    _check_tokens_f32(what, "e", e)
    N, D = e.shape
    if D > 2048:
        raise ValueError(f"{what}: e has more than 2048 channels")
    if not isinstance(group_offsets, torch.Tensor) or group_offsets.dtype != torch.int64 or group_offsets.ndim != 1 \
            or group_offsets.numel() < 2:
        raise ValueError(f"{what}: group_offsets must be int64 [K + 1]")
    host = group_offsets.cpu().contiguous()
    K = host.numel() - 1
    if int(host[0]) != 0 or int(host[-1]) != N or bool((host[1:] <= host[:-1]).any()):
        raise ValueError(f"{what}: group_offsets must ascend strictly from 0 to {N}")
    if out is not None:
        _check_tokens_f32(what, "out", out, (K, D), e)
    _need_gpu(e)
    dev = group_offsets.contiguous() if group_offsets.device == e.device else host.to(e.device)
    if out is None:
        out = torch.empty((K, D), dtype=torch.float32, device=e.device)
    _lib.check(lib.oess_prompt_mean_normalize_f32(_ptr(e), _token_stride(e), N, D, _ptr(host), _ptr(dev), K, _ptr(out),
                                                  _token_stride(out), _stream()), "oess_prompt_mean_normalize_f32")
    return out


# ---- K26: MaskCLIP's refinement of the class logits (prompt denoising + key smoothing)
MASKCLIP_REFINE_MAX_K, MASKCLIP_REFINE_MAX_L, MASKCLIP_REFINE_MAX_C = 32, 4096, 1024
_REFINE_K_DTYPE = {torch.float32: 0, torch.bfloat16: 1}        # OESS_MASKCLIP_K_F32 / OESS_MASKCLIP_K_BF16


def _distinct_elements(t):
    """no two index tuples of `t` share an address: sorted by stride, every stride clears the span of the smaller ones"""
    span = 0
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s > 1), key=lambda p: p[1]):
        if stride <= span:
            return False
        span += (size - 1) * stride
    return True


def _byte_range(t):
    lo = t.data_ptr()
    return lo, lo + (sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1) * t.element_size()


def _maskclip_refine_check(logits, k, pd_thresh, ks_thresh, out):
    what = "maskclip_refine"
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.ndim != 4:
        raise ValueError(f"{what}: logits must be fp32 [B, K, H, W]")
    B, K, H, W = logits.shape
    if B < 1 or not 1 <= K <= MASKCLIP_REFINE_MAX_K or H < 1 or W < 1 or H * W > MASKCLIP_REFINE_MAX_L:
        raise ValueError(f"{what}: logits {tuple(logits.shape)} outside B >= 1, 1 <= K <= {MASKCLIP_REFINE_MAX_K}, "
                         f"1 <= H W <= {MASKCLIP_REFINE_MAX_L}")
    if any(s < 0 for s in logits.stride()):
        raise ValueError(f"{what}: logits must not have negative strides")
    for name, v in (("pd_thresh", pd_thresh), ("ks_thresh", ks_thresh)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v < float("inf"):
            raise ValueError(f"{what}: {name} must be a finite number >= 0, got {v!r}")
    C = 0
    if k is not None:
        if not isinstance(k, torch.Tensor) or k.dtype not in _REFINE_K_DTYPE or k.ndim != 3 or k.device != logits.device:
            raise ValueError(f"{what}: k must be fp32 or bf16 [B, H W, C] on {logits.device}")
        C = k.shape[2]
        if tuple(k.shape[:2]) != (B, H * W) or C < 64 or C % 64 or C > MASKCLIP_REFINE_MAX_C:
            raise ValueError(f"{what}: k {tuple(k.shape)} must be [{B}, {H * W}, C] with C a multiple of 64 up to {MASKCLIP_REFINE_MAX_C}")
        if k.stride(2) != 1 or (H * W > 1 and k.stride(1) < C) or (B > 1 and k.stride(0) < (H * W - 1) * k.stride(1) + C):
            raise ValueError(f"{what}: k must have dense channels, a row stride >= {C} and images that do not overlap")
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != logits.device \
                or tuple(out.shape) != (B, K, H, W) or any(s < 0 for s in out.stride()) or not _distinct_elements(out):
            raise ValueError(f"{what}: out must be fp32 {[B, K, H, W]} on {logits.device} with distinct elements")
        (a0, a1), (b0, b1) = _byte_range(out), _byte_range(logits)
        if a0 < b1 and b0 < a1:
            raise ValueError(f"{what}: out must not overlap logits")
    return B, K, H, W, C


def _maskclip_refine_args(logits, k, out, C):
    B, K, H, W = logits.shape
    L = H * W
    krs = kis = 0
    if k is not None:
        krs = k.stride(1) if L > 1 else C
        kis = k.stride(0) if B > 1 else L * krs
    return (_ptr(logits), *logits.stride(), B, K, H, W, _ptr(k), _REFINE_K_DTYPE[k.dtype] if k is not None else 0, krs, kis, C)


def maskclip_refine(logits, k, pd_thresh=0.5, ks_thresh=1.0, out=None):
    """MaskCLIP's test-time refinement (MaskClipHead.refine_output of the reference, oess_maskclip_refine_f32).
    logits: fp32 [B, K, H, W], any strides.  Prompt denoising (pd_thresh > 0): a class whose softmax(100 logits) confidence stays
    below pd_thresh on every pixel of an image gets the logit -100 there.  Key smoothing (k given and ks_thresh > 0): P =
    softmax(100 denoised logits); k: the last layer's keys [B, H W, C] in fp32 or bf16 as a strided view (dense channels), each
    channel divided by max(its norm over the tokens, 1e-12); a pixel with max P < ks_thresh takes its row of (k^ k^T) P.
    Returns probabilities [B, K, H, W] in the logits' layout when smoothing runs, the denoised logits otherwise.  The input is
    not modified (the reference writes the -100 rows into it).  fp32 arithmetic, no atomics: two calls give the same bits."""
    B, K, H, W, C = _maskclip_refine_check(logits, k, pd_thresh, ks_thresh, out)
    _need_gpu(logits, k, out)
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(logits)
        if not _distinct_elements(out):                  # a broadcast input: empty_like keeps its zero strides
            out = torch.empty(logits.shape, dtype=torch.float32, device=logits.device)
    ws = _workspace(lib.oess_maskclip_refine_workspace_bytes(B, K, H, W, C), logits.device, tag="maskclip_refine")
    _lib.check(lib.oess_maskclip_refine_f32(*_maskclip_refine_args(logits, k, out, C), float(pd_thresh), float(ks_thresh), _ptr(out),
                                            *out.stride(), _ptr(ws), ws.numel(), _stream()), "oess_maskclip_refine_f32")
    _bump(out)
    return out


def maskclip_refine_phase_ms(logits, k, pd_thresh=0.5, ks_thresh=1.0):
    """Milliseconds of the five kernels of one hip.maskclip_refine call (confidence | mask + softmax | k^T P per chunk | chunk sum
    + norms | k Hm + select), HIP events between the same launches.  Synchronises: a measurement aid."""
    B, K, H, W, C = _maskclip_refine_check(logits, k, pd_thresh, ks_thresh, None)
    _need_gpu(logits, k)
    lib = _lib.load()
    out = torch.empty(logits.shape, dtype=torch.float32, device=logits.device)
    ws = _workspace(lib.oess_maskclip_refine_workspace_bytes(B, K, H, W, C), logits.device, tag="maskclip_refine")
    ms = (ctypes.c_float * 5)()
    _lib.check(lib.oess_maskclip_refine_phase_ms(*_maskclip_refine_args(logits, k, out, C), float(pd_thresh), float(ks_thresh), _ptr(out),
                                                 *out.stride(), _ptr(ws), ws.numel(), ms, _stream()), "oess_maskclip_refine_phase_ms")
    return dict(zip(("conf", "prob", "gram", "hm", "apply"), (float(v) for v in ms)))


# scratch of oess_norm_reduce_finalize_tile_stats (per-slice double sums + last-block tickets; tickets are kept zero by the kernel)
_STATS_SCRATCH = {}


class _StatsScratch:
    def __init__(self, n, device):
        self.buf64 = torch.zeros((64, n), dtype=torch.float64, device=device)      # [32 slices][2][C]
        self.tickets = torch.zeros(((n + 31) // 32,), dtype=torch.int32, device=device)


def _stats_scratch(n, device):
    # stream-ordered reuse is only safe on one stream: key by the current stream as well
    key = (device.index, n, torch.cuda.current_stream(device).cuda_stream)
    sc = _STATS_SCRATCH.get(key)
    if sc is None:
        sc = _STATS_SCRATCH[key] = _StatsScratch(n, device)
    return sc


def _norm_partials(G, ppg, C, device, backward=False):
    """Workspace of the deterministic statistics kernels (per-workgroup partial sums, reduced in a fixed order)."""
    lib = _lib.load()
    nbytes = lib.oess_norm_partials_bytes(G, ppg, C, int(backward))
    ws = _workspace(nbytes, device, tag=("norm_part", torch.cuda.current_stream(device).cuda_stream))
    return ws, ws.numel()


# ------------------------------------------------------------------------------------------ norms / resampling
def _norm_forward(x_nhwc, G, gamma, beta, eps, relu, residual, running=None, momentum=0.1, out=None):
    """Shared BatchNorm(train)/InstanceNorm forward on an NHWC bf16 view.  Returns (out, mean, rstd)."""
    lib = _lib.load()
    B, H, W, C, ps = _nhwc_geom(x_nhwc)
    ppg = (B * H * W) // G
    dev = x_nhwc.device
    stats = torch.empty((6, G, C), dtype=torch.float32, device=dev)        # (unused, unused), mean, rstd, scale, shift
    rm = rv = None
    if running is not None:
        rm, rv = running
    ws, wsn = _norm_partials(G, ppg, C, dev)
    _lib.check(lib.oess_norm_stats_finalize_nhwc_bf16(_ptr(x_nhwc), ps, G, ppg, C, float(eps), _ptr(gamma), _ptr(beta), _ptr(rm),
                                                      _ptr(rv), float(momentum), _ptr(stats[2]), _ptr(stats[3]), _ptr(stats[4]),
                                                      _ptr(stats[5]), _ptr(ws), wsn, _stream()),
               "oess_norm_stats_finalize_nhwc_bf16")
    if out is None:
        out = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=dev)
    _, _, _, _, ops = _nhwc_geom(out)
    rps = 0
    if residual is not None:
        _, _, _, _, rps = _nhwc_geom(residual)
    _lib.check(lib.oess_norm_apply_nhwc_bf16(_ptr(x_nhwc), ps, _ptr(stats[4]), _ptr(stats[5]), _ptr(residual), rps, int(relu),
                                             G, ppg, C, _ptr(out), ops, _stream()), "oess_norm_apply_nhwc_bf16")
    return out, stats[2], stats[3]


def batch_norm_train_nhwc(x_nhwc, bn, relu=False, residual=None):
    """nn.BatchNorm2d in TRAIN mode (batch statistics, running-stat update), inference-only (no autograd):
    the frozen teacher encoder (image_model.py:113-114 freezes it but leaves it in .train())."""
    out, _, _ = _norm_forward(x_nhwc, 1, bn.weight.detach(), bn.bias.detach(), bn.eps, relu, residual,
                              running=(bn.running_mean, bn.running_var),
                              momentum=0.0 if bn.momentum is None else bn.momentum)
    from . import engine as _engine
    _engine.bump_bn_counter(bn)
    return out


class _BatchNormTrainFn(torch.autograd.Function):
    """nn.BatchNorm2d in train mode [+ residual add] [+ ReLU], forward and backward on the norm kernels."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, relu, eps, momentum, running_mean, running_var):
        xn = x.permute(0, 2, 3, 1)
        rn = None if residual is None else residual.permute(0, 2, 3, 1)
        out, mean, rstd = _norm_forward(xn, 1, gamma.detach(), beta.detach(), eps, relu, rn,
                                        running=(running_mean, running_var), momentum=momentum)
        ctx.save_for_backward(x, gamma, mean, rstd, out if relu else None)
        ctx.relu = relu
        ctx.has_res = residual is not None
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.load()
        x, gamma, mean, rstd, out = ctx.saved_tensors
        gy = gy.to(torch.bfloat16)
        if gy.stride(1) != 1:
            gy = gy.contiguous(memory_format=torch.channels_last)
        xn, gn = x.permute(0, 2, 3, 1), gy.permute(0, 2, 3, 1)
        B, H, W, C, xps = _nhwc_geom(xn)
        _, _, _, _, gps = _nhwc_geom(gn)
        dx = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=x.device)
        dres = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=x.device) if (ctx.has_res and ctx.relu) else None
        # d(beta), d(gamma) as two separate allocations: AccumulateGrad steals a whole tensor but has to COPY a view (one tiny
        # copy kernel per BatchNorm parameter and step otherwise)
        dgb = (torch.empty(C, dtype=torch.float32, device=x.device), torch.empty(C, dtype=torch.float32, device=x.device))
        g32 = gamma.detach().float().contiguous()
        ws, wsn = _norm_partials(1, B * H * W, C, x.device, backward=True)
        _lib.check(lib.oess_batchnorm_bwd_nhwc_bf16(_ptr(xn), xps, _ptr(gn), gps, None if out is None else _ptr(out), C, _ptr(mean),
                                                    _ptr(rstd), _ptr(g32), int(ctx.relu), B * H * W, C, _ptr(dgb[0]), _ptr(dgb[1]),
                                                    _ptr(dx), C, None if dres is None else _ptr(dres), C, _ptr(ws), wsn, _stream()),
                   "oess_batchnorm_bwd_nhwc_bf16")
        gres = None
        if ctx.has_res:
            gres = dres.permute(0, 3, 1, 2) if dres is not None else gy       # no ReLU: the residual sees dy itself
        return dx.permute(0, 3, 1, 2), dgb[1].to(gamma.dtype), dgb[0].to(gamma.dtype), gres, None, None, None, None, None


def batch_norm_train(x, bn, relu=False, residual=None):
    """Differentiable nn.BatchNorm2d (train mode: batch statistics + running-stat update) [+ residual] [+ ReLU] on a
    logical-NCHW channels_last bf16 tensor (models/_resnet.py:96-114, models/deeplabv3.py:295-348)."""
    _need_gpu(x)
    if x.dtype != torch.bfloat16 or x.stride(1) != 1:
        x = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    if residual is not None and (residual.dtype != torch.bfloat16 or residual.stride(1) != 1):
        residual = residual.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    y = _BatchNormTrainFn.apply(x, bn.weight, bn.bias, residual, bool(relu), float(bn.eps),
                                0.0 if bn.momentum is None else float(bn.momentum), bn.running_mean, bn.running_var)
    from . import engine as _engine
    _engine.bump_bn_counter(bn)
    return y


class _InstanceNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, relu, residual, eps):
        xn = x.permute(0, 2, 3, 1)
        rn = None if residual is None else residual.permute(0, 2, 3, 1)
        out, mean, rstd = _norm_forward(xn, x.shape[0], None, None, eps, relu, rn)
        ctx.save_for_backward(x, mean, rstd)
        ctx.relu = relu
        ctx.has_res = residual is not None
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.load()
        x, mean, rstd = ctx.saved_tensors
        gy = gy.to(torch.bfloat16)
        if gy.stride(1) != 1:
            gy = gy.contiguous(memory_format=torch.channels_last)
        xn, gn = x.permute(0, 2, 3, 1), gy.permute(0, 2, 3, 1)
        B, H, W, C, xps = _nhwc_geom(xn)
        _, _, _, _, gps = _nhwc_geom(gn)
        dx = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=x.device)
        s = torch.empty((2, B, C), dtype=torch.float32, device=x.device)
        ws, wsn = _norm_partials(B, H * W, C, x.device, backward=True)
        _lib.check(lib.oess_instnorm_bwd_nhwc_bf16(_ptr(xn), xps, _ptr(gn), gps, _ptr(mean), _ptr(rstd), int(ctx.relu), B, H * W,
                                                   C, _ptr(s[0]), _ptr(s[1]), _ptr(dx), C, _ptr(ws), wsn, _stream()),
                   "oess_instnorm_bwd_nhwc_bf16")
        return dx.permute(0, 3, 1, 2), None, (gy if ctx.has_res else None), None


def instance_norm(x, relu=False, residual=None, eps=1e-5):
    """nn.InstanceNorm2d(affine=False) [+ residual add] [+ ReLU] on a logical-NCHW channels_last bf16 tensor."""
    _need_gpu(x)
    if relu and residual is not None:
        raise NotImplementedError("ReLU after the residual add is not a pattern of the reference (the backward mask "
                                  "would depend on the residual)")
    if x.dtype != torch.bfloat16 or x.stride(1) != 1:
        x = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    if residual is not None and (residual.dtype != torch.bfloat16 or residual.stride(1) != 1):
        residual = residual.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    return _InstanceNormFn.apply(x, bool(relu), residual, float(eps))


class _UpsampleConcatFn(torch.autograd.Function):
    """cat([F.interpolate(x, scale_factor=2, mode='nearest'), skip], 1) written straight into one NHWC buffer."""

    @staticmethod
    def forward(ctx, x, skip):
        lib = _lib.load()
        xn = x.permute(0, 2, 3, 1)
        B, H, W, C, ps = _nhwc_geom(xn)
        Cs = 0 if skip is None else skip.shape[1]
        buf = torch.empty((B, 2 * H, 2 * W, C + Cs), dtype=torch.bfloat16, device=x.device)
        _lib.check(lib.oess_upsample_nearest2x_nhwc_bf16(_ptr(xn), ps, B, H, W, C, _ptr(buf), C + Cs, _stream()),
                   "oess_upsample_nearest2x_nhwc_bf16")
        if skip is not None:
            buf[..., C:] = skip.permute(0, 2, 3, 1)
        ctx.meta = (B, H, W, C, Cs)
        return buf.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        B, H, W, C, Cs = ctx.meta
        g = g.to(torch.bfloat16)
        if g.stride(1) != 1:
            g = g.contiguous(memory_format=torch.channels_last)
        gn = g.permute(0, 2, 3, 1)
        _, _, _, _, gps = _nhwc_geom(gn)
        gx = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=g.device)
        _lib.check(lib.oess_downsample_sum2x_nhwc_bf16(_ptr(gn), gps, B, H, W, C, _ptr(gx), C, _stream()),
                   "oess_downsample_sum2x_nhwc_bf16")
        gskip = None
        if Cs and ctx.needs_input_grad[1]:
            gskip = g[:, C:]
        return gx.permute(0, 3, 1, 2), gskip


def upsample2x_concat(x, skip=None):
    _need_gpu(x)
    if x.dtype != torch.bfloat16 or x.stride(1) != 1:
        x = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    return _UpsampleConcatFn.apply(x, skip)


def zero_insert(x_nhwc, stride, Hz, Wz):
    """z[:, ::stride, ::stride] = x on a zero Hz x Wz grid (NHWC bf16 views): the dilate step of a strided conv's dgrad."""
    lib = _lib.load()
    _need_gpu(x_nhwc)
    B, H, W, C, ps = _nhwc_geom(x_nhwc)
    out = torch.empty((B, Hz, Wz, C), dtype=torch.bfloat16, device=x_nhwc.device)
    _lib.check(lib.oess_zero_insert_nhwc_bf16(_ptr(x_nhwc), ps, B, H, W, C, stride, Hz, Wz, _ptr(out), C, _stream()),
               "oess_zero_insert_nhwc_bf16")
    return out


def upsample2x_sum_nhwc(x_nhwc, skip_nhwc=None, out=None):
    """bf16(bilinear2x(f32(x) + f32(skip))) on NHWC bf16 views, bilinear2x = F.interpolate(scale_factor=2, mode='bilinear',
    align_corners=False): the skip sum and the upsampling of an E2VID UpsampleConvLayer in one pass, fp32 inside, rounded once
    (K30).  skip_nhwc None: no sum.  out: optional [B, 2H, 2W, C] bf16 NHWC view (a channel slice of a wider buffer is fine) that
    shares no memory with an input.  Returns [B, 2H, 2W, C] bf16."""
    lib = _lib.load()
    _need_gpu(x_nhwc, skip_nhwc, out)
    B, H, W, C, ps = _nhwc_geom(x_nhwc)
    if C % 8:
        raise ValueError(f"upsample2x_sum_nhwc needs a channel count that is a multiple of 8, got {C}")
    sps = 0
    if skip_nhwc is not None:
        if tuple(skip_nhwc.shape) != (B, H, W, C):
            raise ValueError(f"skip has shape {tuple(skip_nhwc.shape)}, x has {(B, H, W, C)}")
        sps = _nhwc_geom(skip_nhwc)[4]
    if out is None:
        out = torch.empty((B, 2 * H, 2 * W, C), dtype=torch.bfloat16, device=x_nhwc.device)
    elif out.dtype != torch.bfloat16 or tuple(out.shape) != (B, 2 * H, 2 * W, C):
        raise ValueError(f"out must be bf16 {(B, 2 * H, 2 * W, C)}, got {out.dtype} {tuple(out.shape)}")
    ops = _nhwc_geom(out)[4]
    _lib.check(lib.oess_upsample_bilinear2x_sum_nhwc_bf16(_ptr(x_nhwc), ps, _ptr(skip_nhwc), sps, B, H, W, C, _ptr(out), ops, _stream()),
               "oess_upsample_bilinear2x_sum_nhwc_bf16")
    return out


def bilinear_l2norm(x, scale=4, normalize=True):
    """nn.Upsample(scale, bilinear, align_corners=True) + F.normalize(dim=1), inference form (no autograd)."""
    lib = _lib.load()
    _need_gpu(x)
    xn = x.permute(0, 2, 3, 1)
    B, H, W, C, ps = _nhwc_geom(xn)
    out = torch.empty((B, H * scale, W * scale, C), dtype=torch.bfloat16, device=x.device)
    _lib.check(lib.oess_bilinear_l2norm_nhwc_bf16(_ptr(xn), ps, B, H, W, C, scale, int(normalize), _ptr(out), C, None, _stream()),
               "oess_bilinear_l2norm_nhwc_bf16")
    return out.permute(0, 3, 1, 2)


class _BilinearL2NormTrain(torch.autograd.Function):
    """Differentiable nn.Upsample(scale, bilinear, align_corners=True) + F.normalize(dim=1) as ONE node: the forward is the fused
    inference kernel (which also leaves 1 / |x| per output pixel), so the un-normalised full-resolution tensor -- 1.15 GB at the
    BASELINE size -- is never written or re-read; the backward is the L2 adjoint on (y, g, 1 / |x|) followed by the
    deterministic two-pass bilinear adjoint."""

    @staticmethod
    def forward(ctx, x, scale):
        lib = _lib.load()
        xn = x.permute(0, 2, 3, 1)
        B, H, W, C, ps = _nhwc_geom(xn)
        y = torch.empty((B, H * scale, W * scale, C), dtype=torch.bfloat16, device=x.device)
        inv = torch.empty(B * H * scale * W * scale, dtype=torch.float32, device=x.device)
        _lib.check(lib.oess_bilinear_l2norm_nhwc_bf16(_ptr(xn), ps, B, H, W, C, scale, 1, _ptr(y), C, _ptr(inv), _stream()),
                   "oess_bilinear_l2norm_nhwc_bf16")
        ctx.save_for_backward(y, inv)
        ctx.meta = (B, H, W, C, scale)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        y, inv = ctx.saved_tensors
        B, H, W, C, scale = ctx.meta
        Ho, Wo = H * scale, W * scale
        gn = _nhwc_any(g.to(torch.bfloat16))
        gup = torch.empty_like(y)
        _lib.check(lib.oess_l2norm_nhwc_bwd(_ptr(y), C, _ptr(gn), _pix_stride(gn), _ptr(inv), B * Ho * Wo, C, 1, 1e-12, _ptr(gup), C,
                                            _stream()), "oess_l2norm_nhwc_bwd")
        gin = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=g.device)
        nbytes = lib.oess_resize_bilinear_bwd_workspace_bytes(B, W, C, Ho)
        ws = _workspace(nbytes, g.device, tag="resize")
        _lib.check(lib.oess_resize_bilinear_nhwc_bwd(_ptr(gup), C, B, H, W, C, 1, Ho, Wo, 1, _ptr(ws), ws.numel(), _ptr(gin), C, _stream()),
                   "oess_resize_bilinear_nhwc_bwd")
        return gin.permute(0, 3, 1, 2), None


class _BilinearL2NormPool(torch.autograd.Function):
    """k = scatter_mean(F.normalize(nn.Upsample(scale, bilinear, align_corners=True)(x)), superpixels) as ONE node: forward = the
    fused upsample + normalise kernel followed by K7 on its output; backward = ONE pass over the saved normalised map that gathers
    gk / (n + 1e-6) rows from the S x C table, forms the L2 adjoint on the fly and does the x pass of the bilinear adjoint,
    then the y pass -- instead of row gather -> L2 adjoint -> bilinear adjoint through three 1.15 GB tensors."""

    @staticmethod
    def forward(ctx, x, scale, ids, sps, S):
        lib = _lib.load()
        xn = x.permute(0, 2, 3, 1)
        B, H, W, C, ps = _nhwc_geom(xn)
        Ho, Wo = H * scale, W * scale
        y = torch.empty((B, Ho, Wo, C), dtype=torch.bfloat16, device=x.device)
        inv = torch.empty(B * Ho * Wo, dtype=torch.float32, device=x.device)
        _lib.check(lib.oess_bilinear_l2norm_nhwc_bf16(_ptr(xn), ps, B, H, W, C, scale, 1, _ptr(y), C, _ptr(inv), _stream()),
                   "oess_bilinear_l2norm_nhwc_bf16")
        k = torch.empty((S, C), dtype=torch.float32, device=x.device)
        cnt = torch.empty((S,), dtype=torch.float32, device=x.device)
        ws_bytes = lib.oess_segment_mean_fwd_workspace_bytes(S, C)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        _lib.check(lib.oess_segment_mean_fwd(_ptr(y), 1, _ptr(ids), B * Ho * Wo, Ho * Wo, sps, C, S, _ptr(k), _ptr(cnt), _ptr(ws), ws_bytes,
                                             _stream()), "oess_segment_mean_fwd")
        ctx.save_for_backward(y, inv, ids, cnt)
        ctx.meta = (B, H, W, C, scale, sps, S)
        return k

    @staticmethod
    def backward(ctx, gk):
        lib = _lib.load()
        y, inv, ids, cnt = ctx.saved_tensors
        B, H, W, C, scale, sps, S = ctx.meta
        Ho, Wo = H * scale, W * scale
        gk = gk.contiguous().float()
        gin = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=gk.device)
        nbytes = lib.oess_bilinear_l2norm_pool_bwd_workspace_bytes(B, W, C, Ho, S)
        ws = _workspace(nbytes, gk.device, tag="resize")
        _lib.check(lib.oess_bilinear_l2norm_pool_bwd_bf16(_ptr(y), C, _ptr(inv), _ptr(ids), _ptr(gk), _ptr(cnt), sps, S, B, H, W, C, Ho, Wo, 1,
                                                          1e-12, _ptr(ws), ws.numel(), _ptr(gin), C, _stream()),
                   "oess_bilinear_l2norm_pool_bwd_bf16")
        return gin.permute(0, 3, 1, 2), None, None, None, None


HEADPOOL_F32_CHANNELS = (64, 128, 256)


class _BilinearL2NormPoolF32(torch.autograd.Function):
    """The same node in fp32 (K20) with NO full-resolution tensor in either direction: forward and backward recompute every
    output pixel's four-corner blend from x (oess_bilinear_l2norm_pool_fwd_f32 / _bwd_f32).  Saves x, ids and count only."""

    @staticmethod
    def forward(ctx, x, scale, ids, sps, S):
        if x.dtype != torch.float32 or x.ndim != 4 or x.shape[1] not in HEADPOOL_F32_CHANNELS:
            raise ValueError(f"the fp32 head-pool node takes a float32 [B, C, H, W] map with C in {HEADPOOL_F32_CHANNELS}, not "
                             f"{x.dtype} {tuple(x.shape)}")
        lib = _lib.load()
        xn = _nhwc_any(x)
        B, H, W, C = xn.shape
        k = torch.empty((S, C), dtype=torch.float32, device=x.device)
        cnt = torch.empty((S,), dtype=torch.float32, device=x.device)
        ws_bytes = lib.oess_segment_mean_fwd_workspace_bytes(S, C)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        _lib.check(lib.oess_bilinear_l2norm_pool_fwd_f32(_ptr(xn), _pix_stride(xn), _ptr(ids), sps, S, B, H, W, C, scale, 1, 1e-12, _ptr(k),
                                                         _ptr(cnt), _ptr(ws), ws_bytes, _stream()), "oess_bilinear_l2norm_pool_fwd_f32")
        ctx.save_for_backward(xn, ids, cnt)
        ctx.meta = (B, H, W, C, scale, sps, S)
        ctx.mark_non_differentiable(cnt)
        return k, cnt

    @staticmethod
    def backward(ctx, gk, _gcnt):
        lib = _lib.load()
        xn, ids, cnt = ctx.saved_tensors
        B, H, W, C, scale, sps, S = ctx.meta
        gk = gk.contiguous().float()
        gin = torch.empty((B, H, W, C), dtype=torch.float32, device=gk.device)
        nbytes = lib.oess_bilinear_l2norm_pool_bwd_workspace_bytes(B, W, C, H * scale, S)
        ws = _workspace(nbytes, gk.device, tag="resize")
        _lib.check(lib.oess_bilinear_l2norm_pool_bwd_f32(_ptr(xn), _pix_stride(xn), _ptr(ids), _ptr(gk), _ptr(cnt), sps, S, B, H, W, C, scale, 1,
                                                         1e-12, _ptr(ws), ws.numel(), _ptr(gin), C, _stream()),
                   "oess_bilinear_l2norm_pool_bwd_f32")
        return gin.permute(0, 3, 1, 2), None, None, None, None


class UpsampledNormalizedFeature:
    """DilationFeatureExtractor's output  F.normalize(nn.Upsample(x4, bilinear, align_corners=True)(x))  (models/image_model.py:
    121-143) kept as (x, scale) for a consumer that only pools it over superpixels (training/pretrain_trainer.py:445-465):
    `pool` is the one-node form above; `materialize()` is the full-resolution tensor for anything else.  bf16 x: the bf16 nodes;
    fp32 x (C in HEADPOOL_F32_CHANNELS): the fp32 node / the composed fp32 chain.  Anything else raises before any launch."""

    def __init__(self, x, scale):
        if x.dtype == torch.float32:
            if x.ndim != 4 or x.shape[1] not in HEADPOOL_F32_CHANNELS:
                raise ValueError(f"the fp32 head-pool node runs C in {HEADPOOL_F32_CHANNELS}, not a map of shape {tuple(x.shape)}")
        elif x.dtype != torch.bfloat16:
            raise ValueError(f"UpsampledNormalizedFeature holds a bfloat16 or float32 map, not {x.dtype}")
        if int(scale) != scale or int(scale) < 1:
            raise ValueError("integer scale factors >= 1 only")
        self.x, self.scale = x, int(scale)

    @property
    def shape(self):
        B, C, H, W = self.x.shape
        return torch.Size((B, C, H * self.scale, W * self.scale))

    def materialize(self):
        if self.x.dtype == torch.float32:
            return l2_normalize(bilinear_resize(self.x, scale_factor=self.scale, align_corners=True))
        return bilinear_l2norm_train(self.x, self.scale)

    def pool(self, superpixels, superpixel_size, S=None, with_count=False):
        B, C, Ho, Wo = self.shape
        _need_gpu(self.x, superpixels)
        if tuple(superpixels.shape) != (B, Ho, Wo):
            raise ValueError("superpixel map does not match the upsampled feature size")
        if S is None:
            off = torch.arange(0, B * superpixel_size, superpixel_size, device=superpixels.device)[:, None, None]
            S = int((superpixels + off).max().item()) + 1
        ids = superpixels.reshape(-1).contiguous().to(torch.int64)
        if self.x.dtype == torch.float32:
            k, cnt = _BilinearL2NormPoolF32.apply(self.x, self.scale, ids, int(superpixel_size), int(S))
            return (k, cnt) if with_count else k
        if with_count:
            raise ValueError("with_count is a form of the fp32 node")
        return _BilinearL2NormPool.apply(self.x, self.scale, ids, int(superpixel_size), int(S))


class _PoolMatrixMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, matrix, S):
        lib = _lib.load()
        yn = _nhwc_any(y)
        B, h, w, C = yn.shape
        k = torch.empty((S, C), dtype=torch.float32, device=y.device)
        cnt = torch.empty((S,), dtype=torch.float32, device=y.device)
        _lib.check(lib.oess_pool_matrix_fwd(_ptr(matrix), _ptr(yn), _pix_stride(yn), int(yn.dtype == torch.bfloat16), B, h, w, C, S,
                                            _ptr(k), _ptr(cnt), _stream()), "oess_pool_matrix_fwd")
        ctx.save_for_backward(matrix)
        ctx.meta = (B, h, w, C, S, yn.dtype)
        return k

    @staticmethod
    def backward(ctx, gk):
        lib = _lib.load()
        (matrix,) = ctx.saved_tensors
        B, h, w, C, S, dtype = ctx.meta
        gk = gk.contiguous().float()
        gy = torch.empty((B, h, w, C), dtype=dtype, device=gk.device)
        _lib.check(lib.oess_pool_matrix_bwd(_ptr(matrix), _ptr(gk), B, h, w, C, S, _ptr(gy), C, int(dtype == torch.bfloat16), _stream()),
                   "oess_pool_matrix_bwd")
        return gy.permute(0, 3, 1, 2), None, None


POOL_MATRIX_MAX_BYTES = 256 << 20       # B = 8 at OS16: 18-26 MB; B = 32 at OS8 would be ~1 GB (see pool_matrix)


def pool_matrix(superpixels, in_hw, superpixel_size, S, align_corners=False):
    """Pooling matrix of (bilinear upsample from in_hw to the size of `superpixels`) followed by the superpixel scatter-mean:
    an opaque device buffer for UpsampledFeature.pool / _PoolMatrixMean (2^-40 fixed-point weight sums + pixel counts)."""
    lib = _lib.load()
    _need_gpu(superpixels)
    B, Ho, Wo = superpixels.shape
    h, w = int(in_hw[0]), int(in_hw[1])
    ids = superpixels.reshape(-1).contiguous().to(torch.int64)
    nbytes = lib.oess_pool_matrix_bytes(int(S), B, h, w)
    if nbytes > POOL_MATRIX_MAX_BYTES:
        # the matrix is dense S x (B h w) and both S and the column count grow with B: O(B^2) memset + scan per step.  Above the
        # cap the caller pools the materialised tensor instead (UpsampledFeature.pool does that on a None matrix).
        return None
    m = torch.empty(nbytes, dtype=torch.uint8, device=superpixels.device)
    _lib.check(lib.oess_pool_matrix_build(_ptr(ids), B, Ho, Wo, h, w, int(bool(align_corners)), int(superpixel_size), int(S), _ptr(m), nbytes,
                                          _stream()), "oess_pool_matrix_build")
    return m


class UpsampledFeature:
    """DeepLabv3's `feats = F.interpolate(feats, size=input_shape, mode='bilinear', align_corners=False)` (models/deeplabv3.py:184)
    kept as (low-resolution map, size) for a consumer that only pools it over superpixels (training/pretrain_trainer.py:445-465,
    frame2recon): upsampling and pooling are both linear, so `pool` multiplies the low-resolution map with the pooling matrix of
    the superpixel map (pool_matrix) -- forward and backward without any full-resolution tensor.  `materialize()` is the tensor."""

    def __init__(self, x, size, align_corners=False):
        self.x, self.size, self.align_corners = x, (int(size[0]), int(size[1])), bool(align_corners)

    @property
    def shape(self):
        B, C = self.x.shape[:2]
        return torch.Size((B, C, self.size[0], self.size[1]))

    def materialize(self):
        return bilinear_resize(self.x, size=self.size, align_corners=self.align_corners)

    def pool(self, superpixels, superpixel_size, S=None, matrix=None):
        B, C, Ho, Wo = self.shape
        _need_gpu(self.x, superpixels)
        if tuple(superpixels.shape) != (B, Ho, Wo):
            raise ValueError("superpixel map does not match the upsampled feature size")
        if S is None:
            off = torch.arange(0, B * superpixel_size, superpixel_size, device=superpixels.device)[:, None, None]
            S = int((superpixels + off).max().item()) + 1
        if matrix is None:
            matrix = pool_matrix(superpixels, self.x.shape[2:], superpixel_size, S, self.align_corners)
        if matrix is None:              # above POOL_MATRIX_MAX_BYTES: the reference's own order, upsample then scatter-mean (K7)
            return superpixel_pool(self.materialize(), superpixels, superpixel_size, S=S)
        return _PoolMatrixMean.apply(self.x, matrix, int(S))


class _UpsampledL1Mean(torch.autograd.Function):
    """mean |up(a - b)| of two fp32 low-resolution maps as ONE node: saves the two maps, forms no
    full-resolution tensor in forward or backward."""

    @staticmethod
    def forward(ctx, a, b, Ho, Wo, align):
        lib = _lib.load()
        an, bn = _nhwc_any(a), _nhwc_any(b)
        B, h, w, C = an.shape
        nbytes = lib.oess_upsampled_l1_workspace_bytes(B, h, w, C, Ho, Wo)
        ws = _workspace(nbytes, a.device, tag="upsampled_l1")
        loss = torch.empty(1, dtype=torch.float32, device=a.device)
        _lib.check(lib.oess_upsampled_l1_fwd_f32(_ptr(an), _pix_stride(an), _ptr(bn), _pix_stride(bn), B, h, w, C, Ho, Wo, align,
                                                 _ptr(ws), ws.numel(), _ptr(loss), _stream()), "oess_upsampled_l1_fwd_f32")
        ctx.save_for_backward(an, bn)
        ctx.meta = (Ho, Wo, align)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        an, bn = ctx.saved_tensors
        (B, h, w, C), (Ho, Wo, align) = an.shape, ctx.meta
        ga = torch.empty((B, h, w, C), dtype=torch.float32, device=an.device) if ctx.needs_input_grad[0] else None
        gb = torch.empty((B, h, w, C), dtype=torch.float32, device=an.device) if ctx.needs_input_grad[1] else None
        if ga is None and gb is None:
            return None, None, None, None, None
        gdev = g.reshape(1).float().contiguous()
        _lib.check(lib.oess_upsampled_l1_bwd_f32(_ptr(an), _pix_stride(an), _ptr(bn), _pix_stride(bn), B, h, w, C, Ho, Wo, align,
                                                 _ptr(gdev), _ptr(ga), C, _ptr(gb), C, _stream()), "oess_upsampled_l1_bwd_f32")
        return (None if ga is None else ga.permute(0, 3, 1, 2)), (None if gb is None else gb.permute(0, 3, 1, 2)), None, None, None


def upsampled_l1_supported(C, in_hw, size):
    """Geometry of the fused fp32 node's entries (include/oess.h, oess_upsampled_l1_*)."""
    return C % 4 == 0 and C <= 1024 and size[0] >= in_hw[0] and size[1] >= in_hw[1]


def upsampled_l1_mean(a, b):
    """nn.L1Loss()(a, b) (training/openess_trainer.py:497) of two UpsampledFeature operands of equal geometry with fp32 maps, as
    one autograd node on the low-resolution maps: |up(a) - up(b)| = |up(a - b)| is recomputed element by element in forward and
    backward, nothing of the full-resolution size is allocated (l1_mean on the same operands writes the upsampled difference
    and its gradient: 2.3 GB each at 8 x 256 x 440 x 640).  Geometry the entries refuse goes through l1_mean."""
    if not (isinstance(a, UpsampledFeature) and isinstance(b, UpsampledFeature)):
        raise TypeError("upsampled_l1_mean takes two hip.UpsampledFeature")
    if a.size != b.size or a.align_corners != b.align_corners or a.x.shape != b.x.shape:
        raise ValueError("upsampled_l1_mean: operands differ in geometry")
    _need_gpu(a.x, b.x)
    if a.x.dtype != torch.float32 or b.x.dtype != torch.float32 or a.x.ndim != 4:
        raise ValueError("upsampled_l1_mean: the low-resolution maps must be 4-D float32")
    if not upsampled_l1_supported(a.x.shape[1], a.x.shape[2:], a.size):
        return l1_mean(a, b)
    return _UpsampledL1Mean.apply(a.x, b.x, a.size[0], a.size[1], int(a.align_corners))


class _UpsampledCosine(torch.autograd.Function):
    """mean(1 - cos(up(a), resize(t)[:Ho, :Wo])) of a low-resolution student map and an fp32 teacher map as ONE node (DESIGN.md
    K34): saves the two small maps and two fp32 scalars per output pixel, forms no full-resolution tensor in forward or backward.
    The teacher is data: no gradient."""

    @staticmethod
    def forward(ctx, a, t, Ho, Wo, align, Mh, Mw, eps):
        lib = _lib.load()
        an, tn = _nhwc_any(a), _nhwc_any(t)
        (B, h, w, C), (ht, wt) = an.shape, tn.shape[1:3]
        ws = _workspace(lib.oess_upsampled_cosine_workspace_bytes(B, h, w, C, Ho, Wo), a.device, tag="upsampled_cosine")
        planes = None
        if ctx.needs_input_grad[0]:
            planes = torch.empty(lib.oess_upsampled_cosine_planes_floats(B, Ho, Wo), dtype=torch.float32, device=a.device)
        loss = torch.empty(1, dtype=torch.float32, device=a.device)
        _lib.check(lib.oess_upsampled_cosine_fwd(_ptr(an), int(an.dtype == torch.bfloat16), _pix_stride(an), _ptr(tn), _pix_stride(tn),
                                                 B, h, w, C, Ho, Wo, align, ht, wt, Mh, Mw, eps, _ptr(ws), ws.numel(), _ptr(planes),
                                                 _ptr(loss), _stream()), "oess_upsampled_cosine_fwd")
        if planes is not None:
            ctx.save_for_backward(an, tn, planes)
        ctx.meta = (Ho, Wo, align, Mh, Mw)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return (None,) * 8
        lib = _lib.load()
        an, tn, planes = ctx.saved_tensors
        (B, h, w, C), (ht, wt), (Ho, Wo, align, Mh, Mw) = an.shape, tn.shape[1:3], ctx.meta
        ga = torch.empty((B, h, w, C), dtype=an.dtype, device=an.device)
        gdev = g.reshape(1).float().contiguous()
        _lib.check(lib.oess_upsampled_cosine_bwd(_ptr(an), int(an.dtype == torch.bfloat16), _pix_stride(an), _ptr(tn), _pix_stride(tn),
                                                 B, h, w, C, Ho, Wo, align, ht, wt, Mh, Mw, _ptr(planes), _ptr(gdev), _ptr(ga), C,
                                                 _stream()), "oess_upsampled_cosine_bwd")
        return (ga.permute(0, 3, 1, 2),) + (None,) * 7


def sam_distill_supported(C, in_hw, size):
    """Geometry of the fused node's entries (include/oess.h, oess_upsampled_cosine_*); the teacher side takes any map."""
    return C % 4 == 0 and C <= 1024 and size[0] >= in_hw[0] and size[1] >= in_hw[1]


def sam_distill_loss(sam, feat, eps=1e-8):
    """The SAM distillation loss of the frame2recon pre-training step (training/pretrain_trainer.py:519-529):
        M = max(H, W);  sam_up = F.interpolate(sam, size=(M, M), mode='bilinear', align_corners=False)[:, :, :H, :]
        loss = mean(1 - F.cosine_similarity(sam_up, feat, dim=1))
    sam: [B, C, hs, ws] fp32 (data, no gradient is returned for it).  feat: [B, C, H, W] fp32 / bf16, a tensor or a
    hip.UpsampledFeature.  H > W is refused: the reference crops rows only, so its cosine_similarity cannot broadcast there.
    An UpsampledFeature whose map the entries accept runs one fused node on the two small maps (nothing of the
    full-resolution size is allocated, forward or backward).  A plain tensor, or geometry the entries refuse, goes through
    bilinear_resize, the crop and cosine_mean_loss in the reference's order, in fp32 as the reference computes it."""
    lazy = isinstance(feat, UpsampledFeature)
    fx = feat.x if lazy else feat
    if not torch.is_tensor(sam) or not torch.is_tensor(fx) or not sam.is_cuda or not fx.is_cuda:
        raise ValueError("sam_distill_loss needs CUDA/HIP tensors (no CPU fallback)")
    if sam.ndim != 4 or fx.ndim != 4 or sam.dtype != torch.float32 or fx.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("sam_distill_loss: sam must be 4-D float32 and feat 4-D float32 / bfloat16")
    if sam.shape[:2] != fx.shape[:2]:
        raise ValueError(f"sam_distill_loss: batch / channel counts differ: sam {tuple(sam.shape)}, feat {tuple(feat.shape)}")
    H, W = int(feat.shape[2]), int(feat.shape[3])
    if H > W:
        raise ValueError(f"sam_distill_loss: H = {H} > W = {W}: the reference crops the rows of the (M, M) map only")
    M = max(H, W)
    sam = sam.detach()
    if lazy and sam_distill_supported(fx.shape[1], fx.shape[2:], feat.size):
        return _UpsampledCosine.apply(fx, sam, H, W, int(feat.align_corners), M, M, float(eps))
    full = bilinear_resize(fx.float(), size=feat.size, align_corners=feat.align_corners) if lazy else feat.float()
    sam_up = bilinear_resize(sam, size=(M, M), align_corners=False)[:, :, :H, :]
    return cosine_mean_loss(sam_up, full, eps)


def bilinear_l2norm_train(x, scale=4):
    """Differentiable form of bilinear_l2norm (normalisation on) for a channels_last bf16 tensor with C % 64 == 0."""
    _need_gpu(x)
    if x.dtype != torch.bfloat16 or x.shape[1] % 64 or x.shape[1] > 512:
        raise ValueError("bilinear_l2norm_train needs bf16 with C % 64 == 0, C <= 512")
    return _BilinearL2NormTrain.apply(x, int(scale))


def _nhwc_any(x):
    """Logical NCHW fp32/bf16 tensor -> NHWC view with dense channels and uniformly strided pixels (copy if needed)."""
    if x.dtype not in (torch.float32, torch.bfloat16) or x.ndim != 4:
        raise ValueError("expected a 4-D float32 / bfloat16 tensor")
    xn = x.permute(0, 2, 3, 1)
    if xn.stride(3) != 1 or not _uniform_pix_stride(xn):
        xn = xn.contiguous()
    return xn


class _BilinearResize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Ho, Wo, align):
        lib = _lib.load()
        xn = _nhwc_any(x)
        B, H, W, C = xn.shape
        out = torch.empty((B, Ho, Wo, C), dtype=x.dtype, device=x.device)
        _lib.check(lib.oess_resize_bilinear_nhwc_fwd(_ptr(xn), _pix_stride(xn), B, H, W, C, int(x.dtype == torch.bfloat16), Ho, Wo,
                                                     int(align), _ptr(out), C, _stream()), "oess_resize_bilinear_nhwc_fwd")
        ctx.meta = (B, H, W, C, Ho, Wo, int(align))
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        B, H, W, C, Ho, Wo, align = ctx.meta
        gn = _nhwc_any(g)
        gin = torch.empty((B, H, W, C), dtype=g.dtype, device=g.device)
        nbytes = lib.oess_resize_bilinear_bwd_workspace_bytes(B, W, C, Ho)
        ws = _workspace(nbytes, g.device, tag="resize")
        _lib.check(lib.oess_resize_bilinear_nhwc_bwd(_ptr(gn), _pix_stride(gn), B, H, W, C, int(g.dtype == torch.bfloat16), Ho, Wo,
                                                     align, _ptr(ws), ws.numel(), _ptr(gin), C, _stream()),
                   "oess_resize_bilinear_nhwc_bwd")
        return gin.permute(0, 3, 1, 2), None, None, None


def bilinear_resize(x, size=None, scale_factor=None, align_corners=False):
    """F.interpolate(x, size | scale_factor, mode='bilinear', align_corners) for logical B x C x H x W fp32 / bf16
    tensors, differentiable.  Result is logically NCHW, physically channels_last."""
    _need_gpu(x)
    if (size is None) == (scale_factor is None):
        raise ValueError("give exactly one of size / scale_factor")
    if size is None:
        if int(scale_factor) != scale_factor:
            raise ValueError("integer scale factors only (a fractional factor changes ATen's index rule)")
        size = (x.shape[2] * int(scale_factor), x.shape[3] * int(scale_factor))
    return _BilinearResize.apply(x, int(size[0]), int(size[1]), bool(align_corners))


def argmax_labels(logits, size=None, align_corners=False, out=None):
    """Class labels of logical B x K x h x w fp32 / bf16 logits: int64 [B, H, W], the integers of
    bilinear_resize(logits.float(), size, align_corners).argmax(1) without the full-resolution tensor.  size=None
    (or the input size) interpolates nothing: logits.argmax(1) on the raw values.  torch.argmax's tie / NaN rule.  No autograd."""
    if not torch.is_tensor(logits) or not logits.is_cuda:
        raise ValueError("argmax_labels needs a CUDA/HIP tensor (no CPU fallback)")
    if logits.dtype not in (torch.float32, torch.bfloat16) or logits.ndim != 4:
        raise ValueError("argmax_labels expects 4-D float32 / bfloat16 logits [B, K, h, w]")
    B, K, h, w = logits.shape
    if not 1 <= K <= 256:
        raise ValueError(f"argmax_labels handles 1 <= K <= 256 classes, got {K}")
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    if out is None:
        out = torch.empty((B, H, W), dtype=torch.int64, device=logits.device)
    elif (not torch.is_tensor(out) or tuple(out.shape) != (B, H, W) or out.dtype != torch.int64 or out.device != logits.device
          or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous int64 tensor of shape {(B, H, W)} on {logits.device}")
    xn = _nhwc_any(logits.detach())
    _lib.check(_lib.load().oess_argmax_labels(_ptr(xn), int(logits.dtype == torch.bfloat16), _pix_stride(xn), B, K, h, w, H, W,
                                              int(bool(align_corners)), _ptr(out), _stream()), "oess_argmax_labels")
    _bump(out)
    return out


SEGMENT_RENDER_OUTPUTS = ('labels', 'conf', 'rgb')


def _class_offsets(what, class_offsets, P, device):
    """(int32 [K + 1] on the device, K) of a list / tensor of offsets checked on the host: 0 first, strictly increasing, P last"""
    offs = class_offsets.tolist() if torch.is_tensor(class_offsets) else list(class_offsets)
    if (len(offs) < 2 or any(not isinstance(o, int) or isinstance(o, bool) for o in offs) or offs[0] != 0
            or any(b <= a for a, b in zip(offs, offs[1:])) or offs[-1] != P):
        raise ValueError(f"{what}: class_offsets must start at 0, increase strictly and end at the channel count {P}, got {offs!r}")
    K = len(offs) - 1
    if not 1 <= K <= 255:
        raise ValueError(f"{what} handles 1 <= K <= 255 classes, got {K}")
    return h2d_async(torch.tensor(offs, dtype=torch.int32), device), K


def _render_args(what, like, B, K, H, W, palette, background, alpha, min_conf, ignore_label, want):
    """The checks every render shares; returns (want, palette, background, alpha256, min_conf, ignore_label, outputs)."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or len(set(want)) != len(want) or any(name not in SEGMENT_RENDER_OUTPUTS for name in want):
        raise ValueError(f"want must name at least one of {SEGMENT_RENDER_OUTPUTS}, each once, got {want!r}")
    if H < 1 or W < 1:
        raise ValueError(f"size must be positive, got {(H, W)}")
    ignore_label = int(ignore_label)
    if not K <= ignore_label <= 255:
        raise ValueError(f"ignore_label must lie in K ... 255 (it is not a class), got {ignore_label} for K = {K}")
    min_conf = float(min_conf)
    if not min_conf >= 0.0:
        raise ValueError(f"min_conf must be a number >= 0, got {min_conf}")
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must lie in 0 ... 1, got {alpha}")
    if 'rgb' in want:
        if (not torch.is_tensor(palette) or palette.dtype != torch.uint8 or tuple(palette.shape) != (K, 3)
                or palette.device != like.device or not palette.is_contiguous()):
            raise ValueError(f"palette must be a contiguous uint8 tensor of shape {(K, 3)} on {like.device}")
        if background is not None and (not torch.is_tensor(background) or background.dtype != torch.uint8
                                       or tuple(background.shape) != (B, H, W) or background.device != like.device
                                       or not background.is_contiguous()):
            raise ValueError(f"background must be a contiguous uint8 tensor of shape {(B, H, W)} on {like.device}")
    else:
        palette = background = None
    out = {}
    if 'labels' in want:
        out['labels'] = torch.empty((B, H, W), dtype=torch.uint8, device=like.device)
    if 'conf' in want:
        out['conf'] = torch.empty((B, H, W), dtype=torch.float32, device=like.device)
    if 'rgb' in want:
        out['rgb'] = torch.empty((B, H, W, 3), dtype=torch.uint8, device=like.device)
    return palette, background, int(round(alpha * 256)), min_conf, ignore_label, out


def segment_render(logits, size=None, align_corners=False, palette=None, background=None, alpha=0.5, min_conf=0.0, ignore_label=255,
                   want=SEGMENT_RENDER_OUTPUTS, class_offsets=None):
    """Segmentation maps of logical B x K x h x w fp32 / bf16 logits at `size` (None: the input size) without the full-resolution
    logit tensor: a dict of the tensors named in `want`,
      'labels'  u8 [B, H, W]: argmax_labels' label, or ignore_label where the confidence is below min_conf,
      'conf'    fp32 [B, H, W]: the softmax probability of the winning class,
      'rgb'     u8 [B, H, W, 3]: palette[label] (palette: u8 [K, 3] on the device; black for ignore_label), blended over
                `background` (u8 [B, H, W]) with weight alpha, in integers: (a * c + (256 - a) * grey + 128) >> 8, a = round(256 alpha).
    class_offsets (K36): a list / tensor of K + 1 offsets (0 first, strictly increasing, the channel count P <= 1024 last): the
    logits are those of P NAMES, class k owns the channels class_offsets[k] ... class_offsets[k + 1] - 1 and its value is
    torch.amax over them; labels, conf and rgb are over the K class values.  Singleton groups give the bits of class_offsets=None.
    No autograd."""
    if not torch.is_tensor(logits) or not logits.is_cuda:
        raise ValueError("segment_render needs a CUDA/HIP tensor (no CPU fallback)")
    if logits.dtype not in (torch.float32, torch.bfloat16) or logits.ndim != 4:
        raise ValueError("segment_render expects 4-D float32 / bfloat16 logits [B, K, h, w]")
    B, P, h, w = logits.shape
    offs = None
    if class_offsets is None:
        K = P
        if not 1 <= K <= 255:
            raise ValueError(f"segment_render handles 1 <= K <= 255 classes, got {K}")
    else:
        if not 1 <= P <= 1024:
            raise ValueError(f"segment_render handles 1 <= P <= 1024 names, got {P}")
        offs, K = _class_offsets("segment_render", class_offsets, P, logits.device)
    if min(B, h, w) < 1:
        raise ValueError(f"segment_render needs a non-empty batch, got {tuple(logits.shape)}")
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    palette, background, alpha256, min_conf, ignore_label, out = _render_args("segment_render", logits, B, K, H, W, palette, background,
                                                                              alpha, min_conf, ignore_label, want)
    xn = _nhwc_any(logits.detach())
    if offs is None:
        _lib.check(_lib.load().oess_segment_render(_ptr(xn), int(logits.dtype == torch.bfloat16), _pix_stride(xn), B, K, h, w, H, W,
                                                   int(bool(align_corners)), _ptr(palette), _ptr(background), alpha256,
                                                   min_conf, ignore_label, _ptr(out.get('labels')), _ptr(out.get('conf')),
                                                   _ptr(out.get('rgb')), _stream()), "oess_segment_render")
    else:
        _lib.check(_lib.load().oess_segment_render_grouped(_ptr(xn), int(logits.dtype == torch.bfloat16), _pix_stride(xn), B, K, P, h, w,
                                                           H, W, int(bool(align_corners)), _ptr(offs), _ptr(palette),
                                                           _ptr(background), alpha256, min_conf, ignore_label,
                                                           _ptr(out.get('labels')), _ptr(out.get('conf')), _ptr(out.get('rgb')),
                                                           _stream()), "oess_segment_render_grouped")
    for t in out.values():
        _bump(t)
    return out


RENDER_MAX_VIEWS = 8                            # OESS_RENDER_MAX_VIEWS of include/oess.h


def ensemble_render(views, flips=None, size=None, align_corners=False, palette=None, background=None, alpha=0.5, min_conf=0.0,
                    ignore_label=255, want=SEGMENT_RENDER_OUTPUTS):
    """segment_render's outputs from the MEAN class probability of 1 ... 8 views (flip and multi-scale inference)
    without any full-resolution [B, K, H, W] tensor.  views: logical B x K x h_v x w_v fp32 / bf16 logits of one dtype, device, B
    and K, each of its own size; flips: one bool per view (None: none) -- a flipped view is the logits of the MIRRORED input and
    counts as resize(view).flip(-1).  size=None is view 0's size.  Per view the probabilities are softmax over segment_render's
    class values, the mean runs over the views in order, the label is argmax of the mean and 'conf' its value; min_conf,
    ignore_label, palette, background and alpha as segment_render.  One unflipped view IS segment_render.  No autograd."""
    views = list(views) if isinstance(views, (list, tuple)) else None
    if not views or len(views) > RENDER_MAX_VIEWS:
        raise ValueError(f"ensemble_render takes a list of 1 ... {RENDER_MAX_VIEWS} views, got "
                         f"{'no list' if views is None else len(views)}")
    flips = [False] * len(views) if flips is None else list(flips)
    if len(flips) != len(views) or any(f not in (False, True, 0, 1) for f in flips):
        raise ValueError(f"flips must hold one bool per view ({len(views)}), got {flips!r}")
    x0 = views[0]
    for x in views:
        if not torch.is_tensor(x) or x.dtype not in (torch.float32, torch.bfloat16) or x.ndim != 4:
            raise ValueError("ensemble_render expects 4-D float32 / bfloat16 logits [B, K, h, w]")
        if x.dtype != x0.dtype or x.device != x0.device or x.shape[:2] != x0.shape[:2]:
            raise ValueError("ensemble_render: every view must share view 0's dtype, device, B and K, got "
                             f"{[(str(v.dtype), str(v.device), tuple(v.shape)) for v in views if torch.is_tensor(v)]}")
    if not x0.is_cuda:
        raise ValueError("ensemble_render needs CUDA/HIP tensors (no CPU fallback)")
    B, K = x0.shape[:2]
    if not 1 <= K <= 255:
        raise ValueError(f"ensemble_render handles 1 <= K <= 255 classes, got {K}")
    if min(min(x.shape) for x in views) < 1:
        raise ValueError(f"ensemble_render needs non-empty views, got {[tuple(x.shape) for x in views]}")
    H, W = tuple(x0.shape[2:]) if size is None else (int(size[0]), int(size[1]))
    if len(views) == 1 and not flips[0]:
        return segment_render(x0, size=(H, W), align_corners=align_corners, palette=palette, background=background, alpha=alpha,
                              min_conf=min_conf, ignore_label=ignore_label, want=want)
    palette, background, alpha256, min_conf, ignore_label, out = _render_args("ensemble_render", x0, B, K, H, W, palette, background,
                                                                              alpha, min_conf, ignore_label, want)
    xs = [_nhwc_any(x.detach()) for x in views]
    V = len(xs)
    _lib.check(_lib.load().oess_segment_render_ensemble(
        (ctypes.c_void_p * V)(*[_ptr(x) for x in xs]), (ctypes.c_longlong * V)(*[_pix_stride(x) for x in xs]),
        (ctypes.c_int * V)(*[x.shape[1] for x in xs]), (ctypes.c_int * V)(*[x.shape[2] for x in xs]),
        (ctypes.c_int * V)(*[int(bool(f)) for f in flips]), V, int(x0.dtype == torch.bfloat16), B, K, H, W, int(bool(align_corners)),
        _ptr(palette), _ptr(background), alpha256, min_conf, ignore_label, _ptr(out.get('labels')), _ptr(out.get('conf')),
        _ptr(out.get('rgb')), _stream()), "oess_segment_render_ensemble")
    for t in out.values():
        _bump(t)
    return out


def vocab_render_max_names(C):
    """The largest name count P hip.vocab_render takes at C channels: its weights [P, C] and bias [P] sit in 48 KB of LDS."""
    return int(_lib.load().oess_head_render_max_names(int(C)))


def vocab_render(x, weight, bias=None, class_offsets=None, palette=None, background=None, alpha=0.5, min_conf=0.0, ignore_label=255,
                 want=SEGMENT_RENDER_OUTPUTS):
    """A linear head and its render in one pass: the outputs of segment_render(conv1x1(x, weight, bias),
    class_offsets=...) at the input size without any [B, P, H, W] tensor.  x: logical B x C x H x W fp32 / bf16, 1 <= C <= 64 (read
    where it is when its channels are dense and its pixels uniformly strided); weight: fp32 [P, C]; bias: fp32 [P] or None, on the
    device.  The value of name p is fmaf(w[p][C-1], x[C-1], ... fmaf(w[p][0], x[0], bias[p]) ...), ascending c, bf16 widened first.
    class_offsets=None: one name per class (K = P <= 255).  ValueError when P exceeds vocab_render_max_names(C) (the weights' LDS
    budget): the caller then forms the logits and calls segment_render(class_offsets=...).  No autograd."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise ValueError("vocab_render needs a CUDA/HIP tensor (no CPU fallback)")
    if x.dtype not in (torch.float32, torch.bfloat16) or x.ndim != 4:
        raise ValueError("vocab_render expects a 4-D float32 / bfloat16 map [B, C, H, W]")
    B, C, H, W = x.shape
    if not 1 <= C <= 64:
        raise ValueError(f"vocab_render handles 1 <= C <= 64 channels, got {C}")
    if min(B, H, W) < 1:
        raise ValueError(f"vocab_render needs a non-empty batch, got {tuple(x.shape)}")
    if (not torch.is_tensor(weight) or weight.dtype != torch.float32 or weight.ndim != 2 or weight.shape[1] != C
            or weight.device != x.device or not weight.is_contiguous()):
        raise ValueError(f"weight must be a contiguous float32 tensor of shape [P, {C}] on {x.device}")
    P = int(weight.shape[0])
    if not 1 <= P <= 1024:
        raise ValueError(f"vocab_render handles 1 <= P <= 1024 names, got {P}")
    if bias is not None and (not torch.is_tensor(bias) or bias.dtype != torch.float32 or tuple(bias.shape) != (P,)
                             or bias.device != x.device or not bias.is_contiguous()):
        raise ValueError(f"bias must be a contiguous float32 tensor of shape {(P,)} on {x.device}, or None")
    offs, K = (None, P) if class_offsets is None else _class_offsets("vocab_render", class_offsets, P, x.device)
    if not 1 <= K <= 255:
        raise ValueError(f"vocab_render handles 1 <= K <= 255 classes, got {K}")
    limit = vocab_render_max_names(C)
    if P > limit:
        raise ValueError(f"vocab_render keeps the weights in LDS: at C = {C} at most {limit} names, got {P}")
    palette, background, alpha256, min_conf, ignore_label, out = _render_args("vocab_render", x, B, K, H, W, palette, background, alpha,
                                                                              min_conf, ignore_label, want)
    xn = _nhwc_any(x.detach())
    _lib.check(_lib.load().oess_head_render(_ptr(xn), int(x.dtype == torch.bfloat16), _pix_stride(xn), B, C, H, W, _ptr(weight.detach()),
                                            _ptr(bias.detach() if bias is not None else None), K, P, _ptr(offs), _ptr(palette),
                                            _ptr(background), alpha256, min_conf, ignore_label, _ptr(out.get('labels')),
                                            _ptr(out.get('conf')), _ptr(out.get('rgb')), _stream()), "oess_head_render")
    for t in out.values():
        _bump(t)
    return out


class _L2Normalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps):
        lib = _lib.load()
        xn = _nhwc_any(x)
        B, H, W, C = xn.shape
        y = torch.empty((B, H, W, C), dtype=x.dtype, device=x.device)
        inv = torch.empty(B * H * W, dtype=torch.float32, device=x.device)
        _lib.check(lib.oess_l2norm_nhwc_fwd(_ptr(xn), _pix_stride(xn), B * H * W, C, int(x.dtype == torch.bfloat16), eps, _ptr(y), C,
                                            _ptr(inv), _stream()), "oess_l2norm_nhwc_fwd")
        ctx.save_for_backward(y, inv)
        ctx.eps = eps
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        y, inv = ctx.saved_tensors
        B, H, W, C = y.shape
        gn = _nhwc_any(g.to(y.dtype))
        gx = torch.empty_like(y)
        _lib.check(lib.oess_l2norm_nhwc_bwd(_ptr(y), C, _ptr(gn), _pix_stride(gn), _ptr(inv), B * H * W, C,
                                            int(y.dtype == torch.bfloat16), ctx.eps, _ptr(gx), C, _stream()), "oess_l2norm_nhwc_bwd")
        return gx.permute(0, 3, 1, 2), None


def l2_normalize(x, eps=1e-12):
    """F.normalize(x, p=2, dim=1, eps) for logical B x C x H x W fp32 / bf16 tensors, differentiable."""
    _need_gpu(x)
    return _L2Normalize.apply(x, float(eps))


_WGRAD_WS_BYTES = 256 << 20


def _wgrad_workspace_check(workspace):
    if workspace.dtype != torch.uint8 or not workspace.is_cuda or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous uint8 CUDA tensor")


def conv2d_wgrad(x, gy, Cout, Cin, R, S, stride=1, pad=0, dil=1, workspace=None, out=None):
    """dW (OIHW fp32) of conv2d_nhwc from NHWC bf16 views x [B,H,W,Cin_x>=Cin] and gy [B,Ho,Wo,Cout].
    workspace: a caller-owned uint8 CUDA tensor for the split-K partial tiles (all of it is on offer, nothing beyond it is
    touched); default: the wrapper's cached 256 MiB buffer.  out: a dense fp32 (Cout, Cin, R, S) tensor to write into."""
    lib = _lib.load()
    _need_gpu(x, gy)
    B, H, W, Cin_x, xps = _nhwc_geom(x)
    _, Ho, Wo, Cg, gps = _nhwc_geom(gy)
    if Cg != Cout:
        raise ValueError("gy channel count != Cout")
    if out is None:
        dw = torch.empty((Cout, Cin, R, S), dtype=torch.float32, device=x.device)
    else:
        if out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (Cout, Cin, R, S):
            raise ValueError(f"out must be a dense fp32 CUDA tensor of shape {(Cout, Cin, R, S)}")
        dw = out
    if workspace is None:
        ws = _workspace(_WGRAD_WS_BYTES, x.device, tag="wgrad")
    else:
        _wgrad_workspace_check(workspace)
        ws = workspace
    _lib.check(lib.oess_conv2d_wgrad_bf16(_ptr(x), xps, B, H, W, Cin_x, _ptr(gy), gps, Cout, Cin, R, S, stride, pad, dil,
                                          _ptr(dw), _ptr(ws), ws.numel(), _stream()), "oess_conv2d_wgrad_bf16")
    return dw


def conv2d_wgrad_route(x, gy, Cout, Cin, R, S, stride=1, pad=0, dil=1, workspace=None, x_pix_stride=None, dy_pix_stride=None):
    """The kernel conv2d_wgrad would launch for these arguments: OESS_WGRAD_* of include/oess.h | slices << 8 (route & 0xff is
    the kernel, route >> 8 the number of partial tiles the reduce kernel sums per element); raises where the call would.  Host
    only, needs no GPU.  With x a tensor the arguments are conv2d_wgrad's own: strides from the views, the workspace's size (the
    default buffer's without one).  With x a (B, H, W, Cin_x) shape gy is not looked at, *_pix_stride stand in for the views
    (default: dense) and workspace is a byte count."""
    lib = _lib.load()
    if torch.is_tensor(x):
        B, H, W, Cin_x, xps = _nhwc_geom(x)
        Cg, gps = _nhwc_geom(gy)[3:]
        if Cg != Cout:
            raise ValueError("gy channel count != Cout")
        if workspace is not None:
            _wgrad_workspace_check(workspace)
        nbytes = _WGRAD_WS_BYTES if workspace is None else workspace.numel()
    else:
        B, H, W, Cin_x = x
        xps = Cin_x if x_pix_stride is None else x_pix_stride
        gps = Cout if dy_pix_stride is None else dy_pix_stride
        nbytes = _WGRAD_WS_BYTES if workspace is None else int(workspace)
    r = lib.oess_conv2d_wgrad_route(B, H, W, Cin_x, Cout, Cin, R, S, stride, pad, dil, xps, gps, nbytes)
    if r < 0:
        _lib.check(r, "oess_conv2d_wgrad_route")
    return r


class _GlobalAvgPool(torch.autograd.Function):
    """nn.AdaptiveAvgPool2d(1) on a channels_last bf16 map -> fp32 [B, C, 1, 1] (models/deeplabv3.py ASPPPooling): per-sample
    channel sums straight from the bf16 map by the deterministic statistics kernel (G = B groups) -- no fp32 copy of the map;
    the backward hands autograd the [B, C, 1, 1] quotient EXPANDED over H x W (stride 0, channels-last compatible), so the sum
    with the other ASPP branches' gradients reads it as a broadcast instead of a materialised, NCHW-ordered tensor."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        xn = x.permute(0, 2, 3, 1)
        B, H, W, C, ps = _nhwc_geom(xn)
        st = torch.empty((2, B, C), dtype=torch.float32, device=x.device)
        ws, wsn = _norm_partials(B, H * W, C, x.device)
        _lib.check(lib.oess_norm_stats_nhwc_bf16(_ptr(xn), ps, B, H * W, C, _ptr(st[0]), _ptr(st[1]), _ptr(ws), wsn, _stream()),
                   "oess_norm_stats_nhwc_bf16")
        ctx.meta = (H, W, x.dtype)
        return (st[0] * (1.0 / (H * W))).view(B, C, 1, 1)

    @staticmethod
    def backward(ctx, g):
        H, W, dtype = ctx.meta
        return (g * (1.0 / (H * W))).to(dtype).expand(-1, -1, H, W)


def global_avg_pool(x):
    """Mean over H x W of a logical B x C x H x W channels_last bf16 tensor -> fp32 [B, C, 1, 1], differentiable."""
    _need_gpu(x)
    if x.dtype != torch.bfloat16 or x.stride(1) != 1:
        raise ValueError("global_avg_pool needs a channels_last bf16 tensor")
    return _GlobalAvgPool.apply(x)


class _LinearProbe(torch.autograd.Function):
    """nn.Conv2d(K, K, 1) on the fp32 channels_last logits (models/style_networks.py:169-170, models/deeplabv3.py:186-187):
    per-pixel K x K product; weight / bias gradients from fixed-order double partial rows (bit-repeatable)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        lib = _lib.load()
        B, K, H, W = x.shape
        y = torch.empty_like(x, memory_format=torch.channels_last)
        w2 = weight.detach().reshape(K, K).contiguous()
        _lib.check(lib.oess_linear_probe_fwd_f32(_ptr(x), _ptr(w2), _ptr(bias.detach()) if bias is not None else None, B * H * W, K,
                                                 _ptr(y), _stream()), "oess_linear_probe_fwd_f32")
        ctx.save_for_backward(x, w2)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, w2 = ctx.saved_tensors
        B, K, H, W = x.shape
        if not _dense_cl(g):
            g = g.contiguous(memory_format=torch.channels_last)
        gx = torch.empty_like(x, memory_format=torch.channels_last) if ctx.needs_input_grad[0] else None
        gw = torch.empty((K, K, 1, 1), dtype=torch.float32, device=x.device)
        gb = torch.empty((K,), dtype=torch.float32, device=x.device)
        nb = lib.oess_linear_probe_partials_bytes(K)
        ws = _workspace(nb, x.device, tag=("linear_probe", torch.cuda.current_stream(x.device).cuda_stream))
        _lib.check(lib.oess_linear_probe_bwd_f32(_ptr(x), _ptr(g), _ptr(w2), B * H * W, K, _ptr(gx) if gx is not None else None,
                                                 _ptr(gw), _ptr(gb), _ptr(ws), nb, _stream()), "oess_linear_probe_bwd_f32")
        return gx, gw, (gb if ctx.has_bias else None)


def _dense_cl(t):
    B, C, H, W = t.shape
    return t.dtype == torch.float32 and t.stride() == (H * W * C, 1, W * C, C)


def linear_probe(x, conv):
    """`conv(x)` for the linear-probe nn.Conv2d(K, K, 1) on fp32 channels_last logits [B, K, H, W], differentiable."""
    _need_gpu(x)
    K = x.shape[1]
    if K > 32 or tuple(conv.weight.shape) != (K, K, 1, 1) or conv.weight.dtype != torch.float32:
        # outside the kernel's range (more than 32 classes, or not the K x K probe): the module's own convolution, said once
        global _PROBE_WARNED
        if not _PROBE_WARNED:
            _PROBE_WARNED = True
            import warnings
            warnings.warn(f"linear_probe: K = {K} / weight {tuple(conv.weight.shape)} is outside the HIP kernel's range "
                          "(K <= 32, K x K x 1 x 1 fp32); using nn.Conv2d for this layer")
        return conv(x)
    if not _dense_cl(x):        # any other layout / dtype of the logits: one re-layout, then the kernel
        x = x.float().contiguous(memory_format=torch.channels_last)
        if not _dense_cl(x):    # degenerate shapes (H * W == 1 ...) where channels_last strides are ambiguous
            x = torch.empty_strided(x.shape, (x.shape[1] * x.shape[2] * x.shape[3], 1, x.shape[3] * x.shape[1], x.shape[1]),
                                    dtype=torch.float32, device=x.device).copy_(x)
    return _LinearProbe.apply(x, conv.weight, conv.bias)


_PROBE_WARNED = False


def channel_sum(x_nhwc):
    """Per-channel sum over all pixels of an NHWC bf16 view (bias gradient) -> fp32 [C]."""
    lib = _lib.load()
    B, H, W, C, ps = _nhwc_geom(x_nhwc)
    st = torch.empty((2, C), dtype=torch.float32, device=x_nhwc.device)
    ws, wsn = _norm_partials(1, B * H * W, C, x_nhwc.device)
    _lib.check(lib.oess_norm_stats_nhwc_bf16(_ptr(x_nhwc), ps, 1, B * H * W, C, _ptr(st[0]), _ptr(st[1]), _ptr(ws), wsn, _stream()),
               "oess_norm_stats_nhwc_bf16")
    return st[0]


ROUTE_CONV1X1_W128 = 14       # OESS_ROUTE_CONV1X1_W128 of include/oess.h (values are stable)
BN_FUSED_MAX_TILES = 320      # up to here conv_bn_train_nhwc takes the one-launch statistics + apply kernel (Cout % 64 == 0)


def conv_bn_train_separate_apply(M, Cout):
    """True where conv_bn_train_nhwc over M output pixels runs conv + reduce_finalize + apply as separate launches with the
    scale / shift in memory between them: the only route on which an apply can be deferred, fused elsewhere or dropped
    (`defer`, `residual_affine`, `want_output`).  Small maps take ONE statistics + apply launch that has no such seam."""
    return (M + 127) // 128 > BN_FUSED_MAX_TILES


class RawBN(NamedTuple):
    """conv_bn_train_nhwc(defer=True): the raw conv result (NHWC bf16) and the BatchNorm's fp32 [1, C] scale / shift for it.  The
    running statistics have moved and the batch counter is bumped; only y * scale + shift is still to be applied."""
    y: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor


def conv_bn_train_nhwc(x, packed, Cout, R, S, stride, pad, dil, bn, relu=False, residual=None, out=None, defer=False,
                       residual_affine=None, want_output=True):
    """Bias-free conv + nn.BatchNorm2d in TRAIN mode [+ residual] [+ ReLU], inference form (frozen teacher): the batch
    statistics come from the conv epilogue's fp32 accumulators (no separate statistics pass over the activation).
    `out`: optional NHWC bf16 destination view (e.g. a channel slice of a concat buffer).
    Three forms exist only where conv_bn_train_separate_apply(M, Cout) holds (ValueError elsewhere: the caller asks first):
      defer=True            no apply: returns RawBN(raw result, scale, shift) for a consumer that applies them itself;
      residual_affine=RawBN the residual is another layer's deferred result: ONE pass normalises both branches
                            (oess_norm_apply2_nhwc_bf16: the bits of that layer's apply followed by this one's);
      want_output=False     nobody reads the result, the call is made for the running statistics: no apply, returns None; a 1x1
                            layer on the w128 GEMM does not store its result either (oess_conv2d_stats_only_bf16)."""
    lib = _lib.load()
    B, H, W, _, xps = _nhwc_geom(x)
    Ho = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (S - 1) - 1) // stride + 1
    M = B * Ho * Wo
    tiles = (M + 127) // 128
    special = defer or residual_affine is not None or not want_output
    if special:
        if not conv_bn_train_separate_apply(M, Cout):
            raise ValueError(f"conv_bn_train_nhwc: M = {M} takes the one-launch statistics + apply kernel: nothing to defer or drop")
        if defer + (residual_affine is not None) + (not want_output) > 1 or (residual_affine is not None and residual is not None):
            raise ValueError("conv_bn_train_nhwc: defer, residual_affine and want_output=False exclude each other")
    part = torch.empty((tiles, 2, Cout), dtype=torch.float32, device=x.device)
    y = None
    if not want_output and R == 1 and S == 1 and stride == 1 and pad == 0 and out is None and \
            conv2d_route((B, H, W, x.shape[3]), None, False, Cout, 1, 1, tile_stats=True, in_pix_stride=xps) == ROUTE_CONV1X1_W128:
        _need_gpu(x, packed)
        _lib.check(lib.oess_conv2d_stats_only_bf16(_ptr(x), xps, B, H, W, x.shape[3], _ptr(packed), Cout, _ptr(part), _stream()),
                   "oess_conv2d_stats_only_bf16")
    else:
        y = conv2d_nhwc(x, packed, None, Cout, R, S, stride, pad, dil, tile_stats=part, out=out)
        _, _, _, _, yps = _nhwc_geom(y)
    mom = 0.0 if bn.momentum is None else bn.momentum
    rps = 0
    if residual is not None:
        _, _, _, _, rps = _nhwc_geom(residual)
    from . import engine as _engine
    if not special and tiles <= BN_FUSED_MAX_TILES and Cout % 64 == 0:
        # small map: statistics + apply in ONE launch (every workgroup reduces the partials of its 64 channels itself)
        _lib.check(lib.oess_norm_tile_stats_apply_nhwc_bf16(_ptr(part), tiles, Cout, float(M), float(bn.eps), _ptr(bn.weight.detach()),
                                                            _ptr(bn.bias.detach()), _ptr(bn.running_mean), _ptr(bn.running_var),
                                                            float(mom), None, None, _ptr(y), yps, _ptr(residual), rps, int(relu), M,
                                                            _ptr(y), yps, _stream()), "oess_norm_tile_stats_apply_nhwc_bf16")
        _engine.bump_bn_counter(bn)
        return y
    st = torch.empty((6, 1, Cout), dtype=torch.float32, device=x.device)
    sc = _stats_scratch(Cout, x.device)
    _lib.check(lib.oess_norm_reduce_finalize_tile_stats(_ptr(part), tiles, Cout, _ptr(sc.buf64), _ptr(sc.tickets),
                                                        float(M), float(bn.eps), _ptr(bn.weight.detach()), _ptr(bn.bias.detach()),
                                                        _ptr(bn.running_mean), _ptr(bn.running_var), float(mom), _ptr(st[2]), _ptr(st[3]),
                                                        _ptr(st[4]), _ptr(st[5]), _stream()), "oess_norm_reduce_finalize_tile_stats")
    if not want_output:
        _engine.bump_bn_counter(bn)
        return None
    if defer:
        _engine.bump_bn_counter(bn)
        return RawBN(y, st[4], st[5])
    if residual_affine is not None:
        r = residual_affine
        if tuple(r.y.shape) != tuple(y.shape) or r.scale.numel() != Cout or r.shift.numel() != Cout:
            raise ValueError(f"conv_bn_train_nhwc: residual_affine of shape {tuple(r.y.shape)} for a result of {tuple(y.shape)}")
        _, _, _, _, r2ps = _nhwc_geom(r.y)
        _lib.check(lib.oess_norm_apply2_nhwc_bf16(_ptr(y), yps, _ptr(st[4]), _ptr(st[5]), _ptr(r.y), r2ps, _ptr(r.scale), _ptr(r.shift),
                                                  int(relu), M, Cout, _ptr(y), yps, _stream()), "oess_norm_apply2_nhwc_bf16")
        _engine.bump_bn_counter(bn)
        return y
    _lib.check(lib.oess_norm_apply_nhwc_bf16(_ptr(y), yps, _ptr(st[4]), _ptr(st[5]), _ptr(residual), rps, int(relu), 1, M, Cout,
                                             _ptr(y), yps, _stream()), "oess_norm_apply_nhwc_bf16")
    _engine.bump_bn_counter(bn)
    return y


def max_pool_3x3s2_affine_relu(x, scale, shift):
    """max_pool_3x3s2(relu(x * scale + shift) rounded to bf16) on a logical NCHW channels_last bf16 tensor, C % 8 == 0, without
    writing the normalised map: the ResNet stem behind a deferred train-mode BatchNorm (conv_bn_train_nhwc(defer=True)).
    scale / shift: fp32, C elements.  No autograd (no winner index is kept)."""
    _need_gpu(x, scale, shift)
    if x.dtype != torch.bfloat16 or x.stride(1) != 1 or x.shape[1] % 8:
        raise ValueError("max_pool_3x3s2_affine_relu needs a channels_last bf16 tensor with C % 8 == 0")
    lib = _lib.load()
    xn = x.permute(0, 2, 3, 1)
    B, H, W, C, ps = _nhwc_geom(xn)
    if scale.dtype != torch.float32 or shift.dtype != torch.float32 or scale.numel() != C or shift.numel() != C or \
            not scale.is_contiguous() or not shift.is_contiguous():
        raise ValueError("max_pool_3x3s2_affine_relu: scale / shift are contiguous fp32 tensors of C elements")
    y = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), dtype=torch.bfloat16, device=x.device)
    _lib.check(lib.oess_maxpool3x3s2_affine_relu_fwd_nhwc_bf16(_ptr(xn), ps, B, H, W, C, _ptr(scale), _ptr(shift), _ptr(y), C, _stream()),
               "oess_maxpool3x3s2_affine_relu_fwd_nhwc_bf16")
    return y.permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------ small ops of the DeepLabv3 path (round 5)
class _MaxPool3x3s2(torch.autograd.Function):
    """nn.MaxPool2d(3, stride=2, padding=1) of the ResNet stem on a channels_last bf16 map (models/_resnet.py:124,197 of the
    reference): forward keeps one byte per output element (the winning tap), backward is a gather (every input element written
    once, fixed order)."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        xn = x.permute(0, 2, 3, 1)
        B, H, W, C, ps = _nhwc_geom(xn)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty((B, Ho, Wo, C), dtype=torch.bfloat16, device=x.device)
        need = ctx.needs_input_grad[0]
        idx = torch.empty((B, Ho, Wo, C), dtype=torch.uint8, device=x.device) if need else None
        _lib.check(lib.oess_maxpool3x3s2_fwd_nhwc_bf16(_ptr(xn), ps, B, H, W, C, _ptr(y), C, _ptr(idx), _stream()),
                   "oess_maxpool3x3s2_fwd_nhwc_bf16")
        ctx.idx, ctx.geom = idx, (B, H, W, C)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        B, H, W, C = ctx.geom
        gn = g.permute(0, 2, 3, 1)
        if gn.dtype != torch.bfloat16 or gn.stride(3) != 1 or not _uniform_pix_stride(gn):
            gn = gn.to(torch.bfloat16).contiguous()
        _, _, _, _, gps = _nhwc_geom(gn)
        gx = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=g.device)
        _lib.check(lib.oess_maxpool3x3s2_bwd_nhwc_bf16(_ptr(gn), gps, _ptr(ctx.idx), B, H, W, C, _ptr(gx), C, _stream()),
                   "oess_maxpool3x3s2_bwd_nhwc_bf16")
        return gx.permute(0, 3, 1, 2)


def max_pool_3x3s2(x):
    """MaxPool2d(kernel_size=3, stride=2, padding=1) on a logical NCHW channels_last bf16 tensor with C % 8 == 0."""
    _need_gpu(x)
    if x.dtype != torch.bfloat16 or x.stride(1) != 1 or x.shape[1] % 8:
        raise ValueError("max_pool_3x3s2 needs a channels_last bf16 tensor with C % 8 == 0")
    return _MaxPool3x3s2.apply(x)


_DROPOUT_CALLS = 0


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed, offset):
        lib = _lib.load()
        xn = x.permute(0, 2, 3, 1)
        B, H, W, C, ps = _nhwc_geom(xn)
        y = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=x.device)
        _lib.check(lib.oess_dropout_nhwc_bf16(_ptr(xn), ps, _ptr(y), C, B * H * W, C, float(p), seed, offset, _stream()),
                   "oess_dropout_nhwc_bf16")
        ctx.meta = (float(p), seed, offset)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        p, seed, offset = ctx.meta
        gn = g.permute(0, 2, 3, 1)
        if gn.dtype != torch.bfloat16 or gn.stride(3) != 1 or not _uniform_pix_stride(gn):
            gn = gn.to(torch.bfloat16).contiguous()
        B, H, W, C, gps = _nhwc_geom(gn)
        gx = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=g.device)
        _lib.check(lib.oess_dropout_nhwc_bf16(_ptr(gn), gps, _ptr(gx), C, B * H * W, C, p, seed, offset, _stream()),
                   "oess_dropout_nhwc_bf16")
        return gx.permute(0, 3, 1, 2), None, None, None


def dropout(x, p, training=True, owner=None):
    """nn.Dropout(p) on a channels_last bf16 map (models/deeplabv3.py:343): Philox mask keyed by (torch.initial_seed(), a call
    counter, element), recomputed in the backward pass instead of stored.  `owner` (the nn.Dropout module) carries its OWN counter:
    the mask sequence of a model then depends on that model's calls only, not on what other models of the process did;
    without an owner the counter is the process-wide one.  Reproducible under torch.manual_seed."""
    global _DROPOUT_CALLS
    if not training or p <= 0.0:
        return x
    _need_gpu(x)
    if x.dtype != torch.bfloat16 or x.stride(1) != 1 or x.shape[1] % 8:
        raise ValueError("dropout needs a channels_last bf16 tensor with C % 8 == 0")
    if owner is not None:
        calls = getattr(owner, "_oess_dropout_calls", 0) + 1
        owner._oess_dropout_calls = calls
        calls += 1 << 40                                         # own sequence: never collides with the process-wide counter
    else:
        _DROPOUT_CALLS += 1
        calls = _DROPOUT_CALLS
    return _Dropout.apply(x, float(p), int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF, calls)


class _ASPPPoolBranch(torch.autograd.Function):
    """ASPPPooling (models/deeplabv3.py:305-316) as one node: AdaptiveAvgPool2d(1) -> 1x1 conv -> BatchNorm2d(train) over the B
    pooled vectors -> ReLU -> the 1x1 map broadcast back over H x W (bilinear from 1x1 == broadcast).  Forward: the per-sample
    channel sums of the bf16 map (statistics kernel) + one B-row GEMV/BatchNorm kernel; backward: per-sample sums of the incoming
    gradient slice, BatchNorm + GEMV adjoints, and the map's gradient as a stride-0 expanded [B, C, 1, 1] quotient."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, run_mean, run_var, momentum, eps):
        lib = _lib.load()
        xn = x.permute(0, 2, 3, 1)
        B, H, W, C, ps = _nhwc_geom(xn)
        Cout = weight.shape[0]
        st = torch.empty((2, B, C), dtype=torch.float32, device=x.device)
        ws, wsn = _norm_partials(B, H * W, C, x.device)
        _lib.check(lib.oess_norm_stats_nhwc_bf16(_ptr(xn), ps, B, H * W, C, _ptr(st[0]), _ptr(st[1]), _ptr(ws), wsn, _stream()),
                   "oess_norm_stats_nhwc_bf16")
        sums = st[0]                                  # per-sample channel sums; pooled = sums / (H W) is applied inside the kernels
        w2 = weight.detach().reshape(Cout, C)
        if w2.dtype != torch.float32 or not w2.is_contiguous():
            w2 = w2.float().contiguous()
        buf = torch.empty((2 * B + 2, Cout), dtype=torch.float32, device=x.device)      # y_pre | z | mean, rstd
        y_pre, z, stat = buf[:B], buf[B:2 * B], buf[2 * B:]
        zb = torch.empty((B, Cout), dtype=torch.bfloat16, device=x.device)
        _lib.check(lib.oess_aspp_pool_fwd_f32(_ptr(sums), 1.0 / (H * W), _ptr(w2), _ptr(gamma.detach()), _ptr(beta.detach()), _ptr(run_mean),
                                              _ptr(run_var), float(momentum), float(eps), B, C, Cout, _ptr(y_pre), _ptr(stat), _ptr(z),
                                              _ptr(zb), _stream()), "oess_aspp_pool_fwd_f32")
        ctx.save_for_backward(sums, w2, gamma.detach(), buf)
        ctx.geom = (B, H, W, C, Cout)
        return zb.view(B, Cout, 1, 1).expand(B, Cout, H, W)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        sums, w2, gamma, buf = ctx.saved_tensors
        B, H, W, C, Cout = ctx.geom
        y_pre, z, stat = buf[:B], buf[B:2 * B], buf[2 * B:]
        gn = g.permute(0, 2, 3, 1)
        if gn.dtype != torch.bfloat16 or gn.stride(3) != 1 or not _uniform_pix_stride(gn):
            gn = gn.to(torch.bfloat16).contiguous()
        _, _, _, _, gps = _nhwc_geom(gn)
        gs = torch.empty((2, B, Cout), dtype=torch.float32, device=g.device)
        ws, wsn = _norm_partials(B, H * W, Cout, g.device)
        _lib.check(lib.oess_norm_stats_nhwc_bf16(_ptr(gn), gps, B, H * W, Cout, _ptr(gs[0]), _ptr(gs[1]), _ptr(ws), wsn, _stream()),
                   "oess_norm_stats_nhwc_bf16")
        out = torch.empty((B * Cout + Cout * C + 2 * Cout,), dtype=torch.float32, device=g.device)
        dy = out[:B * Cout]
        gw = out[B * Cout:B * Cout + Cout * C].view(Cout, C, 1, 1)
        gg = out[B * Cout + Cout * C:B * Cout + Cout * C + Cout]
        gb = out[B * Cout + Cout * C + Cout:]
        gp = torch.empty((B, C), dtype=torch.bfloat16, device=g.device) if ctx.needs_input_grad[0] else None
        _lib.check(lib.oess_aspp_pool_bwd_f32(_ptr(gs[0]), _ptr(sums), 1.0 / (H * W), _ptr(w2), _ptr(gamma), _ptr(y_pre), _ptr(stat), _ptr(z),
                                              B, C, Cout, _ptr(dy), _ptr(gw), _ptr(gg), _ptr(gb), _ptr(gp), _stream()), "oess_aspp_pool_bwd_f32")
        gx = gp.view(B, C, 1, 1).expand(B, C, H, W) if gp is not None else None
        return gx, gw, gg, gb, None, None, None, None


def aspp_pool_branch(x, conv, bn):
    """ASPPPooling.forward for a channels_last bf16 map in TRAIN mode (batch statistics over the B pooled vectors)."""
    _need_gpu(x)
    B = x.shape[0]
    if x.dtype != torch.bfloat16 or x.stride(1) != 1 or x.shape[1] % 8 or x.shape[1] > 2048 or not 2 <= B <= 16:
        raise ValueError("aspp_pool_branch needs a channels_last bf16 map with C % 8 == 0, C <= 2048 and 2 <= B <= 16")
    from . import engine as _engine
    y = _ASPPPoolBranch.apply(x, conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                              0.0 if bn.momentum is None else float(bn.momentum), float(bn.eps))
    _engine.bump_bn_counter(bn)
    return y


# ------------------------------------------------------------------------------------------ f4: E2VID post-processing
class E2VIDHdrState:
    """Device state of the auto-HDR bounds (IntensityRescaler's deque of (Imin, Imax) and its medians): a zero-filled buffer of
    oess_e2vid_postproc_state_bytes(filter_size) bytes, updated on the device by every e2vid_postprocess call that gets it."""

    def __init__(self, filter_size, device):
        nbytes = _lib.load().oess_e2vid_postproc_state_bytes(int(filter_size))
        if nbytes == 0:
            raise ValueError(f"auto_hdr_median_filter_size must be in [0, 255], got {filter_size}")
        self.filter_size = int(filter_size)
        self.buf = torch.zeros(nbytes, dtype=torch.uint8, device=device)

    def bounds(self):
        """(Imin, Imax) after the last call, as float64 (the header's two doubles at byte 32); synchronises with the device."""
        v = self.buf[32:48].view(torch.float64).cpu()
        return float(v[0]), float(v[1])


def e2vid_postprocess(img, weights, amount, bounds=None, hdr_state=None, out_u8=None, out_f32=None, want_f32=False):
    """PostProcessor.process (unsharp mask + intensity rescaling) of fp32 [N, 1, H, W] `img` (any view whose last dimension is
    contiguous) in one launch (fixed `bounds` = (Imin, Imax)) or two (auto-HDR: `hdr_state`, an E2VIDHdrState).  `weights` is the
    5 x 5 fp32 gkern, read on the host (ignored when amount <= 0).  Returns (uint8 [N, H, W], fp32 [N, 1, H, W] = byte / 255 or
    None); the float output is written when `out_f32` is given or `want_f32` is set."""
    lib = _lib.load()
    _need_gpu(img, out_u8, out_f32)
    if img.dtype != torch.float32 or img.dim() != 4 or img.shape[1] != 1 or img.stride(3) != 1:
        raise ValueError("e2vid_postprocess needs an fp32 [N, 1, H, W] tensor whose last dimension is contiguous")
    if (bounds is None) == (hdr_state is None):
        raise ValueError("e2vid_postprocess needs exactly one of bounds=(Imin, Imax) and hdr_state")
    N, _, H, W = img.shape
    w = None
    if amount > 0:
        w = torch.as_tensor(weights, dtype=torch.float32).reshape(-1)
        if w.numel() != 25:
            raise ValueError("e2vid_postprocess needs the 25 weights of a 5 x 5 kernel")
        w = w.cpu().contiguous()
    if out_u8 is None:
        out_u8 = torch.empty((N, H, W), dtype=torch.uint8, device=img.device)
    elif out_u8.dtype != torch.uint8 or tuple(out_u8.shape) != (N, H, W) or not out_u8.is_contiguous():
        raise ValueError("out_u8 must be a contiguous uint8 [N, H, W] tensor")
    if out_f32 is None and want_f32:
        out_f32 = torch.empty((N, 1, H, W), dtype=torch.float32, device=img.device)
    elif out_f32 is not None and (out_f32.dtype != torch.float32 or tuple(out_f32.shape) != (N, 1, H, W) or not out_f32.is_contiguous()):
        raise ValueError("out_f32 must be a contiguous fp32 [N, 1, H, W] tensor")
    geo = (_ptr(img), img.stride(0), img.stride(2) if H > 1 else W, N, H, W, _ptr(w), float(amount))
    if hdr_state is None:
        _lib.check(lib.oess_e2vid_postprocess_f32(*geo, float(bounds[0]), float(bounds[1]), _ptr(out_u8), _ptr(out_f32), _stream()),
                   "oess_e2vid_postprocess_f32")
    else:
        _need_gpu(hdr_state.buf)
        _lib.check(lib.oess_e2vid_postprocess_auto_hdr_f32(*geo, hdr_state.filter_size, _ptr(hdr_state.buf), hdr_state.buf.numel(),
                                                           _ptr(out_u8), _ptr(out_f32), _stream()), "oess_e2vid_postprocess_auto_hdr_f32")
    return out_u8, out_f32


# ------------------------------------------------------------------------------------------ K27: grey levels -> augmented student image
def recon_augment(u8, flip, brightness, contrast, noise_seed, out=None):
    """uint8 [B, H, W] grey levels (PostProcessor.process_u8) -> fp32 [B, 3, H, W]: byte / 255 on three channels, then per sample
    the reference's augmentation of the reconstruction (DSEC/dataset/sequence_ov.py:204-221) in its order: mirror along W
    (`flip[b]`), adjust_brightness (`brightness[b]`, 1.0 = off), adjust_contrast (`contrast[b]`, 1.0 = off), + 0.05 N(0, 1) from
    Philox keyed by `noise_seed[b]` (0 = off).  The four per-sample sequences live on the host and have length B; they travel as
    kernel arguments, so nothing is copied or waited for.  ValueError before any launch for what the call cannot serve."""
    import numpy as np
    if not torch.is_tensor(u8) or u8.dtype != torch.uint8 or u8.dim() != 3:
        raise ValueError("recon_augment needs a uint8 [B, H, W] tensor")
    if not u8.is_cuda:
        raise ValueError("recon_augment needs a GPU tensor (no CPU fallback)")
    if not u8.is_contiguous() or u8.numel() == 0:
        raise ValueError("recon_augment needs a contiguous, non-empty uint8 [B, H, W] tensor")
    B, H, W = u8.shape
    if 3 * H * W >= 2 ** 31:
        raise ValueError(f"recon_augment: a {H} x {W} sample has 2^31 or more output elements")

    def column(name, v, dtype):
        if torch.is_tensor(v):
            if v.is_cuda:
                raise ValueError(f"recon_augment: {name} is a per-sample HOST sequence")
            v = v.numpy()
        a = np.ascontiguousarray(np.asarray(v)).astype(dtype, copy=False).reshape(-1)
        if a.size != B:
            raise ValueError(f"recon_augment: {name} has {a.size} entries for a batch of {B}")
        return np.ascontiguousarray(a)

    raw_flip = column('flip', flip, np.int64)
    if ((raw_flip != 0) & (raw_flip != 1)).any():
        raise ValueError("recon_augment: flip entries are 0 or 1")
    f = raw_flip.astype(np.int32)
    bri, con = column('brightness', brightness, np.float32), column('contrast', contrast, np.float32)
    for name, a in (('brightness', bri), ('contrast', con)):
        if not (np.isfinite(a).all() and (a >= 0).all()):
            raise ValueError(f"recon_augment: {name} factors are finite and >= 0")
    seed = column('noise_seed', noise_seed, np.uint64)
    if out is None:
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=u8.device)
    elif (not torch.is_tensor(out) or not out.is_cuda or out.device != u8.device or out.dtype != torch.float32
          or tuple(out.shape) != (B, 3, H, W) or not out.is_contiguous()):
        raise ValueError("recon_augment: out must be a contiguous fp32 [B, 3, H, W] tensor on u8's device")
    lib = _lib.load()
    ws, need = None, 0
    if (con != 1.0).any():
        need = lib.oess_gray_augment_scratch_bytes(B, H, W)
        ws = _workspace(need, u8.device, tag="recon_augment")
    _lib.check(lib.oess_gray_augment_rgb_f32(_ptr(u8), B, H, W, f.ctypes.data, bri.ctypes.data, con.ctypes.data, seed.ctypes.data,
                                             _ptr(out), _ptr(ws), need, _stream()), "oess_gray_augment_rgb_f32")
    _bump(out)
    return out


# ------------------------------------------------------------------------------------------ K14: fp32 E2VID inference
_F32_ACT = {None: 0, 'relu': 1, 'sigmoid': 2}


def _f32_view(t, what):
    """Logical [B, C, H, W] fp32 tensor with any strides (NCHW, channels_last, channel / crop views) -> oess_f32_view_t."""
    if t.dtype != torch.float32 or t.ndim != 4:
        raise ValueError(f"{what} must be a 4-D float32 tensor [B, C, H, W]")
    return _lib.F32View(t.data_ptr(), t.stride(0), t.stride(2), t.stride(3), t.stride(1))


def _f32_ref(v):
    return None if v is None else ctypes.byref(v)


def _f32_operands(x, x2, packed, bias, Cout, need):
    _need_gpu(x, x2, packed, bias)
    vx = _f32_view(x, "x")
    v2 = None
    if x2 is not None:
        if tuple(x2.shape) != tuple(x.shape):
            raise ValueError(f"x2 {tuple(x2.shape)} must have the shape of x {tuple(x.shape)}")
        v2 = _f32_view(x2, "x2")
    if packed.dtype != torch.float32 or not packed.is_contiguous() or need == 0 or packed.numel() < need:
        raise ValueError(f"packed weight must be a contiguous fp32 tensor of at least {need} floats")
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous() or bias.numel() != Cout):
        raise ValueError(f"bias must be a contiguous fp32 tensor of {Cout} elements")
    return vx, v2


def _f32_out(out, B, Cout, Ho, Wo, device):
    if out is None:
        return torch.empty((B, Ho, Wo, Cout), dtype=torch.float32, device=device).permute(0, 3, 1, 2)
    _need_gpu(out)
    if tuple(out.shape) != (B, Cout, Ho, Wo):
        raise ValueError(f"bad output shape {tuple(out.shape)} != {(B, Cout, Ho, Wo)}")
    return out


def _f32_residual(residual, shape):
    """The view of a residual, which must have `shape`; None stays None."""
    if residual is None:
        return None
    if tuple(residual.shape) != shape:
        raise ValueError(f"residual shape {tuple(residual.shape)} != {shape}")
    return _f32_view(residual, "residual")


def _f32_workspace(need, what, shape, device, tag):
    """The `tag` workspace for the `need` bytes a query answered; 0 bytes: `what` has no kernel for a map of `shape`."""
    if need == 0:
        raise ValueError(f"{what}: no kernel for a {shape} map")
    return _workspace(need, device, tag=tag)


def _f32_grad(g):
    """An incoming gradient in fp32 (autograd may hand over another dtype)."""
    return g if g.dtype == torch.float32 else g.float()


def pack_conv_weight_f32(w):
    """Conv2d weight [Cout, Cin, R, S] -> the fp32 operand of oess_conv2d_fwd_f32: [ceil16(R S Cin)][ceil32(Cout)], row
    (r S + s) Cin + ci (include/oess.h).  Parameter preparation, once per weight version (engine.PackedWeightF32)."""
    Co, Ci, R, S = w.shape
    n = _lib.load().oess_conv2d_f32_packed_floats(Co, Ci, R, S)
    if n == 0:
        raise ValueError(f"no fp32 packing for a {tuple(w.shape)} weight")
    Kp, Cp = (R * S * Ci + 15) // 16 * 16, (Co + 31) // 32 * 32
    out = torch.zeros((Kp, Cp), dtype=torch.float32, device=w.device)
    out[:R * S * Ci, :Co] = w.detach().float().permute(2, 3, 1, 0).reshape(R * S * Ci, Co)
    return out


def pack_conv_transpose_weight_f32(w):
    """ConvTranspose2d weight [Cin, Cout, 5, 5] -> the four phase blocks of oess_conv_transpose2d_fwd_f32 (include/oess.h)."""
    Ci, Co, R, S = w.shape
    if (R, S) != (5, 5):
        raise ValueError("oess_conv_transpose2d_fwd_f32 takes 5 x 5 kernels")
    Cp = (Co + 31) // 32 * 32
    blocks = []
    for p in range(4):
        py, px = p >> 1, p & 1
        sub = w.detach().float()[:, :, py::2, px::2]                  # [Cin, Cout, ny, nx]: taps ky = py + 2 ty
        ny, nx = sub.shape[2], sub.shape[3]
        blk = torch.zeros(((ny * nx * Ci + 15) // 16 * 16, Cp), dtype=torch.float32, device=w.device)
        blk[:ny * nx * Ci, :Co] = sub.permute(2, 3, 0, 1).reshape(ny * nx * Ci, Co)
        blocks.append(blk)
    out = torch.cat(blocks, 0).reshape(-1)
    assert out.numel() == _lib.load().oess_conv_transpose2d_f32_packed_floats(Co, Ci)
    return out


def conv2d_f32(x, packed, bias, Cout, R, S, stride=1, pad=0, act=None, x2=None, upsample2x=False, residual=None, out=None,
               dilation=1):
    """out = act(conv(x [+ x2]) + bias [+ residual]) in fp32 on the f32-input MFMA (oess_conv2d_fwd_f32).  x, x2, residual, out:
    logical [B, C, H, W] fp32 tensors with any strides (channels_last and channel slices take the vector loads); act: None, 'relu'
    or 'sigmoid'; upsample2x: convolve the bilinear x2 (align_corners=False) of x [+ x2].  dilation > 1, pad >= R or more than 25
    taps (DeepLabv3: the 7 x 7 stem, the atrous convs) go to oess_conv2d_dilated_fwd_f32, the same kernel without the geometry
    limits.  Returns out (channels_last if new)."""
    lib = _lib.load()
    B, Cin, H, W = x.shape
    vx, v2 = _f32_operands(x, x2, packed, bias, Cout, lib.oess_conv2d_f32_packed_floats(Cout, Cin, R, S))
    if act not in _F32_ACT:
        raise ValueError(f"act must be one of {list(_F32_ACT)}")
    Hl, Wl = (2 * H, 2 * W) if upsample2x else (H, W)
    if dilation < 1 or Hl + 2 * pad < dilation * (R - 1) + 1 or Wl + 2 * pad < dilation * (S - 1) + 1:
        raise ValueError(f"conv2d_f32: no output for a {Hl} x {Wl} map, {R} x {S} taps, pad {pad}, dilation {dilation}")
    Ho, Wo = (Hl + 2 * pad - dilation * (R - 1) - 1) // stride + 1, (Wl + 2 * pad - dilation * (S - 1) - 1) // stride + 1
    out = _f32_out(out, B, Cout, Ho, Wo, x.device)
    _need_gpu(residual)
    vr = _f32_residual(residual, (B, Cout, Ho, Wo))
    vo = _f32_view(out, "out")
    if dilation == 1 and R * S <= 25 and pad < R and pad < S:
        _lib.check(lib.oess_conv2d_fwd_f32(ctypes.byref(vx), _f32_ref(v2), B, H, W, Cin, int(bool(upsample2x)), _ptr(packed), _ptr(bias),
                                           Cout, R, S, stride, pad, _F32_ACT[act], _f32_ref(vr), ctypes.byref(vo), _stream()),
                   "oess_conv2d_fwd_f32")
    else:
        _lib.check(lib.oess_conv2d_dilated_fwd_f32(ctypes.byref(vx), _f32_ref(v2), B, H, W, Cin, int(bool(upsample2x)), _ptr(packed),
                                                   _ptr(bias), Cout, R, S, stride, pad, dilation, _F32_ACT[act], _f32_ref(vr),
                                                   ctypes.byref(vo), _stream()), "oess_conv2d_dilated_fwd_f32")
    _bump(out)
    return out


def conv_transpose2d_f32(x, packed, bias, Cout, act=None, x2=None, out=None):
    """ConvTranspose2d(k 5, stride 2, padding 2, output_padding 1) of x [+ x2] + bias, act, in fp32: four phase sub-convolutions in
    one launch (oess_conv_transpose2d_fwd_f32).  `packed` from pack_conv_transpose_weight_f32.  out: [B, Cout, 2H, 2W]."""
    lib = _lib.load()
    B, Cin, H, W = x.shape
    vx, v2 = _f32_operands(x, x2, packed, bias, Cout, lib.oess_conv_transpose2d_f32_packed_floats(Cout, Cin))
    if act not in _F32_ACT:
        raise ValueError(f"act must be one of {list(_F32_ACT)}")
    out = _f32_out(out, B, Cout, 2 * H, 2 * W, x.device)
    vo = _f32_view(out, "out")
    _lib.check(lib.oess_conv_transpose2d_fwd_f32(ctypes.byref(vx), _f32_ref(v2), B, H, W, Cin, _ptr(packed), _ptr(bias), Cout,
                                                 _F32_ACT[act], ctypes.byref(vo), _stream()), "oess_conv_transpose2d_fwd_f32")
    _bump(out)
    return out


def convlstm_step_f32(xh, packed, bias, C, k, pad, cell, hidden_out, prev_cell_is_zero=False):
    """One fp32 ConvLSTM step (oess_convlstm_step_f32): gates = conv(xh) + bias (k x k, `pad`), then the cell update in place in
    `cell` (contiguous fp32 [B, H, W, C]) and the new hidden state into `hidden_out` (a [B, C, H, W] fp32 view, e.g. the h half of
    the cat(x, h) buffer that xh belongs to: the gates are complete before it is written).  xh: [B, Cin, H, W] fp32 view."""
    lib = _lib.load()
    B, Cin, H, W = xh.shape
    vx, _ = _f32_operands(xh, None, packed, bias, 4 * C, lib.oess_conv2d_f32_packed_floats(4 * C, Cin, k, k))
    _need_gpu(cell, hidden_out)
    if cell.dtype != torch.float32 or not cell.is_contiguous() or tuple(cell.shape) != (B, H, W, C):
        raise ValueError(f"cell must be a contiguous fp32 [B, H, W, C] = {(B, H, W, C)} tensor")
    if tuple(hidden_out.shape) != (B, C, H, W):
        raise ValueError(f"hidden_out shape {tuple(hidden_out.shape)} != {(B, C, H, W)}")
    vh = _f32_view(hidden_out, "hidden_out")
    need = lib.oess_convlstm_f32_workspace_bytes(B * H * W, C)
    ws = _workspace(need, xh.device, tag="convlstm_f32")
    _lib.check(lib.oess_convlstm_step_f32(ctypes.byref(vx), B, H, W, Cin, _ptr(packed), _ptr(bias), C, k, k, pad, int(bool(prev_cell_is_zero)),
                                          _ptr(cell), ctypes.byref(vh), _ptr(ws), ws.numel(), _stream()), "oess_convlstm_step_f32")
    _bump(cell)
    _bump(hidden_out)
    return hidden_out


def convgru_gates_f32(pre, h_prev, u, rh_out):
    """fp32 ConvGRU gates (oess_convgru_gates_f32, K28): pre = contiguous fp32 [B, H, W, 2C] pre-activations (update | reset);
    u = sigmoid(update) -> `u` (contiguous fp32 [B, H, W, C]); sigmoid(reset) * h_prev -> `rh_out`.  h_prev, rh_out: [B, C, H, W]
    fp32 views (h_prev None: zero state)."""
    lib = _lib.load()
    _need_gpu(pre, h_prev, u, rh_out)
    B, C, H, W = rh_out.shape
    _convgru_f32_state(pre, (B, H, W, 2 * C), "convgru_gates_f32: pre")
    _convgru_f32_state(u, (B, H, W, C), "convgru_gates_f32: u")
    if h_prev is not None and tuple(h_prev.shape) != (B, C, H, W):
        raise ValueError(f"convgru_gates_f32: h_prev shape {tuple(h_prev.shape)} != {(B, C, H, W)}")
    vh = None if h_prev is None else _f32_view(h_prev, "h_prev")
    vr = _f32_view(rh_out, "rh_out")
    _lib.check(lib.oess_convgru_gates_f32(_ptr(pre), _f32_ref(vh), B, H, W, C, _ptr(u), ctypes.byref(vr), _stream()),
               "oess_convgru_gates_f32")
    _bump(u)
    _bump(rh_out)
    return u


def convgru_blend_f32(pre, u, h_prev, h_out):
    """fp32 ConvGRU blend (oess_convgru_blend_f32, K28): h_out = h_prev (1 - u) + tanh(pre) u.  pre, u: contiguous fp32
    [B, H, W, C]; h_prev (None: zero state), h_out: [B, C, H, W] fp32 views; h_out may be h_prev."""
    lib = _lib.load()
    _need_gpu(pre, u, h_prev, h_out)
    B, C, H, W = h_out.shape
    _convgru_f32_state(pre, (B, H, W, C), "convgru_blend_f32: pre")
    _convgru_f32_state(u, (B, H, W, C), "convgru_blend_f32: u")
    if h_prev is not None and tuple(h_prev.shape) != (B, C, H, W):
        raise ValueError(f"convgru_blend_f32: h_prev shape {tuple(h_prev.shape)} != {(B, C, H, W)}")
    vh = None if h_prev is None else _f32_view(h_prev, "h_prev")
    vo = _f32_view(h_out, "h_out")
    _lib.check(lib.oess_convgru_blend_f32(_ptr(pre), _ptr(u), _f32_ref(vh), B, H, W, C, ctypes.byref(vo), _stream()),
               "oess_convgru_blend_f32")
    _bump(h_out)
    return h_out


def convgru_step_f32(hxr, gates_packed, gates_bias, out_packed, out_bias, C, k, pad, h_is_zero=False):
    """One fp32 ConvGRU step (K28) on the state buffer hxr = fp32 [B, H, W, 3C] ordered h | x | r h, whose x window was just
    written: conv2d_f32 of the (h | x) window -> gates -> conv2d_f32 of the (x | r h) window -> blend into the h window: four
    launches.  gates_packed: pack_conv_weight_f32 of the [2C, 2C, k, k] weight (rows update | reset, input channels h | x),
    out_packed of the out gate's weight in its own (x | r h) order; h_is_zero: both are the x-half operands ([.., C, k, k]) and
    only the x window is convolved.  Returns the h window as a [B, C, H, W] view."""
    lib = _lib.load()
    _need_gpu(hxr)
    if hxr.dtype != torch.float32 or hxr.ndim != 4 or not hxr.is_contiguous() or hxr.shape[3] != 3 * C:
        raise ValueError("convgru_step_f32: the state buffer is contiguous fp32 [B, H, W, 3C]")
    B, H, W, _ = hxr.shape
    P = B * H * W
    need = lib.oess_convgru_f32_workspace_bytes(P, C)
    ws = _f32_workspace(need, "convgru_step_f32", (B, H, W, C), hxr.device, "convgru_f32").view(torch.float32)
    pre = ws[:2 * P * C].view(B, H, W, 2 * C)
    u = ws[2 * P * C:3 * P * C].view(B, H, W, C)
    pre_o = ws[3 * P * C:4 * P * C].view(B, H, W, C)
    win = lambda c0, c1: hxr[..., c0:c1].permute(0, 3, 1, 2)
    h = win(0, C)
    conv2d_f32(win(C, 2 * C) if h_is_zero else win(0, 2 * C), gates_packed, gates_bias, 2 * C, k, k, 1, pad, out=pre.permute(0, 3, 1, 2))
    convgru_gates_f32(pre, None if h_is_zero else h, u, win(2 * C, 3 * C))
    conv2d_f32(win(C, 2 * C) if h_is_zero else win(C, 3 * C), out_packed, out_bias, C, k, k, 1, pad, out=pre_o.permute(0, 3, 1, 2))
    convgru_blend_f32(pre_o, u, None if h_is_zero else h, h)
    return h


# ------------------------------------------------------------------------------------------ K15: fp32 SemSegE2VID inference
def instance_norm_f32(x, relu=False, residual=None, eps=1e-5, out=None):
    """nn.InstanceNorm2d(affine=False, eps) [+ residual] [+ ReLU] in fp32 (oess_instance_norm_fwd_f32): x, residual, out logical
    [B, C, H, W] fp32 tensors with any strides (channels_last and channel slices of it take the vector path); out may be x
    itself.  Statistics are merged from shifted per-thread sums in a fixed order: stable and bit-repeatable.  Returns out."""
    lib = _lib.load()
    _need_gpu(x, residual, out)
    if relu and residual is not None:
        raise NotImplementedError("ReLU after the residual add is not a pattern of the reference")
    vx = _f32_view(x, "x")
    B, C, H, W = x.shape
    vr = _f32_residual(residual, (B, C, H, W))
    out = _f32_out(out, B, C, H, W, x.device)
    vo = _f32_view(out, "out")
    ws = _f32_workspace(lib.oess_instance_norm_f32_workspace_bytes(B, H, W, C), "instance_norm_f32", (B, C, H, W), x.device,
                        "instnorm_f32")
    _lib.check(lib.oess_instance_norm_fwd_f32(ctypes.byref(vx), B, H, W, C, float(eps), int(bool(relu)), _f32_ref(vr), ctypes.byref(vo),
                                              _ptr(ws), ws.numel(), _stream()), "oess_instance_norm_fwd_f32")
    _bump(out)
    return out


def upsample2x_concat_f32(x, skip=None, out=None):
    """cat([F.interpolate(x, scale_factor=2, mode='nearest'), skip], 1) in fp32 written by one gather kernel
    (oess_upsample_nearest2x_concat_f32).  x [B, C, H, W], skip [B, Cs, 2H, 2W] or None: fp32 tensors with any strides (the E2VID
    latents are read where they are).  Returns out [B, C + Cs, 2H, 2W] (channels_last if new)."""
    lib = _lib.load()
    _need_gpu(x, skip, out)
    vx = _f32_view(x, "x")
    B, C, H, W = x.shape
    Cs, vs = 0, None
    if skip is not None:
        if skip.ndim != 4 or (skip.shape[0], skip.shape[2], skip.shape[3]) != (B, 2 * H, 2 * W):
            raise ValueError(f"skip {tuple(skip.shape)} must be [B, Cs, 2H, 2W] = {(B, '*', 2 * H, 2 * W)}")
        Cs, vs = skip.shape[1], _f32_view(skip, "skip")
    out = _f32_out(out, B, C + Cs, 2 * H, 2 * W, x.device)
    vo = _f32_view(out, "out")
    _lib.check(lib.oess_upsample_nearest2x_concat_f32(ctypes.byref(vx), B, H, W, C, _f32_ref(vs), Cs, ctypes.byref(vo), _stream()),
               "oess_upsample_nearest2x_concat_f32")
    _bump(out)
    return out


# ------------------------------------------------------------------------------------------ K16: fp32 DeepLabv3 inference
def max_pool_3x3s2_f32(x, out=None):
    """nn.MaxPool2d(3, stride=2, padding=1) in fp32 (oess_maxpool3x3s2_fwd_f32): x, out logical [B, C, H, W] fp32 tensors with any
    strides (channels_last takes 16-byte loads).  Exact: values are selected, not computed.  Returns out (channels_last if new)."""
    lib = _lib.load()
    _need_gpu(x, out)
    vx = _f32_view(x, "x")
    B, C, H, W = x.shape
    out = _f32_out(out, B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1, x.device)
    vo = _f32_view(out, "out")
    _lib.check(lib.oess_maxpool3x3s2_fwd_f32(ctypes.byref(vx), B, H, W, C, ctypes.byref(vo), _stream()), "oess_maxpool3x3s2_fwd_f32")
    _bump(out)
    return out


def global_avg_pool_f32(x):
    """nn.AdaptiveAvgPool2d(1) in fp32 (oess_global_avg_pool_fwd_f32): x logical [B, C, H, W] fp32 with any strides -> fp32
    [B, C, 1, 1] (channels dense).  Fixed summation order: bit-repeatable."""
    lib = _lib.load()
    _need_gpu(x)
    vx = _f32_view(x, "x")
    B, C, H, W = x.shape
    ws = _f32_workspace(lib.oess_global_avg_pool_f32_workspace_bytes(B, H, W, C), "global_avg_pool_f32", (B, C, H, W), x.device,
                        "avgpool_f32")
    out = torch.empty((B, 1, 1, C), dtype=torch.float32, device=x.device).permute(0, 3, 1, 2)     # NHWC: the 1 x 1 conv's vector loads
    _lib.check(lib.oess_global_avg_pool_fwd_f32(ctypes.byref(vx), B, H, W, C, _ptr(out), _ptr(ws), ws.numel(), _stream()),
               "oess_global_avg_pool_fwd_f32")
    return out


# ------------------------------------------------------------------------------------------ K17: fp32 image-teacher inference
def batch_norm_train_f32(x, bn, relu=False, residual=None, out=None, return_stats=False):
    """nn.BatchNorm2d in TRAIN mode [+ residual] [+ ReLU] in fp32 (oess_batch_norm_train_fwd_f32), inference only (no autograd):
    batch statistics over B x H x W, the running statistics moved one momentum step (unbiased variance) and, for a module,
    num_batches_tracked counted, as torch does.  x, residual, out: logical [B, C, H, W] fp32 tensors with any strides
    (channels_last and channel slices of it take the vector path); out may be x itself.  bn: an nn.BatchNorm2d, or a dict with
    'weight', 'bias', 'running_mean', 'running_var' (fp32 [C] or None), 'momentum' and 'eps'.  Statistics are merged from shifted
    per-thread sums in a fixed order: stable and bit-repeatable.  Returns out, or (out, batch mean, biased batch variance)."""
    if isinstance(bn, dict):
        module, p = None, bn
    else:
        module, p = bn, dict(weight=bn.weight, bias=bn.bias, running_mean=bn.running_mean, running_var=bn.running_var,
                             momentum=bn.momentum, eps=bn.eps)
    if p.get('momentum', 0.1) is None:
        raise NotImplementedError("batch_norm_train_f32: momentum=None (cumulative moving average) is not built")
    lib = _lib.load()
    gamma, beta, rm, rv = (p.get(k) for k in ('weight', 'bias', 'running_mean', 'running_var'))
    gamma, beta = (None if t is None else t.detach() for t in (gamma, beta))
    _need_gpu(x, residual, out, gamma, beta, rm, rv)
    vx = _f32_view(x, "x")
    B, C, H, W = x.shape
    if (rm is None) != (rv is None):
        raise ValueError("running_mean and running_var come together")
    for name, t in (('weight', gamma), ('bias', beta), ('running_mean', rm), ('running_var', rv)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != C):
            raise ValueError(f"batch_norm_train_f32: {name} must be a contiguous fp32 tensor of {C} elements")
    vr = _f32_residual(residual, (B, C, H, W))
    if B * H * W < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    out = _f32_out(out, B, C, H, W, x.device)
    vo = _f32_view(out, "out")
    ws = _f32_workspace(lib.oess_batch_norm_train_f32_workspace_bytes(B, H, W, C), "batch_norm_train_f32", (B, C, H, W), x.device,
                        "batchnorm_f32")
    stats = torch.empty((2, C), dtype=torch.float32, device=x.device) if return_stats else None
    _lib.check(lib.oess_batch_norm_train_fwd_f32(ctypes.byref(vx), B, H, W, C, _ptr(gamma), _ptr(beta), float(p.get('eps', 1e-5)),
                                                 float(p.get('momentum', 0.1)), _ptr(rm), _ptr(rv),
                                                 None if stats is None else _ptr(stats[0]), None if stats is None else _ptr(stats[1]),
                                                 int(bool(relu)), _f32_ref(vr), ctypes.byref(vo), _ptr(ws), ws.numel(), _stream()),
               "oess_batch_norm_train_fwd_f32")
    _bump(out)
    if rm is not None:
        _bump(rm)
        _bump(rv)
    if module is not None:
        from . import engine as _engine
        _engine.bump_bn_counter(module)
    return (out, stats[0], stats[1]) if return_stats else out


# ------------------------------------------------------------------------------------------ K18: fp32 SemSegE2VID training
def pack_conv_weight_f32_dgrad(w):
    """Conv2d weight [Cout, Cin, R, S] -> the operand with which oess_conv2d_fwd_f32 computes the DATA gradient of the stride-1
    convolution: dX = conv(dY, W', pad' = R - 1 - pad) with W'[ci][co][r][s] = W[co][ci][R - 1 - r][S - 1 - s], in
    pack_conv_weight_f32's layout: [ceil16(R S Cout)][ceil32(Cin)], row (r S + s) Cout + co, column ci.  Needs no library."""
    Co, Ci, R, S = w.shape
    Kp, Cp = (R * S * Co + 15) // 16 * 16, (Ci + 31) // 32 * 32
    out = torch.zeros((Kp, Cp), dtype=torch.float32, device=w.device)
    out[:R * S * Co, :Ci] = w.detach().float().flip(2, 3).permute(2, 3, 0, 1).reshape(R * S * Co, Ci)
    return out


def _wgrad_f32_check(x, dy, R, stride, pad, dilation):
    for name, t in (("x", x), ("dy", dy)):
        if t.dtype != torch.float32 or t.ndim != 4:
            raise ValueError(f"conv2d_wgrad_f32: {name} must be a 4-D fp32 tensor [B, C, H, W]")
    if stride != 1 or dilation != 1 or R not in (1, 3) or pad != (R - 1) // 2:
        raise ValueError(f"conv2d_wgrad_f32 runs stride 1, dilation 1, 1 x 1 or 3 x 3 taps with 'same' padding, not "
                         f"stride {stride}, dilation {dilation}, {R} x {R}, pad {pad}")
    if (x.shape[0], x.shape[2], x.shape[3]) != (dy.shape[0], dy.shape[2], dy.shape[3]):
        raise ValueError(f"conv2d_wgrad_f32: x {tuple(x.shape)} and dy {tuple(dy.shape)} must share B, H, W")


def _wgrad_f32_launch(name, x, dy, R, stride, pad, dilation, want_db):
    """What conv2d_wgrad_f32 and conv2d_dilated_wgrad_f32 (`name`) do after their own checks: the workspace of the C entry
    oess_<name>, (dw, db) and the launch."""
    _need_gpu(x, dy)
    lib = _lib.load()
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    need = getattr(lib, f"oess_{name}_workspace_bytes")(B, H, W, Cin, Cout, R, R, stride, pad, dilation)
    if need == 0:
        raise ValueError(f"{name}: no kernel for x {tuple(x.shape)}, dy {tuple(dy.shape)}, {R} x {R}")
    ws = _workspace(need, x.device, tag="wgrad_f32")
    dw = torch.empty((Cout, Cin, R, R), dtype=torch.float32, device=x.device)
    db = torch.empty((Cout,), dtype=torch.float32, device=x.device) if want_db else None
    vx, vg = _f32_view(x, "x"), _f32_view(dy, "dy")
    _lib.check(getattr(lib, f"oess_{name}")(ctypes.byref(vx), ctypes.byref(vg), B, H, W, Cin, Cout, R, R, stride, pad, dilation, _ptr(dw),
                                            _ptr(db), _ptr(ws), ws.numel(), _stream()), f"oess_{name}")
    return dw, db


def conv2d_wgrad_f32_splits(B, H, W, Cin, Cout, R):
    """Number of pixel ranges oess_conv2d_wgrad_f32 splits its reduction into for these shapes (a function of the shapes alone),
    read off the workspace query: n (R R Cin Cout + Cout) floats."""
    need = _lib.load().oess_conv2d_wgrad_f32_workspace_bytes(B, H, W, Cin, Cout, R, R, 1, (R - 1) // 2, 1)
    return need // (4 * (R * R * Cin * Cout + Cout))


def conv2d_wgrad_f32(x, dy, R, stride=1, pad=None, dilation=1, want_db=True):
    """Weight and bias gradient of y = conv(x, w, stride 1, 'same' pad) + b in fp32 on the f32-input MFMA (oess_conv2d_wgrad_f32):
    (dw [Cout, Cin, R, R], db [Cout] or None).  x [B, Cin, H, W], dy [B, Cout, H, W]: fp32 tensors with any strides, read where
    they lie (channels_last and channel slices of it take the vector loads).  Fixed summation order: bit-repeatable."""
    pad = (R - 1) // 2 if pad is None else pad
    _wgrad_f32_check(x, dy, R, stride, pad, dilation)
    return _wgrad_f32_launch("conv2d_wgrad_f32", x, dy, R, stride, pad, dilation, want_db)


def conv2d_f32_train(x, weight, bias=None, stride=1, pad=None, dilation=1, act=None, pw=None, ver=None):
    """Differentiable fp32 convolution for training (K18): conv2d_f32 of x with the PARAMETER tensors weight [Cout, Cin, R, R]
    (R in {1, 3}) and bias, stride 1, 'same' padding.  Backward: the weight / bias gradient on oess_conv2d_wgrad_f32 and the data
    gradient on the forward kernel with the operand of pack_conv_weight_f32_dgrad; a gradient nobody asks for (the latents of a
    frozen encoder) is not computed.  pw: an engine.PackedWeightF32 that keeps the two packed operands per weight version (ver:
    the version key of a weight that is itself computed from parameters); without it the operands are packed per call.
    act: None only (the decoder's ReLUs sit behind the norm).  fp32 in, fp32 out; everything else raises before any launch."""
    if x.dtype != torch.float32 or weight.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
        raise ValueError("conv2d_f32_train takes fp32 tensors (the bf16 training path is engine.conv2d_train)")
    if x.ndim != 4 or weight.ndim != 4 or weight.shape[2] != weight.shape[3] or weight.shape[1] != x.shape[1]:
        raise ValueError(f"conv2d_f32_train: x {tuple(x.shape)} does not fit a weight {tuple(weight.shape)}")
    R = weight.shape[2]
    pad = (R - 1) // 2 if pad is None else pad
    if stride != 1 or dilation != 1 or R not in (1, 3) or pad != (R - 1) // 2:
        raise ValueError(f"conv2d_f32_train runs stride 1, dilation 1, 1 x 1 or 3 x 3 taps with 'same' padding, not stride {stride}, "
                         f"dilation {dilation}, {R} x {R}, pad {pad} (strided and dilated weight gradients are not built)")
    if act is not None:
        raise ValueError("conv2d_f32_train has no fused activation")
    _need_gpu(x, weight, bias)
    if pw is None:
        from . import engine as _engine
        pw = _engine.PackedWeightF32()
    return _Conv2dDilatedF32Train.apply(x, weight, bias, 1, pad, 1, conv2d_wgrad_f32, pw, ver)


class _InstanceNormF32Train(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, relu, eps):
        lib = _lib.load()
        B, C, H, W = x.shape
        vx = _f32_view(x, "x")
        vr = None if residual is None else _f32_view(residual, "residual")
        out = _f32_out(None, B, C, H, W, x.device)
        vo = _f32_view(out, "out")
        stats = torch.empty((2, B, C), dtype=torch.float32, device=x.device)
        ws = _f32_workspace(lib.oess_instance_norm_f32_workspace_bytes(B, H, W, C), "instance_norm_f32_train", (B, C, H, W), x.device,
                            "instnorm_f32")
        _lib.check(lib.oess_instance_norm_train_fwd_f32(ctypes.byref(vx), B, H, W, C, float(eps), int(relu), _f32_ref(vr),
                                                        ctypes.byref(vo), _ptr(stats[0]), _ptr(stats[1]), _ptr(ws), ws.numel(),
                                                        _stream()), "oess_instance_norm_train_fwd_f32")
        ctx.save_for_backward(x, stats)
        ctx.relu, ctx.has_res = relu, residual is not None
        return out

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.load()
        x, stats = ctx.saved_tensors
        B, C, H, W = x.shape
        gy = _f32_grad(gy)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _f32_out(None, B, C, H, W, x.device)
            vx, vg, vd = _f32_view(x, "x"), _f32_view(gy, "dy"), _f32_view(dx, "dx")
            need = lib.oess_instance_norm_bwd_f32_workspace_bytes(B, H, W, C)
            ws = _workspace(need, x.device, tag="instnorm_bwd_f32")
            _lib.check(lib.oess_instance_norm_bwd_f32(ctypes.byref(vx), ctypes.byref(vg), _ptr(stats[0]), _ptr(stats[1]), B, H, W, C,
                                                      int(ctx.relu), ctypes.byref(vd), _ptr(ws), ws.numel(), _stream()),
                       "oess_instance_norm_bwd_f32")
        return dx, (gy if ctx.has_res and ctx.needs_input_grad[1] else None), None, None


def instance_norm_f32_train(x, relu=False, residual=None, eps=1e-5):
    """Differentiable nn.InstanceNorm2d(affine=False, eps) [+ residual] [+ ReLU] in fp32 (K18), not in place: the forward is
    instance_norm_f32's kernels and bits, and keeps x and the per-(sample, channel) mean and rstd for
    oess_instance_norm_bwd_f32.  The residual's gradient is the incoming gradient itself (no copy)."""
    if x.dtype != torch.float32 or x.ndim != 4 or (residual is not None and residual.dtype != torch.float32):
        raise ValueError("instance_norm_f32_train takes 4-D fp32 tensors (the bf16 training path is hip.instance_norm)")
    if relu and residual is not None:
        raise NotImplementedError("ReLU after the residual add is not a pattern of the reference")
    if residual is not None and tuple(residual.shape) != tuple(x.shape):
        raise ValueError(f"residual shape {tuple(residual.shape)} != {tuple(x.shape)}")
    _need_gpu(x, residual)
    return _InstanceNormF32Train.apply(x, residual, bool(relu), float(eps))


class _UpsampleConcatF32Train(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, skip):
        ctx.C = x.shape[1]
        return upsample2x_concat_f32(x, skip)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        C = ctx.C
        g = _f32_grad(g)
        B, _, Ho, Wo = g.shape
        gx = None
        if ctx.needs_input_grad[0]:
            gx = _f32_out(None, B, C, Ho // 2, Wo // 2, g.device)
            vg, vx = _f32_view(g[:, :C], "g"), _f32_view(gx, "gx")
            _lib.check(lib.oess_downsample_sum2x_f32(ctypes.byref(vg), B, Ho // 2, Wo // 2, C, ctypes.byref(vx), _stream()),
                       "oess_downsample_sum2x_f32")
        gskip = g[:, C:] if g.shape[1] > C and ctx.needs_input_grad[1] else None
        return gx, gskip


def upsample2x_concat_f32_train(x, skip=None):
    """Differentiable upsample2x_concat_f32 (K18): the gradient of x is the fixed-order sum of the four pixels it was copied to
    (oess_downsample_sum2x_f32, reading the first C channels of the concat gradient where they lie); the gradient of skip is the
    remaining channel slice of the incoming gradient, a view."""
    if x.dtype != torch.float32 or x.ndim != 4 or (skip is not None and skip.dtype != torch.float32):
        raise ValueError("upsample2x_concat_f32_train takes 4-D fp32 tensors (the bf16 training path is hip.upsample2x_concat)")
    _need_gpu(x, skip)
    return _UpsampleConcatF32Train.apply(x, skip)


# ------------------------------------------------------------------------------------------ K21: fp32 ResNet-50 training
def pack_conv_weight_f32_dgrad_s2(w):
    """Conv2d weight [Cout, Cin, R, R] (R in {1, 3}) -> the operand of oess_conv2d_dgrad_s2_f32 (include/oess.h): four blocks, one
    per tap parity class c = 2 ry + rx holding the taps r = ry + 2 ty, s = rx + 2 tx; block [ceil16(ny nx Cout)][ceil32(Cin)], row
    (ty nx + tx) Cout + co, column ci = w[co][ci][r][s].  The layout does not depend on the padding.  Needs no library."""
    Co, Ci, R, S = w.shape
    if R != S or R not in (1, 3):
        raise ValueError(f"pack_conv_weight_f32_dgrad_s2 takes 1 x 1 and 3 x 3 kernels, not {R} x {S}")
    Cp = (Ci + 31) // 32 * 32
    wf = w.detach().float()
    blocks = []
    for c in range(4):
        sub = wf[:, :, (c >> 1)::2, (c & 1)::2]                       # [Cout, Cin, ny, nx]
        n = sub.shape[2] * sub.shape[3] * Co
        blk = torch.zeros(((n + 15) // 16 * 16, Cp), dtype=torch.float32, device=w.device)
        if n:
            blk[:n, :Ci] = sub.permute(2, 3, 0, 1).reshape(n, Ci)
        blocks.append(blk)
    return torch.cat(blocks, 0).reshape(-1)


def _conv_out_hw(H, W, R, stride, pad, dilation):
    return (H + 2 * pad - dilation * (R - 1) - 1) // stride + 1, (W + 2 * pad - dilation * (R - 1) - 1) // stride + 1


def _dilated_geometry_check(what, R, stride, pad, dilation, H, W):
    if R not in (1, 3, 7) or stride not in (1, 2) or dilation < 1 or (R - 1) * dilation > 127 or pad < 0:
        raise ValueError(f"{what} runs 1 x 1, 3 x 3 and 7 x 7 taps, stride 1 or 2, dilation >= 1 with (R - 1) dilation <= 127, not "
                         f"{R} x {R}, stride {stride}, dilation {dilation}, pad {pad}")
    if min(H, W) + 2 * pad < dilation * (R - 1) + 1:
        raise ValueError(f"{what}: no output for a {H} x {W} map, {R} x {R} taps, pad {pad}, dilation {dilation}")


def conv2d_dilated_wgrad_f32(x, dy, R, stride, pad, dilation, want_db=True):
    """Weight and bias gradient of y = conv(x, w, stride, pad, dilation) + b in fp32 on the f32-input MFMA
    (oess_conv2d_dilated_wgrad_f32): (dw [Cout, Cin, R, R], db [Cout] or None).  x [B, Cin, H, W], dy [B, Cout, Ho, Wo]: fp32
    tensors with any strides, read where they lie.  R in {1, 3, 7}, stride 1 or 2, any dilation and padding.  At stride 1,
    dilation 1 and 'same' padding the bits are conv2d_wgrad_f32's.  Fixed summation order: bit-repeatable."""
    for name, t in (("x", x), ("dy", dy)):
        if t.dtype != torch.float32 or t.ndim != 4:
            raise ValueError(f"conv2d_dilated_wgrad_f32: {name} must be a 4-D fp32 tensor [B, C, H, W]")
    B, _, H, W = x.shape
    _dilated_geometry_check("conv2d_dilated_wgrad_f32", R, stride, pad, dilation, H, W)
    if (dy.shape[0], dy.shape[2], dy.shape[3]) != (B,) + _conv_out_hw(H, W, R, stride, pad, dilation):
        raise ValueError(f"conv2d_dilated_wgrad_f32: dy {tuple(dy.shape)} is not the output of x {tuple(x.shape)} under {R} x {R}, "
                         f"stride {stride}, pad {pad}, dilation {dilation}")
    return _wgrad_f32_launch("conv2d_dilated_wgrad_f32", x, dy, R, stride, pad, dilation, want_db)


def conv2d_dgrad_s2_f32(dy, packed, Cin, H, W, R, pad, out=None):
    """Data gradient [B, Cin, H, W] of a stride-2, dilation-1 R x R convolution (R in {1, 3}, pad < R) from dy [B, Cout, Ho, Wo]
    in fp32 (oess_conv2d_dgrad_s2_f32): four phase sub-convolutions of dy in one launch; every element is written once, a pixel no
    window reads gets 0.0.  `packed` from pack_conv_weight_f32_dgrad_s2.  Returns out (channels_last if new)."""
    lib = _lib.load()
    if dy.dtype != torch.float32 or dy.ndim != 4:
        raise ValueError("conv2d_dgrad_s2_f32: dy must be a 4-D fp32 tensor [B, Cout, Ho, Wo]")
    B, Cout, Ho, Wo = dy.shape
    if R not in (1, 3) or not 0 <= pad < R or min(H, W) + 2 * pad < R or (Ho, Wo) != _conv_out_hw(H, W, R, 2, pad, 1):
        raise ValueError(f"conv2d_dgrad_s2_f32: dy {tuple(dy.shape)} is not the output of a {H} x {W} map under {R} x {R}, stride 2, "
                         f"pad {pad}")
    _need_gpu(dy, packed, out)
    need = lib.oess_conv2d_dgrad_s2_f32_packed_floats(Cout, Cin, R)
    if packed.dtype != torch.float32 or not packed.is_contiguous() or need == 0 or packed.numel() < need:
        raise ValueError(f"packed weight must be a contiguous fp32 tensor of at least {need} floats")
    out = _f32_out(out, B, Cin, H, W, dy.device)
    vg, vo = _f32_view(dy, "dy"), _f32_view(out, "out")
    _lib.check(lib.oess_conv2d_dgrad_s2_f32(ctypes.byref(vg), B, H, W, Cin, _ptr(packed), Cout, R, R, pad, ctypes.byref(vo), _stream()),
               "oess_conv2d_dgrad_s2_f32")
    _bump(out)
    return out


class _Conv2dDilatedF32Train(torch.autograd.Function):
    """conv(x, weight, stride, pad, dilation) + bias in fp32, the one fp32 training convolution (conv2d_f32_train is its stride 1,
    dilation 1, 'same' padding case): forward hip.conv2d_f32, backward `wgrad` (conv2d_wgrad_f32 or conv2d_dilated_wgrad_f32, as
    the public entry hands over) and, when x needs a gradient, oess_conv2d_dgrad_s2_f32 (stride 2) or the dilated forward on the
    rotated, transposed weight."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, dilation, wgrad, pw, ver):
        Cout, _, R, _ = weight.shape
        op = pw.get_train(weight, bias, ver)
        y = conv2d_f32(x, op.packed, op.bias, Cout, R, R, stride, pad, dilation=dilation)
        ctx.save_for_backward(x, weight)
        ctx.meta = (stride, pad, dilation, wgrad, op, op.key, bias is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        stride, pad, dilation, wgrad, op, key, has_bias = ctx.meta
        Cout, Cin, R, _ = weight.shape
        gy = _f32_grad(gy)
        gx = gw = gb = None
        need_gb = has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or need_gb:
            gw, gb = wgrad(x, gy, R, stride, pad, dilation, want_db=need_gb)
            if not ctx.needs_input_grad[1]:
                gw = None
        if ctx.needs_input_grad[0]:
            same = op.key == key                     # a holder that moved on since the forward is not this node's
            if stride == 2:
                wd = op.dgrad_s2() if same else pack_conv_weight_f32_dgrad_s2(weight)
                gx = conv2d_dgrad_s2_f32(gy, wd, Cin, x.shape[2], x.shape[3], R, pad)
            else:
                wd = op.dgrad() if same else pack_conv_weight_f32_dgrad(weight)
                gx = conv2d_f32(gy, wd, None, Cin, R, R, 1, dilation * (R - 1) - pad, dilation=dilation)
        return gx, gw, gb, None, None, None, None, None, None


def conv2d_dilated_f32_train(x, weight, bias=None, stride=1, pad=0, dilation=1, pw=None, ver=None):
    """Differentiable fp32 convolution for training the dilated ResNet (K21): hip.conv2d_f32(..., dilation=) of x with the
    PARAMETER tensors weight [Cout, Cin, R, R] (R in {1, 3, 7}) and bias, stride 1 or 2, any padding and dilation.  Backward: the
    weight / bias gradient on oess_conv2d_dilated_wgrad_f32; the data gradient, only when x needs one, on oess_conv2d_dgrad_s2_f32
    (stride 2) or on the dilated forward with the operand of pack_conv_weight_f32_dgrad and pad' = dilation (R - 1) - pad
    (stride 1).  Stride 2 with dilation > 1, and the data gradient of a 7 x 7 kernel (the stem reads the image), do not occur in
    ResNet-50 and are refused.  pw: an engine.PackedWeightF32 that keeps the packed operands per weight version.  fp32 in, fp32
    out; everything else raises before any launch."""
    if x.dtype != torch.float32 or weight.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
        raise ValueError("conv2d_dilated_f32_train takes fp32 tensors (the bf16 training path is engine.conv2d_train)")
    if x.ndim != 4 or weight.ndim != 4 or weight.shape[2] != weight.shape[3] or weight.shape[1] != x.shape[1]:
        raise ValueError(f"conv2d_dilated_f32_train: x {tuple(x.shape)} does not fit a weight {tuple(weight.shape)}")
    R = weight.shape[2]
    _dilated_geometry_check("conv2d_dilated_f32_train", R, stride, pad, dilation, x.shape[2], x.shape[3])
    if stride == 2 and dilation != 1:
        raise ValueError("conv2d_dilated_f32_train: stride 2 together with dilation > 1 is not built (no layer of ResNet-50 has it)")
    if x.requires_grad and torch.is_grad_enabled():
        if R == 7:
            raise ValueError("conv2d_dilated_f32_train: the data gradient of a 7 x 7 kernel is not built (the stem reads the image)")
        if (stride == 2 and pad >= R) or (stride == 1 and pad > dilation * (R - 1)):
            raise ValueError(f"conv2d_dilated_f32_train: no data gradient for pad {pad} with {R} x {R} taps, stride {stride}, "
                             f"dilation {dilation}")
    _need_gpu(x, weight, bias)
    if pw is None:
        from . import engine as _engine
        pw = _engine.PackedWeightF32()
    return _Conv2dDilatedF32Train.apply(x, weight, bias, stride, pad, dilation, conv2d_dilated_wgrad_f32, pw, ver)


class _BatchNormF32Train(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, bn, relu, eps):
        out, mean, var = batch_norm_train_f32(x, bn, relu=relu, residual=residual, return_stats=True)
        ctx.save_for_backward(x, out if relu else None, mean, var, gamma)
        ctx.relu, ctx.eps, ctx.has_res = relu, eps, residual is not None
        ctx.has_beta = beta is not None
        return out

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.load()
        x, out, mean, var, gamma = ctx.saved_tensors
        B, C, H, W = x.shape
        gy = _f32_grad(gy)
        need_dx = ctx.needs_input_grad[0]
        need_dg = gamma is not None and ctx.needs_input_grad[1]
        need_db = ctx.has_beta and ctx.needs_input_grad[2]
        need_dr = ctx.has_res and ctx.needs_input_grad[3]
        dx = _f32_out(None, B, C, H, W, x.device) if need_dx else None
        dgb = torch.empty((2, C), dtype=torch.float32, device=x.device) if need_dg or need_db else None
        dres = None
        if need_dr:
            dres = _f32_out(None, B, C, H, W, x.device) if ctx.relu else gy      # without a ReLU: the incoming gradient itself
        if need_dx or dgb is not None or (need_dr and ctx.relu):
            vx, vg = _f32_view(x, "x"), _f32_view(gy, "dy")
            vo = _f32_view(out, "out") if ctx.relu else None
            vd = None if dx is None else _f32_view(dx, "dx")
            vr = _f32_view(dres, "dres") if need_dr and ctx.relu else None
            need = lib.oess_batch_norm_bwd_f32_workspace_bytes(B, H, W, C)
            ws = _workspace(need, x.device, tag="batchnorm_bwd_f32")
            _lib.check(lib.oess_batch_norm_bwd_f32(ctypes.byref(vx), _f32_ref(vo), ctypes.byref(vg), B, H, W, C, _ptr(mean), _ptr(var),
                                                   ctx.eps, _ptr(None if gamma is None else gamma.detach()), int(ctx.relu), _f32_ref(vd),
                                                   _ptr(dgb[1]) if need_dg else None, _ptr(dgb[0]) if need_db else None, _f32_ref(vr),
                                                   _ptr(ws), ws.numel(), _stream()), "oess_batch_norm_bwd_f32")
        return dx, (dgb[1] if need_dg else None), (dgb[0] if need_db else None), dres, None, None, None


def batch_norm_f32_train(x, bn, relu=False, residual=None):
    """Differentiable train-mode nn.BatchNorm2d [+ residual] [+ ReLU] in fp32 (K21), not in place: the forward is
    batch_norm_train_f32's kernels and bits (batch statistics, the running statistics moved one momentum step, the batch counted
    once) and keeps x, the output (the ReLU mask) and the batch mean and variance for oess_batch_norm_bwd_f32, which gives dx,
    dgamma, dbeta and the residual's gradient, each only when asked for (frozen gamma / beta still give dx).  bn: an
    nn.BatchNorm2d in train mode, or batch_norm_train_f32's dict.  An eval-mode BatchNorm folds into its conv: conv_bn_f32."""
    if x.dtype != torch.float32 or x.ndim != 4 or (residual is not None and residual.dtype != torch.float32):
        raise ValueError("batch_norm_f32_train takes 4-D fp32 tensors (the bf16 training path is hip.batch_norm_train)")
    if isinstance(bn, dict):
        gamma, beta, eps, momentum = bn.get('weight'), bn.get('bias'), bn.get('eps', 1e-5), bn.get('momentum', 0.1)
    else:
        if not bn.training:
            raise NotImplementedError("batch_norm_f32_train is the batch-statistics form: an eval-mode BatchNorm folds into its "
                                      "convolution (models._resnet.conv_bn_f32)")
        gamma, beta, eps, momentum = bn.weight, bn.bias, bn.eps, bn.momentum
    if momentum is None:
        raise NotImplementedError("batch_norm_f32_train: momentum=None (cumulative moving average) is not built")
    for name, t in (('weight', gamma), ('bias', beta)):
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"batch_norm_f32_train: {name} must be fp32")
    if residual is not None and tuple(residual.shape) != tuple(x.shape):
        raise ValueError(f"residual shape {tuple(residual.shape)} != {tuple(x.shape)}")
    _need_gpu(x, residual, gamma, beta)
    return _BatchNormF32Train.apply(x, gamma, beta, residual, bn, bool(relu), float(eps))


class _MaxPool3x3s2F32Train(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return max_pool_3x3s2_f32(x)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        B, C, H, W = x.shape
        g = _f32_grad(g)
        dx = _f32_out(None, B, C, H, W, x.device)
        vx, vg, vd = _f32_view(x, "x"), _f32_view(g, "dy"), _f32_view(dx, "dx")
        _lib.check(_lib.load().oess_maxpool3x3s2_bwd_f32(ctypes.byref(vx), ctypes.byref(vg), B, H, W, C, ctypes.byref(vd), _stream()),
                   "oess_maxpool3x3s2_bwd_f32")
        return dx


def max_pool_3x3s2_f32_train(x):
    """Differentiable max_pool_3x3s2_f32 (K21): the backward recomputes each window's winner from x with ATen's rule (first
    maximum in scan order, a NaN wins) and gathers, per input pixel, the gradient of the windows it won
    (oess_maxpool3x3s2_bwd_f32): no index map is kept, every element of the gradient is written once."""
    if x.dtype != torch.float32 or x.ndim != 4:
        raise ValueError("max_pool_3x3s2_f32_train takes a 4-D fp32 tensor (the bf16 training path is hip.max_pool_3x3s2)")
    _need_gpu(x)
    return _MaxPool3x3s2F32Train.apply(x)


# ------------------------------------------------------------------------------------------ K22: fp32 DeepLabv3-R50 training
def _dropout_f32_launch(x, p, seed, offset):
    B, C, H, W = x.shape
    y = _f32_out(None, B, C, H, W, x.device)
    vx, vy = _f32_view(x, "x"), _f32_view(y, "y")
    _lib.check(_lib.load().oess_dropout_f32(ctypes.byref(vx), ctypes.byref(vy), B, H, W, C, p, seed, offset, _stream()), "oess_dropout_f32")
    return y


class _DropoutF32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed, offset):
        ctx.meta = (p, seed, offset)
        return _dropout_f32_launch(x, p, seed, offset)

    @staticmethod
    def backward(ctx, g):
        g = _f32_grad(g)
        return _dropout_f32_launch(g, *ctx.meta), None, None, None


def dropout_f32(x, p, training=True, owner=None):
    """nn.Dropout(p) on a logical [B, C, H, W] fp32 tensor with any strides, C % 8 == 0 (K22, oess_dropout_f32): the Philox mask
    of hip.dropout, element for element, for the same seed, counter and shape, recomputed in the backward pass instead of stored;
    a kept value is x * float32(1 / (1 - p)).  The counter rule is hip.dropout's own (`owner`: the nn.Dropout module), so a model
    that alternates bf16 and fp32 steps walks one mask sequence.  training=False or p <= 0 returns x itself."""
    global _DROPOUT_CALLS
    if not training or p <= 0.0:
        return x
    if x.dtype != torch.float32 or x.ndim != 4 or x.shape[1] % 8:
        raise ValueError("dropout_f32 needs a 4-D fp32 tensor [B, C, H, W] with C % 8 == 0 (the bf16 training path is hip.dropout)")
    if not p < 1.0:
        raise ValueError(f"dropout_f32: p must lie in [0, 1), got {p}")
    _need_gpu(x)
    if owner is not None:
        calls = getattr(owner, "_oess_dropout_calls", 0) + 1
        owner._oess_dropout_calls = calls
        calls += 1 << 40                                         # own sequence: never collides with the process-wide counter
    else:
        _DROPOUT_CALLS += 1
        calls = _DROPOUT_CALLS
    return _DropoutF32.apply(x, float(p), int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF, calls)


def _avg_pool_rows_f32(x):
    """per-sample channel means of a logical [B, C, H, W] fp32 view -> dense fp32 [B, C] (oess_global_avg_pool_fwd_f32)"""
    lib = _lib.load()
    B, C, H, W = x.shape
    need = lib.oess_global_avg_pool_f32_workspace_bytes(B, H, W, C)
    if need == 0:
        raise ValueError(f"aspp_pool_branch_f32: no pooling kernel for a {(B, C, H, W)} map")
    ws = _workspace(need, x.device, tag="avgpool_f32")
    out = torch.empty((B, C), dtype=torch.float32, device=x.device)
    vx = _f32_view(x, "x")
    _lib.check(lib.oess_global_avg_pool_fwd_f32(ctypes.byref(vx), B, H, W, C, _ptr(out), _ptr(ws), ws.numel(), _stream()),
               "oess_global_avg_pool_fwd_f32")
    return out


class _ASPPPoolBranchF32(torch.autograd.Function):
    """ASPPPooling (models/deeplabv3.py:305-316 of the reference) in fp32 as one node: AdaptiveAvgPool2d(1) -> 1x1 conv ->
    BatchNorm2d(train) over the B pooled vectors -> ReLU -> the 1x1 map broadcast over H x W (bilinear from 1x1 == broadcast)."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, run_mean, run_var, momentum, eps):
        lib = _lib.load()
        B, C, H, W = x.shape
        Cout = weight.shape[0]
        pooled = _avg_pool_rows_f32(x)                          # the means: in_scale = 1 in both directions
        w2 = weight.detach().reshape(Cout, C)
        if not w2.is_contiguous():
            w2 = w2.contiguous()
        buf = torch.empty((2 * B + 2, Cout), dtype=torch.float32, device=x.device)      # y_pre | z | mean, rstd
        y_pre, z, stat = buf[:B], buf[B:2 * B], buf[2 * B:]
        _lib.check(lib.oess_aspp_pool_fwd_f32(_ptr(pooled), 1.0, _ptr(w2), _ptr(gamma.detach()), _ptr(beta.detach()), _ptr(run_mean),
                                              _ptr(run_var), float(momentum), float(eps), B, C, Cout, _ptr(y_pre), _ptr(stat), _ptr(z),
                                              None, _stream()), "oess_aspp_pool_fwd_f32")
        _bump(run_mean)
        _bump(run_var)
        ctx.save_for_backward(pooled, w2, gamma.detach(), buf)
        ctx.geom = (B, H, W, C, Cout)
        return z.clone().view(B, Cout, 1, 1).expand(B, Cout, H, W)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        pooled, w2, gamma, buf = ctx.saved_tensors
        B, H, W, C, Cout = ctx.geom
        y_pre, z, stat = buf[:B], buf[B:2 * B], buf[2 * B:]
        g = _f32_grad(g)
        gz = _avg_pool_rows_f32(g) * float(H * W)               # per-sample sums of the gradient slice, read where it lies
        out = torch.empty((B * Cout + Cout * C + 2 * Cout,), dtype=torch.float32, device=g.device)
        dy = out[:B * Cout]
        gw = out[B * Cout:B * Cout + Cout * C].view(Cout, C, 1, 1)
        gg = out[B * Cout + Cout * C:B * Cout + Cout * C + Cout]
        gb = out[B * Cout + Cout * C + Cout:]
        gp = torch.empty((B, C), dtype=torch.float32, device=g.device) if ctx.needs_input_grad[0] else None
        if any(ctx.needs_input_grad[:4]):
            _lib.check(lib.oess_aspp_pool_bwd_f32o(_ptr(gz), _ptr(pooled), 1.0, _ptr(w2), _ptr(gamma), _ptr(y_pre), _ptr(stat), _ptr(z),
                                                   B, C, Cout, _ptr(dy), _ptr(gw), _ptr(gg), _ptr(gb), _ptr(gp), _stream()),
                       "oess_aspp_pool_bwd_f32o")
        gx = None
        if gp is not None:                                      # d mean / d x = 1 / (H W): the quotient, expanded with stride 0
            gx = (gp * (1.0 / (H * W))).view(B, C, 1, 1).expand(B, C, H, W)
        need = ctx.needs_input_grad
        return gx, (gw if need[1] else None), (gg if need[2] else None), (gb if need[3] else None), None, None, None, None


def aspp_pool_branch_f32(x, conv, bn):
    """ASPPPooling.forward in fp32 for a TRAIN-mode BatchNorm (K22), one autograd node: x logical [B, Cin, H, W] fp32 with any
    strides -> the [B, Cout, 1, 1] row expanded with stride 0 over H x W.  Forward: oess_global_avg_pool_fwd_f32, then
    oess_aspp_pool_fwd_f32 (B-row GEMV, BatchNorm over the B pooled vectors, ReLU, the running statistics moved one step, the batch
    counted).  Backward: the per-sample sums of the incoming gradient by the same pooling kernel, oess_aspp_pool_bwd_f32o, and dx as
    the [B, Cin, 1, 1] quotient expanded with stride 0.  2 <= B <= 16, Cin % 4 == 0; everything else raises before any launch."""
    if x.dtype != torch.float32 or x.ndim != 4:
        raise ValueError("aspp_pool_branch_f32 takes a 4-D fp32 tensor (the bf16 training path is hip.aspp_pool_branch)")
    B, Cin = x.shape[0], x.shape[1]
    if not 2 <= B <= 16:
        raise ValueError(f"aspp_pool_branch_f32 needs 2 <= B <= 16 samples (BatchNorm over the B pooled vectors), got {B}")
    if Cin % 4:
        raise ValueError(f"aspp_pool_branch_f32 needs Cin % 4 == 0, got {Cin}")
    if not bn.training:
        raise NotImplementedError("aspp_pool_branch_f32 is the batch-statistics form: an eval-mode BatchNorm folds (conv_bn_f32)")
    if bn.momentum is None or bn.running_mean is None or bn.weight is None:
        raise NotImplementedError("aspp_pool_branch_f32 needs an affine BatchNorm with running statistics and a momentum")
    w = conv.weight
    if w.dtype != torch.float32 or tuple(w.shape[1:]) != (Cin, 1, 1) or conv.bias is not None or bn.weight.dtype != torch.float32:
        raise ValueError(f"aspp_pool_branch_f32: a bias-free fp32 1 x 1 conv over {Cin} channels is needed, got {tuple(w.shape)}")
    _need_gpu(x, w, bn.weight, bn.running_mean)
    from . import engine as _engine
    y = _ASPPPoolBranchF32.apply(x, w, bn.weight, bn.bias, bn.running_mean, bn.running_var, float(bn.momentum), float(bn.eps))
    _engine.bump_bn_counter(bn)
    return y


# ------------------------------------------------------------------------------------------ K24: SLIC superpixels
SLIC_MAX_CENTERS = 256


def slic_lattice(H, W, n_segments):
    """Centre lattice of hip.slic_superpixels, a pure host function: (ny, nx, step) with s = sqrt(H W / n_segments),
    ny = max(1, floor(H / s)), nx = max(1, floor(W / s)) and step = max(ceil(H / ny), ceil(W / nx)).  K = ny nx <= n_segments
    whenever s <= min(H, W); 440 x 640 with n = 100 gives 8 x 12 = 96 centres and step 55."""
    import math
    H, W, n_segments = int(H), int(W), int(n_segments)
    if H < 1 or W < 1 or n_segments < 1:
        raise ValueError(f"slic_lattice needs H, W, n_segments >= 1, got {(H, W, n_segments)}")
    s = math.sqrt(H * W / n_segments)
    ny, nx = max(1, int(math.floor(H / s))), max(1, int(math.floor(W / s)))
    return ny, nx, max(-(-H // ny), -(-W // nx))


def _slic_blur_radius(sigma):
    return int(4.0 * float(sigma) + 0.5)


def _slic_check_lab(lab, what="lab"):
    if not torch.is_tensor(lab) or lab.dtype != torch.float32 or lab.ndim != 4 or lab.shape[-1] != 3 or not lab.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 tensor [B, H, W, 3]")
    B, H, W, _ = lab.shape
    if B < 1 or H * W < 1 or H * W > (1 << 24):
        raise ValueError(f"{what}: B >= 1 and 1 <= H W <= 2^24 are needed, got {tuple(lab.shape)}")
    return B, H, W


def _slic_check_centers(centers, B, what="centers"):
    if not torch.is_tensor(centers) or centers.dtype != torch.float32 or centers.ndim != 3 or centers.shape[0] != B \
            or centers.shape[2] != 5 or not centers.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 tensor [{B}, K, 5] of (y, x, L, a, b)")
    K = centers.shape[1]
    if not 1 <= K <= SLIC_MAX_CENTERS:
        raise ValueError(f"{what}: 1 <= K <= {SLIC_MAX_CENTERS} centres are served, got {K}")
    return K


def _slic_check_labels(labels, B, H, W, what):
    if not torch.is_tensor(labels) or labels.dtype != torch.int64 or tuple(labels.shape) != (B, H, W) or not labels.is_contiguous():
        raise ValueError(f"{what} must be a contiguous int64 tensor {(B, H, W)}")


def slic_lab(frames, sigma=3.0, compactness=6.0, lattice=None):
    """First pass of SLIC (oess_slic_lab_f32): frames, logical [B, 3, H, W] fp32 with any strides (values nominally in [0, 1]) ->
    the blurred CIELAB map scaled by 1 / compactness, contiguous fp32 [B, H, W, 3].  Gaussian of radius int(4 sigma + 0.5), border
    rule reflect.  lattice = (ny, nx): also returns the starting centres [B, ny nx, 5] = (y, x, L, a, b) at the lattice pixels."""
    if not torch.is_tensor(frames) or frames.dtype != torch.float32 or frames.ndim != 4 or frames.shape[1] != 3:
        raise ValueError("frames must be a 4-D float32 tensor [B, 3, H, W]")
    sigma, compactness = float(sigma), float(compactness)
    if not sigma > 0.0 or not sigma <= 6.0:
        raise ValueError(f"slic: 0 < sigma <= 6 is needed, got {sigma}")
    if not compactness > 0.0:
        raise ValueError(f"slic: compactness > 0 is needed, got {compactness}")
    B, _, H, W = frames.shape
    R = _slic_blur_radius(sigma)
    if min(H, W) < R + 1:
        raise ValueError(f"slic: min(H, W) >= {R + 1} is needed (one reflection must cover the blur radius {R}), got {H} x {W}")
    if B < 1 or H * W > (1 << 24):
        raise ValueError(f"slic: B >= 1 and H W <= 2^24 are needed, got {tuple(frames.shape)}")
    ny = nx = 0
    if lattice is not None:
        ny, nx = int(lattice[0]), int(lattice[1])
        if not (1 <= ny <= H and 1 <= nx <= W):
            raise ValueError(f"slic: a {ny} x {nx} lattice does not fit a {H} x {W} frame")
        if ny * nx > SLIC_MAX_CENTERS:
            raise ValueError(f"slic: K = {ny} x {nx} = {ny * nx} centres, at most {SLIC_MAX_CENTERS} are served")
    _need_gpu(frames)
    lib = _lib.load()
    vf = _f32_view(frames, "frames")
    lab = torch.empty((B, H, W, 3), dtype=torch.float32, device=frames.device)
    centers = torch.empty((B, ny * nx, 5), dtype=torch.float32, device=frames.device) if lattice is not None else None
    _lib.check(lib.oess_slic_lab_f32(ctypes.byref(vf), B, H, W, sigma, compactness, _ptr(lab), ny, nx, _ptr(centers), _stream()),
               "oess_slic_lab_f32")
    return lab if lattice is None else (lab, centers)


def slic_assign(lab, centers, prev_labels, step, lattice=None, out=None):
    """One assignment pass of SLIC (oess_slic_assign_f32): lab [B, H, W, 3] and centers [B, K, 5] fp32, prev_labels int64
    [B, H, W] -> int64 labels [B, H, W].  A pixel is eligible for the centres within 2 step of it (the rule of include/oess.h),
    the lowest distance wins, ties go to the lowest k and a pixel eligible for none keeps its previous label.  prev_labels None
    with lattice = (ny, nx), ny nx = K: every pixel starts with the index of its lattice cell.  out may be prev_labels."""
    B, H, W = _slic_check_lab(lab)
    K = _slic_check_centers(centers, B)
    step = int(step)
    if step < 1:
        raise ValueError(f"slic_assign: step >= 1 is needed, got {step}")
    ny = nx = 0
    if prev_labels is None:
        if lattice is None or int(lattice[0]) * int(lattice[1]) != K or min(int(lattice[0]), int(lattice[1])) < 1:
            raise ValueError(f"slic_assign: without prev_labels a lattice (ny, nx) with ny nx = K = {K} is needed, got {lattice}")
        ny, nx = int(lattice[0]), int(lattice[1])
    else:
        _slic_check_labels(prev_labels, B, H, W, "prev_labels")
    if out is not None:
        _slic_check_labels(out, B, H, W, "out")
    _need_gpu(lab, centers, prev_labels, out)
    lib = _lib.load()
    if out is None:
        out = torch.empty((B, H, W), dtype=torch.int64, device=lab.device)
    _lib.check(lib.oess_slic_assign_f32(_ptr(lab), _ptr(centers), _ptr(prev_labels), B, H, W, K, step, ny, nx, _ptr(out), _stream()),
               "oess_slic_assign_f32")
    _bump(out)
    return out


def slic_update(lab, labels, centers, out=None, return_counts=False):
    """One update pass of SLIC (oess_slic_update_f32): each centre becomes the mean (y, x, L, a, b) of its pixels, an empty centre
    stays.  Integer and 2^-32 fixed-point sums (no floating-point atomics): bit-repeatable; a position is
    the float64 quotient of an exact integer sum and the count, rounded to fp32.  Returns new centres [B, K, 5] (out may be centers), with return_counts also the int32 [B, K] pixel counts."""
    B, H, W = _slic_check_lab(lab)
    K = _slic_check_centers(centers, B)
    _slic_check_labels(labels, B, H, W, "labels")
    if out is not None and _slic_check_centers(out, B, "out") != K:
        raise ValueError(f"out must have the shape of centers {tuple(centers.shape)}")
    _need_gpu(lab, labels, centers, out)
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(centers)
    ws = _workspace(B * K * 48, lab.device, tag="slic")
    counts = torch.empty((B, K), dtype=torch.int32, device=lab.device) if return_counts else None
    _lib.check(lib.oess_slic_update_f32(_ptr(lab), _ptr(labels), _ptr(centers), B, H, W, K, _ptr(out), _ptr(counts), _ptr(ws), ws.numel(),
                                        _stream()), "oess_slic_update_f32")
    _bump(out)
    return (out, counts) if return_counts else out


def slic_connectivity_sizes(H, W, K):
    """skimage's thresholds of the connectivity pass for an H x W map with K placed centres, a pure host function:
    (min_size, max_size, bound) with segment_size = H W / K, min_size = int(0.5 segment_size), max_size = int(3 segment_size)
    and bound = H W // max(min_size, 1), the most labels a sample can hold after the pass (every kept component has at least
    min_size pixels): about 2 K.  The GPU pass takes min_size only: a component of max_size pixels or more stays whole
    (skimage cuts it, by a rule that depends on its fill order); max_size is returned so that a caller can tell."""
    H, W, K = int(H), int(W), int(K)
    if H < 1 or W < 1 or K < 1:
        raise ValueError(f"slic_connectivity_sizes needs H, W, K >= 1, got {(H, W, K)}")
    segment = H * W / K
    min_size = int(0.5 * segment)
    return min_size, int(3 * segment), H * W // max(min_size, 1)


def _slic_check_connectivity(labels, min_size, out):
    if not torch.is_tensor(labels) or labels.dtype != torch.int64 or labels.ndim != 3 or not labels.is_contiguous():
        raise ValueError("labels must be a contiguous int64 tensor [B, H, W]")
    B, H, W = labels.shape
    if B < 1 or H * W < 1 or H * W > (1 << 24):
        raise ValueError(f"labels: B >= 1 and 1 <= H W <= 2^24 are needed, got {tuple(labels.shape)}")
    try:
        min_size = None if isinstance(min_size, bool) else operator.index(min_size)
    except TypeError:
        min_size = None
    if min_size is None or not 0 <= min_size <= 0x7fffffff:
        raise ValueError("slic_enforce_connectivity: min_size must be an integer in [0, 2^31)")
    if out is not None:
        _slic_check_labels(out, B, H, W, "out")
        if out.data_ptr() < labels.data_ptr() + labels.numel() * 8 and labels.data_ptr() < out.data_ptr() + out.numel() * 8:
            raise ValueError("slic_enforce_connectivity: out must not alias labels (every pixel reads its neighbours' labels)")
    return B, H, W, min_size


def slic_enforce_connectivity(labels, min_size, out=None, return_counts=False):
    """The connectivity pass of SLIC (oess_slic_connectivity_i64; skimage's enforce_connectivity=True): contiguous int64 labels
    [B, H, W] on the GPU (any values, compared for equality only) -> int64 [B, H, W].  4-connected components of equal labels with
    at least min_size pixels are numbered 0 .. n - 1 by their first pixel in raster order; a smaller one takes the label of the
    last earlier-rooted neighbour its breadth-first walk (right, left, down, up) sees, or 0 without one.  A component of
    max_size pixels or more stays whole: skimage's order-dependent cut is not made, and there is no max_size.
    out must not alias labels.  return_counts: also the int32 [B] number of kept components n (0: the sample is all 0).
    Launches on the current stream, no read-back; two calls give the same bits."""
    B, H, W, min_size = _slic_check_connectivity(labels, min_size, out)
    _need_gpu(labels, out)
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(labels)
    need = lib.oess_slic_connectivity_workspace_bytes(B, H, W)
    ws = _workspace(need, labels.device, tag="slic_connectivity")
    counts = torch.empty((B,), dtype=torch.int32, device=labels.device) if return_counts else None
    _lib.check(lib.oess_slic_connectivity_i64(_ptr(labels), B, H, W, min_size, _ptr(out), _ptr(counts), _ptr(ws), ws.numel(), _stream()),
               "oess_slic_connectivity_i64")
    _bump(out)
    return (out, counts) if return_counts else out


def slic_connectivity_phase_ms(labels, min_size):
    """Milliseconds of the five phases of one hip.slic_enforce_connectivity call (components | flatten + sizes | ranks | donors |
    resolve + write), HIP events between the same launches (oess_slic_connectivity_phase_ms).  Synchronises: a measurement aid."""
    B, H, W, min_size = _slic_check_connectivity(labels, min_size, None)
    _need_gpu(labels)
    lib = _lib.load()
    out = torch.empty_like(labels)
    ws = _workspace(lib.oess_slic_connectivity_workspace_bytes(B, H, W), labels.device, tag="slic_connectivity")
    ms = (ctypes.c_float * 5)()
    _lib.check(lib.oess_slic_connectivity_phase_ms(_ptr(labels), B, H, W, min_size, _ptr(out), _ptr(ws), ws.numel(), ms, _stream()),
               "oess_slic_connectivity_phase_ms")
    return dict(zip(("components", "sizes", "ranks", "donors", "write"), (float(v) for v in ms)))


def slic_superpixels(frames, n_segments, compactness=6.0, sigma=3.0, iters=10, return_centers=False, enforce_connectivity=False):
    """SLIC superpixels of a batch of frames on the GPU (K24; the reference's offline
    skimage.segmentation.slic(img, n_segments, compactness=6, sigma=3.0, start_label=0)):
    frames [B, 3, H, W] fp32 -> int64 labels [B, H, W] in [0, K), K = ny nx of hip.slic_lattice (K <= 256).  Exactly `iters`
    assignment + update rounds on the current stream, no early exit and no read-back; two calls give the same bits.
    enforce_connectivity=False (the default) stops there: skimage's enforce_connectivity=False.  True appends the connectivity
    pass (hip.slic_enforce_connectivity) with min_size of hip.slic_connectivity_sizes(H, W, K), as skimage's default does: the
    labels are then in [0, bound), bound = H W // max(min_size, 1) of that function (about 2 K), numbered by first pixel, and
    no longer index the returned centres.  Unlike skimage a component of max_size pixels or more stays whole."""
    if not torch.is_tensor(frames) or frames.dtype != torch.float32 or frames.ndim != 4 or frames.shape[1] != 3:
        raise ValueError("frames must be a 4-D float32 tensor [B, 3, H, W]")
    iters = int(iters)
    if iters < 1:
        raise ValueError(f"slic_superpixels: iters >= 1 is needed, got {iters}")
    H, W = frames.shape[2], frames.shape[3]
    ny, nx, step = slic_lattice(H, W, n_segments)
    if ny * nx > SLIC_MAX_CENTERS:
        raise ValueError(f"slic: K = {ny} x {nx} = {ny * nx} centres, at most {SLIC_MAX_CENTERS} are served")
    lab, centers = slic_lab(frames, sigma, compactness, lattice=(ny, nx))
    labels = None
    for _ in range(iters):
        labels = slic_assign(lab, centers, labels, step, lattice=(ny, nx), out=labels)
        centers = slic_update(lab, labels, centers, out=centers)
    if enforce_connectivity:
        labels = slic_enforce_connectivity(labels, slic_connectivity_sizes(H, W, ny * nx)[0])
    return (labels, centers) if return_centers else labels
