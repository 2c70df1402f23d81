"""Mirror of e2vid/image_reconstructor.py:ImageReconstructor (:18-123) for the training path:
preprocess -> pad -> recurrent model step -> keep state.  No CudaTimer syncs in the hot loop.
PostProcessor (:126-140) of the offline reconstruction: unsharp mask + intensity rescaling in one HIP pass.
options.precision = 'fp32' runs the whole network in fp32 (UNetRecurrent.forward_fp32), as the reference does: the offline
reconstruction, fp32 validation and (latents_only: head and encoders alone) the frozen front end of an fp32 training step; the
default 'bf16' is the training path's bf16-storage kernels."""
from types import SimpleNamespace

import torch

from .. import hip
from .utils.inference_utils import CropParameters, EventPreprocessor, gkern


class ImageReconstructor:
    def __init__(self, model, height, width, num_bins, device, options=None, augmentation=False, standardization=False):
        options = options if options is not None else SimpleNamespace()
        self.model = model
        self.device = device
        self.height, self.width, self.num_bins = height, width, num_bins
        if augmentation or standardization:
            raise NotImplementedError("augmentation / standardization act on the discarded image output")
        self.no_recurrent = bool(getattr(options, 'no_recurrent', False))
        self.precision = str(getattr(options, 'precision', None) or 'bf16')
        if self.precision not in ('bf16', 'fp32'):
            raise ValueError(f"precision must be 'bf16' or 'fp32', got {self.precision!r}")
        if self.precision == 'fp32':
            unet = getattr(self.model, 'unetrecurrent', None)
            if unet is None:
                raise NotImplementedError("precision='fp32' runs recurrent E2VID models (E2VIDRecurrent)")
            unet.check_fp32()
        self.crop = CropParameters(self.width, self.height, self.model.num_encoders)
        self.last_states_for_each_channel = {'grayscale': None}
        self.event_preprocessor = EventPreprocessor(options)
        # skewed schedule of the recurrent encoder (UNetRecurrent._forward_skew) for calls with need_latents=False; False = plain order
        self.skew = not bool(getattr(options, 'no_skew', False))

    def update_reconstruction(self, event_tensor, event_tensor_id=None, stamp=None, channel_slice=None, reconstruct=False, wavefront=None,
                              need_latents=True, latents_only=False):
        """event_tensor: fp32 [B, num_bins, H, W] (reference contract), or -- fused form -- the whole
        [B, C_total, H, W] event tensor plus channel_slice=(c0, cs) so that the slice, the normalisation
        and the NHWC re-layout are one kernel.  Returns (img | None, states, latent): the trainers discard the image
        (`_, _, latent = update_reconstruction(...)`), so it is only computed with `reconstruct=True` (offline
        reconstruction, e2vid/run_reconstruction.py), cropped back from the padded size like the reference's CropParameters.
        need_latents=False: the caller drops this call's latents (all but the last sub-window of a step): latent[1] (the head
        output) is None and is never written to memory (head + encoder-0 conv in one kernel).  With `self.skew` (default) such
        calls also run the recurrent encoder on the skewed schedule: the returned states hold levels 1, 2 one / two sub-windows
        behind until the next call with need_latents=True (or reconstruct=True) drains them -- same results, fewer launches.
        latents_only=True (precision 'fp32', whose step computes the image by default): stop after the encoders; img is None,
        states and latents are the same bits.  The bf16 step already stops there unless reconstruct=True, which contradicts it."""
        from .model.unet import check_states
        check_states(self.last_states_for_each_channel['grayscale'], self.precision)
        if latents_only and reconstruct:
            raise ValueError("latents_only=True asks for no image, reconstruct=True for one")
        if self.precision == 'fp32':
            return self._update_fp32(event_tensor, channel_slice, wavefront, need_latents, latents_only)
        with torch.no_grad():
            if channel_slice is None:
                events = event_tensor.to(self.device).float().contiguous()
                c0, cs = 0, events.shape[1]
            else:
                events, (c0, cs) = event_tensor, channel_slice
            import contextlib
            unet = getattr(self.model, 'unetrecurrent', None)
            if unet is not None and unet.recurrent_block_type != 'convlstm':
                wavefront = None        # a ConvLSTM schedule (K28): everything, the slice kernel included, stays on the current stream
            kw = {} if wavefront is None else {'wavefront': wavefront}
            if not need_latents and not reconstruct:
                kw['need_head'] = False
            if self.skew and wavefront is None and not reconstruct and not self.no_recurrent and events.is_cuda and unet is not None:
                kw['skew'] = True
            if (not need_latents and not reconstruct and not self.crop.needs_pad and unet is not None
                    and unet.events_fusable(events, cs)):
                # EventPreprocessor apply + NHWC8 re-layout + head + encoder-0 conv in ONE kernel, straight from the event tensor
                # (hot-pixel mask and flip ride along: the kernel's patch loader applies them, K32)
                kw['raw'] = (events, c0, cs, not self.event_preprocessor.no_normalize, self.event_preprocessor.pre_for(events))
                x = None
            else:
                first = torch.cuda.stream(wavefront.streams[0]) if wavefront is not None else contextlib.nullcontext()
                with first:                               # EventPreprocessor + re-layout belong to level 0's stream
                    x = self.event_preprocessor.slice_to_nhwc8(events, c0, cs)
                    if self.crop.needs_pad:
                        x = self.crop.pad(x.float()).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            img, states, latent = self.model(x, self.last_states_for_each_channel['grayscale'], reconstruct=reconstruct, **kw)
            self.last_states_for_each_channel['grayscale'] = None if self.no_recurrent else states
        return img, states, latent

    def _update_fp32(self, event_tensor, channel_slice, wavefront, need_latents, latents_only=False):
        """fp32 step: EventPreprocessor (reference contract, fp32 out) -> reflection pad -> UNetRecurrent.forward_fp32.  The image
        is computed (the offline reconstruction) unless latents_only (a training step); the bf16 schedules have no fp32 form and
        are refused."""
        if wavefront is not None:
            raise ValueError("precision='fp32': the wavefront schedule (one HIP stream per level) is a bf16-path option")
        if not need_latents:
            raise ValueError("precision='fp32': need_latents=False (fused head / skewed schedule) is a bf16-path option")
        with torch.no_grad():
            if channel_slice is None:
                events = event_tensor.to(self.device).float().contiguous()
                x = self.event_preprocessor(events)
            else:
                (c0, cs) = channel_slice
                pre = self.event_preprocessor.pre_for(event_tensor)
                if pre is not None:          # hot pixels zeroed, H and W mirrored (K32), then the slice's normalisation
                    x = hip.masked_normalize_slice(event_tensor, c0, cs, pre=pre, normalize=not self.event_preprocessor.no_normalize)
                elif self.event_preprocessor.no_normalize:
                    x = event_tensor[:, c0:c0 + cs]
                else:
                    x = hip.masked_normalize_slice(event_tensor, c0, cs)
            if self.crop.needs_pad:
                x = self.crop.pad(x)
            img, states, latent = self.model.forward_fp32(x, self.last_states_for_each_channel['grayscale'],
                                                          reconstruct=not latents_only)
            self.last_states_for_each_channel['grayscale'] = None if self.no_recurrent else states
        return img, states, latent


class PostProcessor:
    """e2vid/image_reconstructor.py:126-140: UnsharpMaskFilter -> IntensityRescaler (-> ImageFilter) on the reconstructed frame,
    fused into oess_e2vid_postprocess_* (one launch with fixed Imin / Imax, two with auto-HDR, no host synchronisation).  Options
    are read with the reference's defaults (e2vid/options/inference_options.py:31-46).  The auto-HDR window lives on the device,
    one per PostProcessor, and persists across calls.  Not implemented: the bilateral filter (cv2.bilateralFilter) and colour."""

    def __init__(self, device, options=None):
        options = options if options is not None else SimpleNamespace()
        self.device = torch.device(device)
        if float(getattr(options, 'bilateral_filter_sigma', 0.0)) > 0:
            raise NotImplementedError("PostProcessor: the bilateral filter (cv2.bilateralFilter) is not implemented")
        if getattr(options, 'color', False):
            raise NotImplementedError("PostProcessor: colour reconstruction is not implemented")
        self.unsharp_mask_amount = float(getattr(options, 'unsharp_mask_amount', 0.3))
        self.unsharp_mask_sigma = float(getattr(options, 'unsharp_mask_sigma', 1.0))
        self.gaussian_kernel = gkern(5, self.unsharp_mask_sigma)            # fp32 [5, 5], kept on the host: the launch reads it there
        self.auto_hdr = bool(getattr(options, 'auto_hdr', False))
        self.auto_hdr_median_filter_size = int(getattr(options, 'auto_hdr_median_filter_size', 10))
        self.Imin = float(getattr(options, 'Imin', 0.0))
        self.Imax = float(getattr(options, 'Imax', 1.0))
        if self.auto_hdr:
            self.hdr_state = hip.E2VIDHdrState(self.auto_hdr_median_filter_size, self.device)
        else:
            self.hdr_state = None
            if not self.Imax > self.Imin:
                raise ValueError(f"PostProcessor: Imax ({self.Imax}) must exceed Imin ({self.Imin})")

    def _run(self, frame, want_f32):
        kw = {'hdr_state': self.hdr_state} if self.auto_hdr else {'bounds': (self.Imin, self.Imax)}
        with torch.no_grad():
            return hip.e2vid_postprocess(frame, self.gaussian_kernel, self.unsharp_mask_amount, want_f32=want_f32, **kw)

    def process(self, new_predicted_frame):
        """fp32 [N, 1, H, W] on the device -> fp32 [N, 1, H, W] = uint8 / 255 (the reference contract)."""
        return self._run(new_predicted_frame, True)[1]

    def process_u8(self, new_predicted_frame):
        """Same, returning the uint8 [N, H, W] grey levels that the PNG writer stores."""
        return self._run(new_predicted_frame, False)[0]

    def current_bounds(self):
        """(Imin, Imax) used by the last call (auto-HDR: the medians on the device, read back -- this synchronises)."""
        return self.hdr_state.bounds() if self.auto_hdr else (self.Imin, self.Imax)
