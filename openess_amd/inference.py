"""Inference: a trained stage-2/3 checkpoint on a batch or a recording -> label map, confidence and a colour
image.  `Segmenter` builds the networks exactly as the fine-tune / linear-probe trainer does (train.build_trainer, so the
pretrained paths, text_classes, ConvGRU front ends and the precision keys behave as in training), loads a checkpoint written by the
trainers' saver, puts every module in eval mode and renders the logits on hip.segment_render:

  event students (frame2voxel, recon2voxel)   E2VID encoder over the sub-windows -> SemSegE2VID logits -> the same-size render
  frame2recon                                 deeplabv3_resnet50.logits_at_stride -> the upsampling render (nothing of the full
                                              resolution but the outputs is formed); with a linear probe, the full-resolution logits
                                              and the same-size render

The event path runs on a reconstructor of the Segmenter's own, in its precision: it shares no recurrent state with the trainer's
steps or validation, and never touches an optimiser."""
import math
import os
import sys
from types import SimpleNamespace

import torch

from . import hip
from .e2vid.image_reconstructor import ImageReconstructor, PostProcessor

EVENT_OPTIONS = ('frame2voxel', 'recon2voxel')
CONFIG_OPTIONS = EVENT_OPTIONS + ('frame2recon',)


def _train_module():
    """train.py at the repository root (build_trainer, seed_everything)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import train
    return train


class Segmenter:
    def __init__(self, settings_file, config_option='frame2voxel', checkpoint=None, precision='bf16', linear_probing=None,
                 ckpt_dir=None):
        """settings_file: a stage-2/3 YAML.  checkpoint: a file of the trainers' saver (None: the weights the trainer builds --
        pretrained paths of the YAML, else seeded).  linear_probing: True / False builds the linear-probe / fine-tune trainer; None
        follows the YAML (fine-tune when it names neither)."""
        from .config.settings import Settings
        if precision not in ('bf16', 'fp32'):
            raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
        if config_option not in CONFIG_OPTIONS:
            raise ValueError(f"config_option must be one of {CONFIG_OPTIONS}, got {config_option!r}")
        train = _train_module()
        train.seed_everything()
        s = Settings(settings_file, generate_log=False)
        s.config_option = config_option
        s.if_supervised_only = False
        if hasattr(s, 'if_pretraining'):
            s.if_pretraining = False
        if linear_probing is None:
            linear_probing = bool(getattr(s, 'if_linear_probing', False)) and not getattr(s, 'if_finetuning', False)
        s.if_finetuning, s.if_linear_probing = not linear_probing, bool(linear_probing)
        # the event networks build their fp32 reconstructor checks under the key; frame2recon's trainer refuses it and needs none
        s.eval_precision = precision if config_option in EVENT_OPTIONS else 'bf16'
        s.train_precision = 'bf16'
        if ckpt_dir is not None:
            s.ckpt_dir = ckpt_dir
        if checkpoint:
            s.resume_training, s.resume_ckpt_file = True, checkpoint
        self.trainer, _ = train.build_trainer(s)
        self.settings, self.precision, self.config_option = s, precision, config_option
        self.device = self.trainer.device
        self.is_event = config_option in EVENT_OPTIONS
        for m in self.trainer.models_dict.values():
            m.eval()
        self.num_classes, self.ignore_label = s.semseg_num_classes, s.semseg_ignore_label
        self.palette = torch.from_numpy(s.semseg_color_map.copy()).to(self.device).contiguous()
        self._states = None                      # recurrent states of the stateful path
        self.render_events = None                # (start, end) HIP events around the last render, for the CLI's timing
        self._rec = self._post = None
        if self.is_event:
            H, W = math.ceil(s.img_size_b[0] / 8.0) * 8, math.ceil(s.img_size_b[1] / 8.0) * 8
            opts = SimpleNamespace(**dict(vars(s.e2vid_config), precision=precision))
            if precision == 'fp32':
                self.trainer.models_dict['back_end'].check_fp32()
            self._rec = ImageReconstructor(self.trainer.models_dict['front_sensor_b'], H, W, s.nr_temporal_bins_b, self.device, opts)

    def _render(self, logits, **kw):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = hip.segment_render(logits, palette=self.palette, ignore_label=self.ignore_label, **kw)
        end.record()
        self.render_events = (start, end)
        return out

    # ------------------------------------------------------------------------------------------------------------ event students
    def reset(self):
        """Forget the recording: the next stateful call starts from empty states."""
        self._states = None

    def _event_logits(self, event, stateful, want_recon):
        """(logits fp32 [B, K, H, W], grey u8 [B, H, W] | None) of fp32 events [B, n * C, H, W]: the sub-windows through the E2VID
        encoder in order (_latents / _latents_fp32 of the trainers, on this object's reconstructor), the decoder on the last."""
        s, rec = self.settings, self._rec
        C = s.input_channels_b
        if (not torch.is_tensor(event) or event.ndim != 4 or event.dtype != torch.float32 or not event.is_cuda
                or event.shape[1] % C or event.shape[1] == 0):
            raise ValueError(f"event tensor must be float32 [B, n * {C}, H, W] on the GPU")
        n = event.shape[1] // C
        if not stateful and n != s.nr_events_data_b:
            raise ValueError(f"a stateless prediction takes nr_events_data_b = {s.nr_events_data_b} sub-windows, got {n}")
        if stateful and event.shape[0] != 1:
            raise ValueError("a stateful prediction follows ONE recording: batch size 1")
        rec.last_states_for_each_channel = {'grayscale': self._states if stateful else None}
        img = latent = None
        try:
            for i in range(n):
                last = i == n - 1
                if self.precision == 'fp32':
                    img, _, latent = rec.update_reconstruction(event, channel_slice=(i * C, C), latents_only=not (last and want_recon))
                else:
                    img, _, latent = rec.update_reconstruction(event, channel_slice=(i * C, C), need_latents=last,
                                                               reconstruct=last and want_recon)
            back = self.trainer.models_dict['back_end']
            logits = (back.forward_fp32(latent) if self.precision == 'fp32' else back(latent))[0][1]
            if stateful:
                self._states = rec.last_states_for_each_channel['grayscale']
        finally:
            rec.last_states_for_each_channel = {'grayscale': None}
        grey = None
        if want_recon:
            if rec.crop.needs_pad:
                img = img[:, :, rec.crop.iy0:rec.crop.iy1, rec.crop.ix0:rec.crop.ix1]
            if self._post is None:
                self._post = PostProcessor(self.device)              # the reference's defaults
            grey = self._post.process_u8(img[:, :1])                 # the crop view goes in as it is, as in run_reconstruction
        return logits.float(), grey

    @torch.no_grad()
    def predict_events(self, event_tensor, stateful=False, want_recon=False, min_conf=0.0, background=None, alpha=0.5):
        """Event students.  event_tensor: fp32 [B, nr_events_data_b * C, H, W] as the loader's voxelizer produces it.
        stateful=False runs the sub-windows from empty states (what validation does).  stateful=True treats them as the NEXT
        windows of one recording (B = 1): the states carry over from the previous stateful call until reset(); one prediction per
        call.  want_recon=True adds 'recon': the E2VID image of the last sub-window, u8 [B, H, W], through PostProcessor.process_u8
        with the reference's defaults.  background: u8 [B, H, W] to blend under the colours, or 'recon' for that image."""
        if not self.is_event:
            raise ValueError(f"predict_events serves the event students {EVENT_OPTIONS}, not {self.config_option!r}")
        over_recon = isinstance(background, str)
        if over_recon and background != 'recon':
            raise ValueError(f"background must be a uint8 tensor, None or 'recon', got {background!r}")
        logits, grey = self._event_logits(event_tensor, bool(stateful), bool(want_recon) or over_recon)
        if grey is not None and tuple(grey.shape[1:]) != tuple(logits.shape[2:]):
            raise ValueError("the reconstruction is cropped to the sensor, the logits are at the padded size: no overlay for sizes "
                             "that are not multiples of 8")
        out = self._render(logits, background=grey if over_recon else background, alpha=alpha, min_conf=min_conf)
        if want_recon:
            out['recon'] = grey
        return out

    # ------------------------------------------------------------------------------------------------------------------- batches
    @torch.no_grad()
    def predict(self, batch, min_conf=0.0, background=None, alpha=0.5):
        """{'labels', 'conf', 'rgb'} of a prepared batch of the trainer's loader (events, labels, frame | reconstruction, ...)."""
        if self.is_event:
            return self.predict_events(batch[0], min_conf=min_conf, background=background, alpha=alpha)
        model = self.trainer.models_dict['model_recon']
        kw = dict(background=background, alpha=alpha, min_conf=min_conf)
        if model.if_linear_probing:                           # the probe sits behind the resize: full-resolution logits
            return self._render(self.trainer.val_logits(batch, self.precision), **kw)
        return self._render(model.logits_at_stride(batch[2], self.precision), size=tuple(batch[2].shape[-2:]), **kw)
