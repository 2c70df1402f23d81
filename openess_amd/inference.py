"""Inference: a trained stage-2/3 checkpoint on a batch or a recording -> label map, confidence and a colour
image.  `Segmenter` builds the networks exactly as the fine-tune / linear-probe trainer does (train.build_trainer, so the
pretrained paths, text_classes, ConvGRU front ends and the precision keys behave as in training), loads a checkpoint written by the
trainers' saver, puts every module in eval mode and renders the logits on hip.segment_render:

  event students (frame2voxel, recon2voxel)   E2VID encoder over the sub-windows -> SemSegE2VID logits -> the same-size render
  frame2recon                                 deeplabv3_resnet50.logits_at_stride -> the upsampling render (nothing of the full
                                              resolution but the outputs is formed); with a linear probe, the full-resolution logits
                                              and the same-size render

An open vocabulary: set_vocabulary / set_vocabulary_embeddings replace the classes at run time -- K classes over
P >= K names, a class's value the maximum over its names.  The event students then go head_features -> hip.vocab_render (head and
render in one pass; above its LDS budget the head conv on the composed operator -> the grouped hip.segment_render), frame2recon
goes logits_at_stride(text_embeddings=T) -> the grouped upsampling render; reset_vocabulary returns to the checkpoint's classes.

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


EMBED_DIM = 512                                 # CLIP ViT-B/16's text width, the width of both students' classifiers
MAX_CLASSES, MAX_NAMES = 255, 1024              # the render kernels' limits (include/oess.h)


def voc_palette(K):
    """uint8 [K, 3] numpy: the PASCAL-VOC colour map (class id bits reversed into the three channels); colour 0 is black"""
    import numpy as np
    pal = np.zeros((K, 3), np.uint8)
    for i in range(K):
        c = i
        for j in range(8):
            for ch in range(3):
                pal[i, ch] |= ((c >> ch) & 1) << (7 - j)
            c >>= 3
    return pal


def check_class_offsets(class_offsets, P):
    """list of K + 1 ints of a list / tensor of offsets over P names: 0 first, strictly increasing, P last, K <= 255"""
    offs = [int(o) for o in (class_offsets.tolist() if torch.is_tensor(class_offsets) else class_offsets)]
    if len(offs) < 2 or offs[0] != 0 or offs[-1] != P or any(b <= a for a, b in zip(offs, offs[1:])):
        raise ValueError(f"class_offsets must start at 0, increase strictly and end at the number of names {P}, got {offs!r}")
    if len(offs) - 1 > MAX_CLASSES:
        raise ValueError(f"a vocabulary holds at most {MAX_CLASSES} classes (labels are bytes, 255 is the ignore label), got {len(offs) - 1}")
    return offs


def tta_views(flip=False, scales=(1.0,)):
    """The views of flip / multi-scale inference as [(scale, mirrored)]: scale 1.0 first, then the other scales
    in the order given, each followed by its mirrored copy when `flip` is set.  Scale 1.0 unflipped is always view 0 (its logits
    are the plain path's).  Refused: scales that are not finite positive numbers, repeat or lack 1.0, and more than 8 views."""
    try:
        scales = [float(v) for v in scales]
    except (TypeError, ValueError):
        raise ValueError(f"scales must be a sequence of numbers, got {scales!r}") from None
    if not scales or any(not (math.isfinite(v) and v > 0.0) for v in scales):
        raise ValueError(f"scales must be finite and positive, got {scales!r}")
    if len(set(scales)) != len(scales) or 1.0 not in scales:
        raise ValueError(f"scales must hold 1.0 (view 0 is the plain prediction) and no scale twice, got {scales!r}")
    views = [(v, m) for v in [1.0] + [v for v in scales if v != 1.0] for m in ((False, True) if flip else (False,))]
    if len(views) > hip.RENDER_MAX_VIEWS:
        raise ValueError(f"flip / multi-scale inference takes at most {hip.RENDER_MAX_VIEWS} views, got {len(views)} "
                         f"({len(scales)} scales{' x 2 for the flip' if flip else ''})")
    return views


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
        self._own = (self.num_classes, self.palette)          # the checkpoint's vocabulary, for reset_vocabulary()
        self._vocab = None                       # the run-time vocabulary (set_vocabulary_embeddings), None: the checkpoint's own
        self._states = None                      # recurrent states of the stateful path
        self._mirror_states = None               # the same for the mirrored recording of predict_events(flip=True)
        self.render_events = None                # (start, end) HIP events around the last render, for the CLI's timing
        self._rec = self._post = None
        if self.is_event:
            H, W = math.ceil(s.img_size_b[0] / 8.0) * 8, math.ceil(s.img_size_b[1] / 8.0) * 8
            opts = SimpleNamespace(**dict(vars(s.e2vid_config), precision=precision))
            if precision == 'fp32':
                self.trainer.models_dict['back_end'].check_fp32()
            self._rec = ImageReconstructor(self.trainer.models_dict['front_sensor_b'], H, W, s.nr_temporal_bins_b, self.device, opts)

    def _render(self, logits, fn=None, **kw):
        """hip.segment_render (or fn: hip.vocab_render) between two timing events, with this object's palette and ignore label"""
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = (fn or hip.segment_render)(logits, palette=self.palette, ignore_label=self.ignore_label, **kw)
        end.record()
        self.render_events = (start, end)
        return out

    def _render_views(self, views, flips, **kw):
        """hip.ensemble_render of the views' logits between two timing events, with this object's palette and ignore label"""
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = hip.ensemble_render(views, flips=flips, palette=self.palette, ignore_label=self.ignore_label, **kw)
        end.record()
        self.render_events = (start, end)
        return out

    def _refuse_vocabulary_tta(self):
        if self._vocab is not None:
            raise ValueError("flip / multi-scale inference under a run-time vocabulary is a follow-up (the ensemble render "
                             "kernel takes no grouped classes): call reset_vocabulary(), or predict without flip / scales")

    # ---------------------------------------------------------------------------------------------------------------- vocabulary
    def _classifier(self):
        return self.trainer.models_dict['back_end' if self.is_event else 'model_recon']

    def _refuse_probe(self):
        if getattr(self._classifier(), 'if_linear_probing', False):
            raise ValueError("a linear-probe checkpoint keeps its vocabulary: the probe's K x K conv is tied to the trained classes")

    def set_vocabulary_embeddings(self, T, class_offsets=None, names=None, palette=None):
        """Classify into the vocabulary of the text embeddings T: float [P, 512] unit rows, one per NAME.  class_offsets: K + 1
        offsets grouping the names into K classes (contiguous groups; None: one name per class); a class's value is the maximum
        over its names.  names: K lists of names (kept for `vocabulary`); palette: uint8 [K, 3] (None: voc_palette(K)).
        num_classes and palette follow.  Refused before any launch: a linear-probe checkpoint, a width other than 512, more than
        255 classes or 1024 names, an ignore label that would be a class."""
        import numpy as np
        self._refuse_probe()
        if not torch.is_tensor(T) or T.ndim != 2 or not T.is_floating_point() or T.shape[0] < 1:
            raise ValueError("text embeddings must be a float [P, 512] tensor, one row per name")
        P = int(T.shape[0])
        if T.shape[1] != EMBED_DIM:
            raise ValueError(f"the classifiers multiply with embeddings of width {EMBED_DIM}, got width {T.shape[1]}")
        if P > MAX_NAMES:
            raise ValueError(f"a vocabulary holds at most {MAX_NAMES} names, got {P}")
        offs = check_class_offsets(range(P + 1) if class_offsets is None else class_offsets, P)
        K = len(offs) - 1
        if K > self.ignore_label:
            raise ValueError(f"{K} classes: the settings' ignore label {self.ignore_label} would be a class")
        if names is not None:
            names = [[n] if isinstance(n, str) else list(n) for n in names]
            if len(names) != K:
                raise ValueError(f"names must hold one entry per class ({K}), got {len(names)}")
        if palette is None:
            palette = voc_palette(K)
        pal = torch.as_tensor(np.asarray(palette.cpu() if torch.is_tensor(palette) else palette))
        if pal.dtype != torch.uint8 or tuple(pal.shape) != (K, 3):
            raise ValueError(f"palette must be uint8 [{K}, 3], got {pal.dtype} {tuple(pal.shape)}")
        v = SimpleNamespace(T=T.detach().to(self.device, torch.float32).contiguous(), offsets=offs, K=K, P=P, names=names,
                            grouped=P != K, weight=None, bias=None, fused=False, pw=None)
        if self.is_event:
            back = self._classifier()
            v.weight, v.bias = back.compose_vocabulary(v.T)
            v.fused = P <= hip.vocab_render_max_names(v.weight.shape[1])
            if not v.fused:                       # the weights exceed vocab_render's LDS budget: the head as a conv of its own
                from . import engine
                w4 = v.weight[:, :, None, None]
                v.pw = (engine.PackedWeightF32().get(w4, v.bias) if self.precision == 'fp32'
                        else engine.PackedWeight().get(w4, v.bias, None, cin_pad=w4.shape[1]))
        self._vocab = v
        self.num_classes, self.palette = K, pal.to(self.device).contiguous()

    def set_vocabulary(self, classes, merge='max', templates='single', palette=None, clip_text_checkpoint=None, clip_bpe_path=None):
        """Classify into `classes`: a list whose entries are a name or a list of names of one class (clip_text.parse_classes
        reads the `a|b` syntax).  CLIP's text tower (clip_text_checkpoint, clip_bpe_path; default: the settings' keys) embeds
        every name under `templates` ('single', 'none' or a file).  merge='max': one embedding per name, a class's value the
        maximum over its names (what the reference's pseudo-label writer does); merge='mean': one embedding per class, its names
        pooled by CLIP's ensemble (K29's text_classes)."""
        from .models import clip_text
        from .models.clip_tokenizer import CLIPTokenizer
        self._refuse_probe()
        if merge not in ('max', 'mean'):
            raise ValueError(f"merge must be 'max' or 'mean', got {merge!r}")
        ckpt = clip_text_checkpoint or getattr(self.settings, 'clip_text_checkpoint', None)
        bpe = clip_bpe_path or getattr(self.settings, 'clip_bpe_path', None)
        if not ckpt or not bpe:
            raise ValueError("set_vocabulary needs clip_text_checkpoint (CLIP weights) and clip_bpe_path (the BPE merges file), "
                             "as arguments or in the settings file")
        for key, path in (('clip_text_checkpoint', ckpt), ('clip_bpe_path', bpe)):
            if not os.path.isfile(path):
                raise ValueError(f"{key}: file not found: {path}")
        classes = list(classes)
        prompts, name_offsets, class_offsets, names = clip_text.build_vocabulary(classes, clip_text.read_templates(templates))
        if len(names) > MAX_CLASSES:
            raise ValueError(f"a vocabulary holds at most {MAX_CLASSES} classes, got {len(names)}")
        if merge == 'mean':
            T, class_offsets = clip_text.compute_text_embeddings(ckpt, bpe, classes, templates, self.device), None
        else:
            model = clip_text.load_clip_text_checkpoint(ckpt, self.device)
            ids = CLIPTokenizer(bpe).tokenize(prompts, context_length=model.context_length)
            T = model.encode_classes(ids, name_offsets)
        self.set_vocabulary_embeddings(T, class_offsets, names, palette)

    def reset_vocabulary(self):
        """Back to the checkpoint's own vocabulary."""
        self._vocab = None
        self.num_classes, self.palette = self._own

    @property
    def vocabulary(self):
        """[{'id', 'names', 'color'}] of the classes in use (names: None where nobody gave them)"""
        pal = self.palette.cpu().tolist()
        if self._vocab is not None:
            names = self._vocab.names
        else:
            own = getattr(self.settings, 'semseg_class_names', None)
            names = [[str(n)] for n in own] if own is not None and len(own) == self.num_classes else None
        return [{'id': k, 'names': None if names is None else names[k], 'color': pal[k]} for k in range(self.num_classes)]

    # ------------------------------------------------------------------------------------------------------------ event students
    def reset(self):
        """Forget the recording: the next stateful call starts from empty states."""
        self._states = self._mirror_states = None

    def _event_logits(self, event, stateful, want_recon, head_operand=False, mirrored=False):
        """(logits fp32 [B, K, H, W], grey u8 [B, H, W] | None) of fp32 events [B, n * C, H, W]: the sub-windows through the E2VID
        encoder in order (_latents / _latents_fp32 of the trainers, on this object's reconstructor), the decoder on the last.
        head_operand=True: the decoder_scale_4 map [B, 32, H, W] takes the logits' place (a vocabulary's head follows in the render).
        mirrored=True: `event` is the mirrored recording of flip inference; its stateful calls carry a state set of their own."""
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
        states = self._mirror_states if mirrored else self._states
        rec.last_states_for_each_channel = {'grayscale': states if stateful else None}
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
            if head_operand:
                logits = back.head_features(latent, self.precision)
            else:
                logits = (back.forward_fp32(latent) if self.precision == 'fp32' else back(latent))[0][1].float()
            if stateful and mirrored:
                self._mirror_states = rec.last_states_for_each_channel['grayscale']
            elif stateful:
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
        return logits, grey

    def _render_vocabulary(self, x, **kw):
        """The event students under a vocabulary: x is the head's operand [B, 32, H, W]"""
        v = self._vocab
        offs = v.offsets if v.grouped else None
        if v.fused:
            return self._render(x, fn=hip.vocab_render, weight=v.weight, bias=v.bias, class_offsets=offs, **kw)
        if self.precision == 'fp32':
            logits = hip.conv2d_f32(x, v.pw.packed, v.pw.bias, v.P, 1, 1)
        else:
            from . import engine
            logits = engine.conv2d_infer(x, v.pw, v.P, 1, out_f32=True)
        return self._render(logits, class_offsets=v.offsets, **kw)

    @torch.no_grad()
    def predict_events(self, event_tensor, stateful=False, want_recon=False, min_conf=0.0, background=None, alpha=0.5, flip=False,
                       scales=(1.0,)):
        """Event students.  event_tensor: fp32 [B, nr_events_data_b * C, H, W] as the loader's voxelizer produces it.
        stateful=False runs the sub-windows from empty states (what validation does).  stateful=True treats them as the NEXT
        windows of one recording (B = 1): the states carry over from the previous stateful call until reset(); one prediction per
        call.  want_recon=True adds 'recon': the E2VID image of the last sub-window, u8 [B, H, W], through PostProcessor.process_u8
        with the reference's defaults.  background: u8 [B, H, W] to blend under the colours, or 'recon' for that image.
        flip=True: the mean class probability of the tensor and of the tensor mirrored along W, on
        hip.ensemble_render; view 0 is the plain prediction ('recon' and the overlay come from it).  The mirrored recording is
        another recording: stateful calls carry one state set per view, reset() clears both, and a stateful call WITHOUT flip
        drops the mirrored one (it missed a window).  scales other than (1.0,) are refused: the reconstructor is built for one size."""
        if not self.is_event:
            raise ValueError(f"predict_events serves the event students {EVENT_OPTIONS}, not {self.config_option!r}")
        over_recon = isinstance(background, str)
        if over_recon and background != 'recon':
            raise ValueError(f"background must be a uint8 tensor, None or 'recon', got {background!r}")
        views = tta_views(flip, scales)
        if any(scale != 1.0 for scale, _ in views):
            raise ValueError("the event students take flip only: scales other than (1.0,) need a reconstructor per size")
        if len(views) > 1:
            self._refuse_vocabulary_tta()
            crop = self._rec.crop
            if crop.padding_left != crop.padding_right:
                raise ValueError(f"flip inference needs the reconstructor's left and right padding equal, got {crop.padding_left} "
                                 f"and {crop.padding_right}: the mirrored tensor would be padded on the other side")
        elif stateful:
            self._mirror_states = None
        logits, grey = self._event_logits(event_tensor, bool(stateful), bool(want_recon) or over_recon, self._vocab is not None)
        if grey is not None and tuple(grey.shape[1:]) != tuple(logits.shape[2:]):
            raise ValueError("the reconstruction is cropped to the sensor, the logits are at the padded size: no overlay for sizes "
                             "that are not multiples of 8")
        kw = dict(background=grey if over_recon else background, alpha=alpha, min_conf=min_conf)
        if len(views) > 1:
            mirror, _ = self._event_logits(event_tensor.flip(-1), bool(stateful), False, mirrored=True)
            out = self._render_views([logits, mirror], [False, True], **kw)
        else:
            out = (self._render if self._vocab is None else self._render_vocabulary)(logits, **kw)
        if want_recon:
            out['recon'] = grey
        return out

    # ------------------------------------------------------------------------------------------------------------------- batches
    @torch.no_grad()
    def predict(self, batch, min_conf=0.0, background=None, alpha=0.5, flip=False, scales=(1.0,)):
        """{'labels', 'conf', 'rgb'} of a prepared batch of the trainer's loader (events, labels, frame | reconstruction, ...).
        flip / scales: the mean class probability over the views of tta_views(flip, scales) on
        hip.ensemble_render -- the image rescaled to (int(H s + 0.5), int(W s + 0.5)) by hip.bilinear_resize and / or mirrored
        along W, one network pass per view through the plain path's own calls.  The event students take flip only
        (predict_events); a linear probe takes flip only (its logits are at the full resolution: raw views)."""
        if self.is_event:
            return self.predict_events(batch[0], min_conf=min_conf, background=background, alpha=alpha, flip=flip, scales=scales)
        model = self.trainer.models_dict['model_recon']
        kw = dict(background=background, alpha=alpha, min_conf=min_conf)
        views = tta_views(flip, scales)
        if len(views) > 1:
            self._refuse_vocabulary_tta()
            img = batch[2]
            size = tuple(img.shape[-2:])
            flips = [m for _, m in views]
            if model.if_linear_probing:
                if any(scale != 1.0 for scale, _ in views):
                    raise ValueError("a linear probe acts on the full-resolution logits of ONE size: scales other than (1.0,) "
                                     "are refused, flip works")
                mirrored = tuple(batch[:2]) + (img.flip(-1),) + tuple(batch[3:])
                return self._render_views([self.trainer.val_logits(mirrored if m else batch, self.precision) for m in flips],
                                          flips, **kw)
            lows = []
            for scale, m in views:
                x = img if scale == 1.0 else hip.bilinear_resize(img, size=(int(size[0] * scale + 0.5), int(size[1] * scale + 0.5)))
                lows.append(model.logits_at_stride(x.flip(-1) if m else x, self.precision))
            return self._render_views(lows, flips, size=size, **kw)
        if model.if_linear_probing:                           # the probe sits behind the resize: full-resolution logits
            return self._render(self.trainer.val_logits(batch, self.precision), **kw)
        if self._vocab is not None:               # (never with a probe: set_vocabulary_embeddings refuses it)
            v = self._vocab
            low = model.logits_at_stride(batch[2], self.precision, text_embeddings=v.T)
            return self._render(low, size=tuple(batch[2].shape[-2:]), class_offsets=v.offsets if v.grouped else None, **kw)
        return self._render(model.logits_at_stride(batch[2], self.precision), size=tuple(batch[2].shape[-2:]), **kw)
