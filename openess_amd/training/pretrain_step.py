"""Stage-1 (pre-training) step of the `frame2voxel` and `frame2recon` options, restated from
training/pretrain_trainer.py: buildModels (:107-208), createOptimizerDict (:211-274), train_step
(:324-361) and task_train_step (:364-534).  This is the self-contained step object used by bench.py,
smoke() and the trainer classes; it owns the models_dict / optimizers_dict with the reference's key names.
"""
import contextlib
import functools
import math
from types import SimpleNamespace

import torch

from .. import hip
from . import pretrained
from ..e2vid.image_reconstructor import ImageReconstructor
from ..e2vid.model.model import E2VID_LIGHTWEIGHT_CONFIG, E2VIDRecurrent
from ..models.deeplabv3 import deeplabv3_resnet50
from ..models.image_model import DilationFeatureExtractor
from ..models.style_networks import SemSegE2VID
from ..utils.loss_functions import NCELoss, TaskLoss
from ..utils.optim import AdamW          # torch.optim.AdamW with its step on the multi-tensor HIP kernel


class _Front:
    """What the frozen half of a step leaves for the trainable half (PretrainStep.front)."""
    __slots__ = ('content', 'teacher_enc', 'teacher_out', 'online_pl', 'streams', 'done')

    def __init__(self):
        self.content = self.teacher_enc = self.teacher_out = self.online_pl = self.streams = self.done = None


def _label_options(init):
    """PretrainStep's keyword-only options of K31, taken off the call before the positional constructor runs -- its
    parameter list is pinned (tests/test_pretrain_precision.py), and these have no place in it:
      online_labels=None      callable frame -> int64 [B, H, W] (maskClipFeatureExtractor.labels: hip.argmax_labels on the
                              stride-level logits); when given, front() calls it in place of online_teacher(frame).argmax(dim=1)
      switchable_train=False  if_switchable_train (pretrain_trainer.py:513-514, :556-557): while epoch_count >= switch_epoch the
      switch_epoch=5          dense-CLIP pseudo-labels are the argmax of the student's own logits; batch[3] and the online teacher
                              (either form) are then unused.  epoch_count starts at 0; the trainer sets it every step.
    and of K32:
      e2vid_options=None      settings.e2vid_config (or any object with these attributes): its hot_pixels_file and flip reach the
                              EventPreprocessor of the frame2voxel front end; nothing else of it is read.
    and of K33 (pretrained weights, training/pretrained.py; every default is the seeded network, no file is looked for):
      e2vid_checkpoint=None   reference-format E2VID checkpoint of the frame2voxel front end: the model is built from the file's
                              own config (it replaces e2vid_config) and its state dict is loaded
      image_weights=None      name of the teacher's self-supervised weights (image_model.IMAGE_WEIGHTS), loaded from
      image_weights_path=None   this file, or from weights/<image_weights>.pt under the working directory
      pretrained_backbone=''  {'model_recon': state_dict} file of the frame2recon student (pre_trained_backbone of the YAML)
      require_pretrained=False  a named file that does not exist: False = one warning, seeded weights; True = FileNotFoundError
      logger=None             where the warnings and the "loaded" lines go (None: the openess_amd.pretrained logger)
    and of K34:
      sam_distillation=False  if_sam_distillation (pretrain_trainer.py:481-482, :519-529): frame2recon adds the cosine distance
                              between the batch's SAM features and the student's upsampled feature (hip.sam_distill_loss) under the
                              key 'sam_distillation_loss'; task_train_step then needs sam_feat.  Refused with frame2voxel."""
    @functools.wraps(init)
    def with_options(self, *args, online_labels=None, switchable_train=False, switch_epoch=5, e2vid_options=None,
                     e2vid_checkpoint=None, image_weights=None, image_weights_path=None, pretrained_backbone='',
                     require_pretrained=False, logger=None, sam_distillation=False, **kwargs):
        self.pretrained_options = SimpleNamespace(e2vid_checkpoint=e2vid_checkpoint, image_weights=image_weights,
                                                  image_weights_path=image_weights_path, pretrained_backbone=pretrained_backbone,
                                                  require=bool(require_pretrained), logger=logger or pretrained._DEFAULT_LOGGER)
        self.e2vid_options = e2vid_options
        self.online_labels = online_labels
        self.switchable_train = bool(switchable_train)
        self.switch_epoch = int(switch_epoch)
        self.epoch_count = 0
        self.sam_distillation = bool(sam_distillation)
        init(self, *args, **kwargs)
    return with_options


def refuse_sam_distillation(config_option, dataset_name=None):
    """What if_sam_distillation cannot run, refused before any model is built (PretrainStep and OpenESSPretrainModel)."""
    if config_option != 'frame2recon':
        raise NotImplementedError(f"if_sam_distillation with config_option {config_option!r}: only frame2recon computes the loss. The "
                                  "reference's trainEpoch reads out[0]['sam_distillation_loss'] (pretrain_trainer.py:300), which its "
                                  "frame2voxel branch never writes: the run ends in a KeyError there")
    if dataset_name is not None and dataset_name != 'DSEC_events':
        raise NotImplementedError(f"if_sam_distillation with dataset {dataset_name!r}: its loader has no SAM feature slot "
                                  "(ddd17_events_loader.py returns six items); only DSEC_events carries sam_feat")


class PretrainStep:
    # frame2voxel + contrastive: the student's 256-channel map is only pooled over superpixels, and the mean commutes with its 1x1
    # convolution (hip.PointwiseFeature); False = materialise the map as the reference does (A/B, tests)
    pooled_student_features = True
    # contrastive: the teacher's upsampled + normalised features are only pooled too -> hip.UpsampledNormalizedFeature (one-pass
    # backward); False = the full-resolution tensor goes through autograd as three separate adjoints
    pooled_teacher_features = True
    # FROZEN FRONT / TRAINABLE BACK.  The teacher's encoder (image_model.py:130-143) and the recurrent E2VID encoder are frozen:
    # nothing in them depends on a weight the optimiser touches.  `front(batch)` runs them on their own HIP streams (teacher on
    # one, E2VID on another: the teacher's BatchNorm-apply passes and short-K 1x1 layers are bound by HBM, the ConvLSTM by the
    # matrix / LDS side) and returns a handle; `task_train_step(batch, front=handle)` is the trainable rest (student decoder /
    # DeepLabv3, teacher head when the contrastive loss trains it, losses).  A loop may therefore enqueue front(batch i+1) BEFORE
    # the back half of batch i (`pipeline_steps`): the frozen front of the next batch then runs under the HBM-bound decoder
    # forward / backward / AdamW of the current one.  Same kernels on the same values in a dependency-respecting order: losses,
    # gradients, weights and the teacher's running statistics are bit-identical to the one-stream order (tests/test_hip_determinism).
    # overlap_teacher = False puts everything on the caller's stream (A/B, per-launch timing without CU sharing).
    overlap_teacher = True
    # if_spatial_contrastive: False -> nothing reads the teacher's output.  True (default) runs the whole forward anyway, as the
    # reference does (pretrain_trainer.py:434); False stops after the encoder, whose BatchNorm updates are the call's only effect.
    run_unused_teacher_head = True

    @_label_options
    def __init__(self, config_option='frame2voxel', num_classes=11, img_size=(440, 640), nr_events_data=20,
                 nr_temporal_bins=5, if_spatial_contrastive=False, if_dense_clip_supervision=True, superpixel_size=100,
                 lr=5e-4, weight_task_loss=1.0, task_loss=('dice', 'cross_entropy'), output_stride=32, device='cuda',
                 e2vid_config=None, text_embeddings=None, seed=1205, online_teacher=None, wavefront=False, precision='bf16'):
        # keyword-only on top of these (see _label_options): online_labels=None, switchable_train=False, switch_epoch=5, e2vid_options=None,
        # e2vid_checkpoint=None, image_weights=None, image_weights_path=None, pretrained_backbone='', require_pretrained=False, logger=None,
        # sam_distillation=False
        # precision: arithmetic of the whole step.  'bf16' (default) builds and runs exactly the bf16 step.  'fp32'
        # is the reference's arithmetic (use_amp: False in every YAML); what it cannot run is refused here, before any model is built
        if precision not in ('bf16', 'fp32'):
            raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
        if precision == 'fp32':
            if config_option != 'frame2voxel':
                raise NotImplementedError(f"precision='fp32' pre-trains frame2voxel, not {config_option!r}: DeepLabv3 has no fp32 "
                                          "backward (train-mode BatchNorm, strided and dilated convolutions)")
            if online_teacher is not None or self.online_labels is not None:
                raise NotImplementedError("precision='fp32' has no online teacher: the MaskCLIP ViT has no fp32 form")
            if wavefront:
                raise NotImplementedError("precision='fp32' has no wavefront schedule: fp32 E2VID runs on one stream "
                                          "(the per-level streams are a bf16-path option)")
            SemSegE2VID.check_fp32_config('concat', 'pooled', train=True)
        if self.sam_distillation:
            refuse_sam_distillation(config_option)
        self.precision = precision
        self.config_option = config_option
        # pretrained weights (K33): every named file is resolved, and what cannot be loaded refused, before any model is built
        po = self.pretrained_options
        e2vid = teacher_file = None
        backbone_file = ''
        if config_option == 'frame2voxel':
            e2vid = pretrained.e2vid_source(po.e2vid_checkpoint, 'e2vid_checkpoint', nr_temporal_bins, precision == 'fp32',
                                            po.require, po.logger)
        elif config_option == 'frame2recon':
            backbone_file = pretrained.backbone_path(po.pretrained_backbone, po.require, po.logger)
        if config_option in ('frame2voxel', 'frame2recon'):
            teacher_file = pretrained.teacher_path(po.image_weights, po.image_weights_path, po.require, po.logger)
        # a frozen MaskCLIP tower as ONLINE teacher: pseudo-labels = argmax of its logits on the frame, computed inside
        # the step, instead of the offline `pl_*_rgb` PNGs (README.md:295).  None = the reference's behaviour (labels from the batch).
        self.online_teacher = online_teacher
        self.device = torch.device(device)
        self.nr_events_data, self.bins = nr_events_data, nr_temporal_bins
        self.if_spatial_contrastive = if_spatial_contrastive
        self.if_dense_clip_supervision = if_dense_clip_supervision
        self.superpixel_size = superpixel_size
        self.weight_task_loss = weight_task_loss
        torch.manual_seed(seed)
        self.models_dict = {}
        if config_option == 'frame2voxel':
            # (a checkpoint brings its own config; construction comes first either way, so the seeded stream that initialises
            # the trainable decoder below is the same with and without a file)
            self.front_end_sensor_b = E2VIDRecurrent(e2vid[0] if e2vid is not None else (e2vid_config or E2VID_LIGHTWEIGHT_CONFIG))
            if e2vid is not None:
                pretrained.load_e2vid(self.front_end_sensor_b, e2vid, po.e2vid_checkpoint, po.logger)
            for p in self.front_end_sensor_b.parameters():
                p.requires_grad = False
            self.front_end_sensor_b.eval()
            self.input_height = math.ceil(img_size[0] / 8.0) * 8
            self.input_width = math.ceil(img_size[1] / 8.0) * 8
            self.models_dict['front_sensor_b'] = self.front_end_sensor_b
            self.task_backend = SemSegE2VID(input_c=256, output_c=num_classes, skip_connect=True, skip_type='concat',
                                            text_embeddings_path='',
                                            materialize_ch256=('pooled' if self.pooled_student_features else True)
                                            if if_spatial_contrastive else False)
            self.models_dict['back_end'] = self.task_backend
        elif config_option == 'frame2recon':
            self.model_recon = deeplabv3_resnet50(num_classes=num_classes, text_embeddings_path='',
                                                  output_stride=output_stride, pretrained_backbone=backbone_file)
            if backbone_file:
                pretrained.report_loaded(po.logger, 'the DeepLabv3 student', backbone_file, self.model_recon.state_dict())
            self.models_dict['model_recon'] = self.model_recon
            # the pooling and the SAM loss read the same stride-level map (hip.UpsampledFeature); autograd sums their gradients
            self.model_recon.lazy_feats = bool(self.pooled_student_features and (if_spatial_contrastive or self.sam_distillation))
        else:
            raise NotImplementedError(config_option)
        if teacher_file is None:
            self.model_frame = DilationFeatureExtractor(image_weights=None)
        else:
            self.model_frame = DilationFeatureExtractor(image_weights=po.image_weights, weights_path=teacher_file)
            pretrained.report_loaded(po.logger, f"the image teacher's {po.image_weights!r} encoder", teacher_file,
                                     self.model_frame.encoder.state_dict())
        self.model_frame.lazy_features = bool(if_spatial_contrastive and self.pooled_teacher_features)
        self.models_dict['model_frame'] = self.model_frame
        if text_embeddings is not None:
            tgt = self.task_backend if config_option == 'frame2voxel' else self.model_recon.classifier
            tgt.text_embeddings.copy_(text_embeddings)
        for m in self.models_dict.values():
            m.to(self.device)
        if config_option == 'frame2voxel':
            # the event-side options of the front end's EventPreprocessor (hot_pixels_file, flip: DESIGN.md K32)
            pre_opts = {k: getattr(self.e2vid_options, k) for k in ('hot_pixels_file', 'flip') if getattr(self.e2vid_options, k, None)}
            self.reconstructor = ImageReconstructor(self.front_end_sensor_b, self.input_height, self.input_width,
                                                    nr_temporal_bins, self.device, SimpleNamespace(**pre_opts) if pre_opts else None)
            # wavefront schedule of the 20 recurrent sub-windows over one HIP stream per ConvLSTM level (e2vid/wavefront.py);
            # `self.wavefront = None` switches back to the single-stream order at any time (same results)
            self.wavefront = None
            if wavefront and self.device.type == 'cuda':
                from ..e2vid.wavefront import EncoderWavefront
                self.wavefront = EncoderWavefront(self.device, self.front_end_sensor_b.num_encoders)
            if precision == 'fp32':
                # a second reconstructor over the SAME frozen model with fp32 states and packed operands of its own (as the
                # stage-2/3 trainers keep one, _supervised.buildModels): nothing the bf16 path reads is shared
                self.task_backend.check_fp32(train=True)
                self.reconstructor_fp32 = ImageReconstructor(self.front_end_sensor_b, self.input_height, self.input_width,
                                                             nr_temporal_bins, self.device, SimpleNamespace(precision='fp32', **pre_opts))
        self.task_loss = TaskLoss(losses=list(task_loss), gamma=2.0, num_classes=num_classes, ignore_index=255)
        self.nce_loss = NCELoss(temperature=0.07)
        # createOptimizerDict (pretrain_trainer.py:225-259)
        params_frame = [p for p in self.model_frame.parameters() if p.requires_grad]
        if config_option == 'frame2voxel':
            params_voxel = [p for p in self.task_backend.parameters() if p.requires_grad]
            params_voxel = [p for p in self.front_end_sensor_b.parameters() if p.requires_grad] + params_voxel
            self.optimizers_dict = {'optimizer_voxel': AdamW(params_voxel, lr=lr),
                                    'optimizer_frame': AdamW(params_frame, lr=lr)}
        else:
            params_recon = [p for p in self.model_recon.parameters() if p.requires_grad]
            self.optimizers_dict = {'optimizer_recon': AdamW(params_recon, lr=lr),
                                    'optimizer_frame': AdamW(params_frame, lr=lr)}

    # ------------------------------------------------------------------ pretrain_trainer.py:364-534
    def _set_modes(self):
        for name, m in self.models_dict.items():
            m.train()
            if name == 'front_sensor_b':
                m.eval()                       # unfrozen_e2vid: False in every pre-training YAML

    @property
    def switched(self):
        """True once the pseudo-labels come from the student's own logits (switchable_train and epoch_count >= switch_epoch)."""
        return self.switchable_train and self.epoch_count >= self.switch_epoch

    def front(self, batch):
        """Frozen half of the step for `batch` (see the class comment): teacher encoder (+ its head when nothing trains it) and,
        for frame2voxel, the 20 recurrent E2VID encoder steps.  Everything is enqueued, nothing is waited for; the handle goes to
        task_train_step(batch, front=handle)."""
        self._set_modes()
        h = _Front()
        frame = batch[2] if self.config_option == 'frame2voxel' else batch[0]
        cuda = self.overlap_teacher and self.device.type == 'cuda' and frame.is_cuda
        main = torch.cuda.current_stream(self.device) if cuda else None
        if cuda:
            if getattr(self, '_front_stream', None) is None:
                # (a higher HIP stream priority for the two front streams was measured: 190.9 / 191.2 vs 190.7 / 191.2 event-frames/s)
                self._front_stream = torch.cuda.Stream(device=self.device)
                self._teacher_stream = torch.cuda.Stream(device=self.device)
            F, T = self._front_stream, self._teacher_stream
            F.wait_stream(main)                  # the batch's tensors and everything queued so far (NOT what the caller enqueues later)
            T.wait_stream(main)
        ctx = (lambda st: torch.cuda.stream(st)) if cuda else (lambda st: contextlib.nullcontext())
        if not self.switched:
            if self.online_labels is not None:
                with ctx(T if cuda else None), torch.no_grad():
                    h.online_pl = self.online_labels(frame)
            elif self.online_teacher is not None:
                with ctx(T if cuda else None), torch.no_grad():
                    h.online_pl = self.online_teacher(frame).argmax(dim=1)
        with ctx(T if cuda else None):
            # the teacher head is trained by the contrastive loss: then it belongs to the back half; otherwise nothing can reach it
            # and the whole forward runs here without autograd bookkeeping (the reference runs it too, pretrain_trainer.py:434,484)
            if self.precision == 'fp32':
                # encode_fp32 / forward_fp32 are no_grad; train-mode BatchNorm moves the running statistics one step as encode does
                if self.if_spatial_contrastive or not self.run_unused_teacher_head:
                    h.teacher_enc = self.model_frame.encode_fp32(frame.float())
                else:
                    h.teacher_out = self.model_frame.forward_fp32(frame.float())
            elif self.if_spatial_contrastive:
                h.teacher_enc = self.model_frame.encode(frame)
            elif self.run_unused_teacher_head:
                with torch.no_grad():
                    h.teacher_out = self.model_frame(frame)
            else:
                # Pixel distillation: nothing reads the teacher's features (pretrain_trainer.py:434 computes them and drops them).
                # What the call leaves behind are the train-mode BatchNorm updates of the ENCODER; the head (1x1 conv, x4 bilinear,
                # L2 normalise: no state) is dead code here exactly like the E2VID decoder whose outputs every caller discards.
                # So is the encoder's own last normalisation pass: want_output=False (h.teacher_enc stays None).
                self.model_frame.encode(frame, want_output=False)
        if self.config_option == 'frame2voxel':
            event = batch[0]
            with ctx(F if cuda else None):
                if self.precision == 'fp32':
                    h.content = self._latents_fp32(event)
                else:
                    wf = getattr(self, 'wavefront', None)
                    if wf is not None:
                        wf.begin()
                    self.reconstructor.last_states_for_each_channel = {'grayscale': None}
                    for i in range(self.nr_events_data):
                        _, _, latent_real = self.reconstructor.update_reconstruction(
                            event, channel_slice=(i * self.bins, self.bins), wavefront=wf,
                            need_latents=(i == self.nr_events_data - 1))      # only the last sub-window's latents are used (:437-441)
                    if wf is not None:
                        wf.end(*latent_real.values())
                    self.reconstructor.last_states_for_each_channel = {'grayscale': None}    # the sequence ends with the step
                    h.content = {k: v.detach() for k, v in latent_real.items()}              # trainTaskStepPretrain (:550-562)
        if cuda:
            h.streams = (F, T)
            h.done = (torch.cuda.Event(), torch.cuda.Event())
            h.done[0].record(F)
            h.done[1].record(T)
        return h

    def _latents_fp32(self, event):
        """Detached fp32 latents of the last sub-window from the encoder-only fp32 E2VID step.  They are views of the sequence's
        own cat(x, h) state buffers: every call starts from empty states, so it allocates them, and it drops the states before it
        returns -- the views saved by the decoder's conv backward of batch i cannot be reached by front(batch i + 1)."""
        rec = self.reconstructor_fp32
        rec.last_states_for_each_channel = {'grayscale': None}
        for i in range(self.nr_events_data):
            _, _, latent = rec.update_reconstruction(event, channel_slice=(i * self.bins, self.bins), latents_only=True)
        rec.last_states_for_each_channel = {'grayscale': None}
        return {k: v.detach() for k, v in latent.items()}

    def _join_front(self, h):
        """The current stream continues after the front half; tensors allocated on the front streams are handed to it."""
        if h.streams is None:
            return
        main = torch.cuda.current_stream(self.device)
        for e in h.done:
            main.wait_event(e)
        live = [h.teacher_enc, h.teacher_out, getattr(h.teacher_out, 'x', None), h.online_pl] + list((h.content or {}).values())
        for t in live:
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(main)
        h.streams = None

    def pipeline_steps(self, batches, back):
        """Software pipeline over an iterable of device batches: front(batch i+1) is enqueued before `back(batch i, front i)` runs,
        so the frozen half of the next batch executes under the trainable half of the current one.  `back` is the caller's step
        body (zero_grad, task_train_step(batch, front=...), backward, optimiser); yields its results in batch order."""
        prev = None
        for batch in batches:
            fr = self.front(batch)
            if prev is not None:
                yield back(*prev)
            prev = (batch, fr)
        if prev is not None:
            yield back(*prev)

    def _pool(self, feat, superpixels, S):
        return hip.superpixel_pool(feat, superpixels, self.superpixel_size, S=S)

    def task_train_step(self, batch, front=None, sam_feat=None):
        """batch: (event | frame, label, frame | recon, pl, superpixels) already on the device.
        `superpixel_rows` (optional 6th item) = max offset id + 1 computed by the loader on the host.
        front: the handle of front(batch) when the caller pipelines the steps; None = the frozen half is enqueued here.
        sam_feat: [B, 256, hs, ws] fp32 on the device, the batch's SAM features; read (and required) with sam_distillation only."""
        if self.sam_distillation and sam_feat is None:
            raise ValueError("sam_distillation=True: task_train_step needs sam_feat (slot 5 of the prepared batch)")
        losses = {}
        t_loss = 0.
        self._set_modes()
        S = batch[5] if len(batch) > 5 else None
        h = front if front is not None else self.front(batch)
        self._join_front(h)
        if h.online_pl is not None:
            batch = (*batch[:3], h.online_pl, *batch[4:])
        if self.precision == 'fp32':
            feat_frame = self.model_frame.head_fp32_train(h.teacher_enc) if self.if_spatial_contrastive else h.teacher_out
        else:
            feat_frame = self.model_frame.head(h.teacher_enc) if self.if_spatial_contrastive else h.teacher_out
        if self.config_option == 'frame2voxel':
            pl = batch[3]
            pred, feat_voxel = self.task_backend.forward_fp32_train(h.content) if self.precision == 'fp32' else self.task_backend(h.content)
            if self.switched:
                pl = hip.argmax_labels(pred[1].detach())
            loss_dense = self.task_loss(pred[1], pl) * self.weight_task_loss
            losses['dense_clip_loss'] = loss_dense.detach()
            if self.if_spatial_contrastive:
                k = self._pool(feat_voxel, batch[4], S)
                q = self._pool(feat_frame, batch[4], S)
                loss_nce = self.nce_loss(k, q)
                losses['contrastive_nce_loss'] = loss_nce.detach()
                t_loss = t_loss + loss_nce
            if self.if_dense_clip_supervision:
                t_loss = t_loss + loss_dense
        else:                                                                   # frame2recon (:475-529)
            recon, pl = batch[2], batch[3]
            logits_recon, feat_recon = self.model_recon(recon)
            if self.if_spatial_contrastive:
                k = self._pool(feat_recon, batch[4], S)
                q = self._pool(feat_frame, batch[4], S)
                loss_nce = self.nce_loss(k, q)
                losses['contrastive_nce_loss'] = loss_nce.detach()
                t_loss = t_loss + loss_nce
            if self.if_dense_clip_supervision:
                if self.switched:
                    pl = hip.argmax_labels(logits_recon.detach())
                loss_dense = self.task_loss(logits_recon, pl) * self.weight_task_loss
                losses['dense_clip_loss'] = loss_dense.detach()
                t_loss = t_loss + loss_dense
            if self.sam_distillation:                                           # :519-529
                loss_sam = hip.sam_distill_loss(sam_feat, feat_recon)
                losses['sam_distillation_loss'] = loss_sam.detach()
                t_loss = t_loss + loss_sam
        return t_loss, losses, {}

    # ------------------------------------------------------------------ pretrain_trainer.py:324-361
    def train_step(self, batch, sam_feat=None):
        for opt in self.optimizers_dict.values():
            opt.zero_grad()
        t_loss, losses, outputs = self.task_train_step(batch, sam_feat=sam_feat)
        t_loss.backward()
        for opt in self.optimizers_dict.values():
            opt.step()
        return losses, outputs, t_loss.detach()
