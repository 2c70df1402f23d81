"""OpenESSPretrainModel (training/pretrain_trainer.py:81-667): stage-1 trainer, F2E contrastive + T2E
pseudo-label distillation.  The step itself lives in pretrain_step.PretrainStep."""
import functools

import torch

from .base_trainer_ov import BaseTrainer, online_maskclip_refine
from .pretrain_step import PretrainStep, refuse_sam_distillation


class OpenESSPretrainModel(BaseTrainer):
    def __init__(self, settings, train=True):
        # `train_precision` (optional YAML key, clip block): arithmetic of the pre-training step.  Set before
        # BaseTrainer.__init__ logs the numeric mode; what fp32 cannot pre-train is refused here, before anything is built
        # (the same refusals as PretrainStep's constructor, which the online teacher's construction would otherwise precede).
        # val_step stays bf16: eval_precision is not wired for this trainer.
        self.train_precision = getattr(settings, 'train_precision', 'bf16')
        if self.train_precision not in ('bf16', 'fp32'):
            raise ValueError(f"train_precision must be 'bf16' or 'fp32', got {self.train_precision!r}")
        if self.train_precision == 'fp32':
            if settings.config_option != 'frame2voxel':
                raise NotImplementedError(f"train_precision: fp32 pre-trains frame2voxel, not {settings.config_option!r}: DeepLabv3 "
                                          "has no fp32 backward (train-mode BatchNorm, strided and dilated convolutions)")
            if getattr(settings, 'pl_sources', '') == 'online_maskclip':
                raise NotImplementedError("train_precision: fp32 has no online teacher (pl_sources: online_maskclip): the MaskCLIP "
                                          "ViT has no fp32 form")
            if getattr(settings, 'unfrozen_e2vid', False):
                raise NotImplementedError("train_precision: fp32 needs the frozen E2VID front end (unfrozen_e2vid: False): E2VID "
                                          "has no fp32 backward (5x5 stride-2 convolutions, ConvLSTM)")
        # `if_sam_distillation: True` runs with frame2recon on DSEC; `sam_feature_sources` names the folder of the
        # per-frame SAM features and means nothing without the loss
        if getattr(settings, 'if_sam_distillation', False):
            refuse_sam_distillation(settings.config_option, settings.dataset_name_b)
        elif getattr(settings, 'sam_feature_sources', ''):
            raise ValueError("sam_feature_sources is set but if_sam_distillation is not True: nothing would read the features")
        # pretrained weights: a checkpoint that cannot serve this run, or -- under require_pretrained: True -- a
        # named file that does not exist, is refused here too, before anything is built; quietly: PretrainStep resolves the
        # same sources again when it builds the networks and is the one that warns or reports
        self._pretrained_kwargs(settings, logger=None, check=True)
        super().__init__(settings, train)

    def _pretrained_kwargs(self, settings, logger, check=False):
        """PretrainStep's keywords of the frozen networks' weights, from the YAML: the E2VID checkpoint (`e2vid_checkpoint`, else
        path_to_model), the teacher's `image_weights` (+ `image_weights_path`), the frame2recon student's
        `pre_trained_backbone`.  check=True resolves them the way the step will and returns nothing."""
        from . import pretrained
        s = settings
        require = bool(getattr(s, 'require_pretrained', False))
        kw = dict(image_weights=getattr(s, 'image_weights', None), image_weights_path=getattr(s, 'image_weights_path', None),
                  require_pretrained=require, logger=logger)
        if s.config_option == 'frame2voxel':
            kw['e2vid_checkpoint'] = pretrained.e2vid_path(s)[1]
        elif s.config_option == 'frame2recon':
            kw['pretrained_backbone'] = s.pretrained_backbone or ''
        if check:
            if 'e2vid_checkpoint' in kw:
                pretrained.e2vid_source(kw['e2vid_checkpoint'], pretrained.e2vid_path(s)[0], s.nr_temporal_bins_b,
                                        self.train_precision == 'fp32', require)
            pretrained.backbone_path(kw.get('pretrained_backbone', ''), require)
            pretrained.teacher_path(kw['image_weights'], kw['image_weights_path'], require)
            return None
        return kw

    def init_fn(self):
        """pretrain_trainer.py:87-89: models, then optimisers, then the loss objects."""
        self.buildModels()
        self.createOptimizerDict()
        self.task_loss, self.nce_loss = self.step.task_loss, self.step.nce_loss

    def buildModels(self):
        """pretrain_trainer.py:106-229: `models_dict` (front_sensor_b / back_end / model_frame / model_recon) and the reconstructor."""
        s = self.settings
        text = None
        if s.text_embeddings_path and torch.cuda.is_available():
            try:
                text = torch.load(s.text_embeddings_path, map_location='cpu')
            except (FileNotFoundError, OSError):
                s.logger.info("text embeddings '%s' not found: random unit-norm embeddings", s.text_embeddings_path)
        online = online_labels = None
        if getattr(s, 'pl_sources', '') == 'online_maskclip':          # extension: labels from the frozen tower, in the step
            from ..models.maskclip_model import maskClipFeatureExtractor
            kw = {k: getattr(s, k) for k in ('text_embeddings_path', 'visual_projs_path', 'maskclip_checkpoint') if getattr(s, k, None)}
            # `online_maskclip_refine: True` (optional YAML keys, clip block): the labels are the argmax of the
            # refined forward (prompt denoising + key smoothing at the two thresholds), in either precision
            refine = online_maskclip_refine(s)
            online = maskClipFeatureExtractor(text_categories=s.semseg_num_classes, **kw, **(refine or {})).to(self.device).eval()
            # `online_teacher_precision: fp32` (optional YAML key, clip block): the labels are the argmax of the
            # tower's fp32 forward.  PretrainStep takes any callable; the student's step stays bf16.
            precision = getattr(s, 'online_teacher_precision', 'bf16')
            if precision not in ('bf16', 'fp32'):
                raise ValueError(f"online_teacher_precision must be 'bf16' or 'fp32', got {precision!r}")
            # the step asks the tower for labels, not logits: the same integers from the stride-level logits on
            # hip.argmax_labels, without the [B, K, H, W] tensor; online_teacher stays the logits form of the same choices (a tower
            # class with no `labels` gets its logits argmax-ed by the step, as before)
            if hasattr(online, 'labels'):
                online_labels = functools.partial(online.labels, refine=refine is not None, precision=precision)
            if precision == 'fp32':
                online = online.forward_fp32
            if refine is not None:
                online = functools.partial(online, refine=True)
        # `if_switchable_train: True` (read next to if_finetuning, config/settings.py): from epoch 5 on the dense-CLIP pseudo-labels
        # are the argmax of the student's own logits (pretrain_trainer.py:513-514, :556-557)
        self._switch_logged = False
        self.step = PretrainStep(config_option=s.config_option, online_teacher=online, online_labels=online_labels,
                                 switchable_train=bool(getattr(s, 'if_switchable_train', False)),
                                 sam_distillation=bool(getattr(s, 'if_sam_distillation', False)),
                                 num_classes=s.semseg_num_classes, img_size=tuple(s.img_size_b),
                                 nr_events_data=s.nr_events_data_b, nr_temporal_bins=s.nr_temporal_bins_b,
                                 if_spatial_contrastive=s.if_spatial_contrastive,
                                 if_dense_clip_supervision=s.if_dense_clip_supervision, superpixel_size=s.superpixel_size,
                                 lr=s.lr_voxel, weight_task_loss=s.weight_task_loss, task_loss=tuple(s.task_loss),
                                 output_stride=s.output_stride, device=self.device, text_embeddings=text,
                                 precision=self.train_precision, e2vid_options=getattr(s, 'e2vid_config', None),
                                 **self._pretrained_kwargs(s, logger=s.logger))
        self.models_dict = self.step.models_dict
        self.reconstructor = getattr(self.step, 'reconstructor', None)

    def createOptimizerDict(self):
        """pretrain_trainer.py:231-243: one AdamW per trained module, keys optimizer_voxel / optimizer_recon / optimizer_frame,
        learning rates from the settings."""
        if not self.is_training:
            self.optimizers_dict = {}
            return
        s = self.settings
        self.optimizers_dict = self.step.optimizers_dict
        for key, lr in (('optimizer_voxel', s.lr_voxel), ('optimizer_recon', s.lr_recon), ('optimizer_frame', s.lr_frame)):
            if key in self.optimizers_dict:
                for g in self.optimizers_dict[key].param_groups:
                    g['lr'] = lr

    def task_train_step(self, batch, front=None, sam_feat=None):
        return self.step.task_train_step(batch, front=front, sam_feat=sam_feat)

    def front_step(self, batch):
        """Frozen half of the step (teacher encoder, recurrent E2VID encoder) for `batch`, enqueued on its own HIP streams: trainEpoch
        calls it for batch i+1 before train_step(batch i, front=...) (PretrainStep.front / pipeline_steps)."""
        self._sync_epoch()
        return self.step.front(batch)

    def _sync_epoch(self):
        """The step switches its pseudo-label source on the trainer's epoch counter (if_switchable_train)."""
        self.step.epoch_count = self.epoch_count
        if self.step.switched and not self._switch_logged:
            self._switch_logged = True
            self.settings.logger.info("if_switchable_train: epoch %d >= %d, pseudo-labels are now the argmax of the student's own "
                                      "logits (batch labels and the online teacher are unused)", self.epoch_count, self.step.switch_epoch)

    def train_step(self, batch, front=None):
        self._sync_epoch()
        for opt in self.optimizers_dict.values():
            opt.zero_grad()
        self.grad_reducer.prepare()          # N > 1: gradients accumulate straight into the all-reduce buckets
        t_loss, losses, outputs = self.task_train_step((batch[0], batch[1], batch[2], batch[3], batch[4], batch[-1]), front=front,
                                                       sam_feat=batch[5] if self.step.sam_distillation else None)
        t_loss.backward()
        self.grad_reducer()
        for opt in self.optimizers_dict.values():
            opt.step()
        return losses, outputs, t_loss.detach()

    def val_step(self, batch, sensor, i_batch, vis_reconstr_idx, file_path):
        """pretrain_trainer.py:625-655."""
        s = self.settings
        losses = {}
        gt = batch[1]
        if s.config_option in ('recon2voxel', 'frame2voxel'):
            self.reconstructor.last_states_for_each_channel = {'grayscale': None}
            for i in range(s.nr_events_data_b):
                _, _, content = self.reconstructor.update_reconstruction(batch[0], channel_slice=(i * s.input_channels_b, s.input_channels_b),
                                                                         need_latents=(i == s.nr_events_data_b - 1))
            pred, _ = self.models_dict['back_end'](content)
            pred = pred[1]
        else:
            pred, _ = self.models_dict['model_recon'](batch[2])
        losses['semseg_' + sensor + '_loss'] = self.task_loss(pred, gt).detach()
        self.metrics_semseg_b.update_batch(pred.argmax(dim=1), gt)
        return losses, None
