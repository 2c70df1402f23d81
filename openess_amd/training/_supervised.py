"""Shared body of the stage-2/3 trainers (supervised Dice + CE on ground-truth labels, one AdamW):
training/finetune_trainer.py:81-492, training/linear_probe_trainer.py:79-491, training/sup_only_trainer.py:80-511 are three
near-copies in the reference; what differs between them lives in the three modules of the same names next to this file."""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as f

from ..e2vid.image_reconstructor import ImageReconstructor
from ..e2vid.model.model import E2VID_LIGHTWEIGHT_CONFIG, E2VIDRecurrent
from ..models.deeplabv3 import deeplabv3_resnet50
from ..models.style_networks import SemSegE2VID
from ..utils.loss_functions import TaskLoss
from ..utils.optim import AdamW          # torch.optim.AdamW with its step on the multi-tensor HIP kernel
from . import pretrained
from .base_trainer_ov import BaseTrainer


class SupervisedTrainer(BaseTrainer):
    """What the three stage-2/3 trainers share.  A subclass states its differences through three hooks:
    `backend_kwargs()` (extra SemSegE2VID constructor arguments), `deeplab_kwargs()` (extra deeplabv3_resnet50 constructor
    arguments) and `amp_requested()` (whether the reference would build a GradScaler for this trainer)."""

    def __init__(self, settings, train=True):
        # `eval_precision` (optional YAML key, clip block): arithmetic of val_step; refused here, before anything is built
        self.eval_precision = getattr(settings, 'eval_precision', 'bf16')
        if self.eval_precision not in ('bf16', 'fp32'):
            raise ValueError(f"eval_precision must be 'bf16' or 'fp32', got {self.eval_precision!r}")
        if self.eval_precision == 'fp32' and settings.config_option == 'frame2recon':
            raise NotImplementedError("eval_precision: fp32 is not wired for frame2recon: the key switches val_step of frame2voxel / "
                                      "recon2voxel only.  DeepLabv3 in fp32 is reached through val_logits(batch, precision='fp32') "
                                      "and tools/eval_precision.py --config-option frame2recon")
        # `train_precision` (optional YAML key, clip block): arithmetic of the training step, independent of
        # eval_precision.  What fp32 cannot train is refused here, before any model is built, naming the missing piece.
        self.train_precision = getattr(settings, 'train_precision', 'bf16')
        if self.train_precision not in ('bf16', 'fp32'):
            raise ValueError(f"train_precision must be 'bf16' or 'fp32', got {self.train_precision!r}")
        if self.train_precision == 'fp32':
            if settings.config_option not in ('frame2voxel', 'recon2voxel'):
                raise NotImplementedError(f"train_precision: fp32 trains frame2voxel / recon2voxel, not {settings.config_option!r}: "
                                          "DeepLabv3 has no fp32 backward (train-mode BatchNorm, strided and dilated convolutions)")
            if settings.unfrozen_e2vid:
                raise NotImplementedError("train_precision: fp32 needs the frozen E2VID front end (unfrozen_e2vid: False): E2VID "
                                          "has no fp32 backward (5x5 stride-2 convolutions, ConvLSTM)")
            SemSegE2VID.check_fp32_config(settings.skip_connect_task_type, False)
        # pretrained weights: a front-end checkpoint that cannot serve this run, or -- under
        # require_pretrained: True -- a named file that does not exist, is refused here, before anything is built (quietly:
        # buildModels resolves the same source again and is the one that warns or reports)
        self._e2vid_source(settings, logger=None)
        if settings.config_option == 'frame2recon':
            pretrained.backbone_path(settings.pretrained_backbone, bool(getattr(settings, 'require_pretrained', False)))
        super().__init__(settings, train)

    def _e2vid_source(self, settings, logger):
        """(path, (config, state_dict) | None) of the frozen front end named by the YAML (`e2vid_checkpoint`, else path_to_model);
        (None, None) for a config_option without one."""
        if settings.config_option not in ('recon2voxel', 'frame2voxel'):
            return None, None
        key, path = pretrained.e2vid_path(settings)
        fp32 = 'fp32' in (getattr(self, 'eval_precision', 'bf16'), getattr(self, 'train_precision', 'bf16'))
        return path, pretrained.e2vid_source(path, key, settings.nr_temporal_bins_b, fp32,
                                             bool(getattr(settings, 'require_pretrained', False)), logger)

    def backend_kwargs(self):
        return {}

    def deeplab_kwargs(self):
        return {}

    def amp_requested(self):
        return False

    def init_fn(self):
        """finetune_trainer.py:86-88 (and its two siblings): models, then optimisers, then the loss object."""
        s = self.settings
        self.buildModels()
        self.createOptimizerDict()
        self.task_loss = TaskLoss(losses=list(s.task_loss), gamma=2.0, num_classes=s.semseg_num_classes, ignore_index=255)
        # The arithmetic follows train_precision (bf16 storage with fp32 accumulation, or fp32) whatever use_amp says; neither
        # has fp16's narrow exponent range, so the GradScaler the reference builds under use_amp (sup_only_trainer.py:247-252)
        # has nothing to do and is None here.
        self.scaler = None
        if self.amp_requested():
            mode = "fp32" if self.train_precision == 'fp32' else "bf16 storage / fp32 accumulation"
            self.settings.logger.info(f"use_amp requested: the step runs in {mode} (train_precision); no GradScaler is built")

    def buildModels(self):
        """finetune_trainer.py:104-196: `models_dict` (front_sensor_b + back_end, or model_recon) and the reconstructor."""
        s = self.settings
        self.models_dict = {}
        text_path = '' if not s.text_embeddings_path else s.text_embeddings_path
        try:
            open(text_path).close() if text_path else None
        except OSError:
            text_path = ''
        if s.config_option in ('recon2voxel', 'frame2voxel'):
            # the front end named by the YAML (finetune_trainer.py: load_model(self.settings.path_to_model)): built from the
            # checkpoint's own config, or -- no file -- E2VID_lightweight from the seed as before
            ckpt_path, ckpt = self._e2vid_source(s, logger=s.logger)
            self.front_end_sensor_b = E2VIDRecurrent(ckpt[0] if ckpt is not None else E2VID_LIGHTWEIGHT_CONFIG)
            if ckpt is not None:
                pretrained.load_e2vid(self.front_end_sensor_b, ckpt, ckpt_path, s.logger)
            if not s.unfrozen_e2vid:
                for p in self.front_end_sensor_b.parameters():
                    p.requires_grad = False
                self.front_end_sensor_b.eval()
            self.input_height = math.ceil(s.img_size_b[0] / 8.0) * 8
            self.input_width = math.ceil(s.img_size_b[1] / 8.0) * 8
            self.models_dict['front_sensor_b'] = self.front_end_sensor_b
            self.task_backend = SemSegE2VID(input_c=256, output_c=s.semseg_num_classes, skip_connect=s.skip_connect_task,
                                            skip_type=s.skip_connect_task_type, text_embeddings_path=text_path,
                                            materialize_ch256=False, **self.backend_kwargs())
            self.models_dict['back_end'] = self.task_backend
        elif s.config_option == 'frame2recon':
            self.model_recon = deeplabv3_resnet50(num_classes=s.semseg_num_classes, text_embeddings_path=text_path,
                                                  output_stride=s.output_stride, pretrained_backbone=s.pretrained_backbone,
                                                  **self.deeplab_kwargs())
            self.models_dict['model_recon'] = self.model_recon
        else:
            raise NotImplementedError(s.config_option)
        for m in self.models_dict.values():
            m.to(self.device)
        if 'front_sensor_b' in self.models_dict:
            self.reconstructor = ImageReconstructor(self.front_end_sensor_b, self.input_height, self.input_width,
                                                    s.nr_temporal_bins_b, self.device, s.e2vid_config)
            if 'fp32' in (self.eval_precision, self.train_precision):
                # the reference's arithmetic: a second reconstructor over the SAME model with states and packed operands of its
                # own, so nothing the bf16 path reads is shared.  ONE serves fp32 validation and fp32 training: the two never run
                # at the same time, and each sequence starts from and leaves empty states (_latents_fp32)
                self.task_backend.check_fp32()
                opts = SimpleNamespace(**dict(vars(s.e2vid_config), precision='fp32'))
                self.reconstructor_fp32 = ImageReconstructor(self.front_end_sensor_b, self.input_height, self.input_width,
                                                             s.nr_temporal_bins_b, self.device, opts)

    def createOptimizerDict(self):
        """finetune_trainer.py:198-238: one AdamW over the trainable parameters of the student (optimizer_voxel / optimizer_recon)."""
        if not self.is_training:
            self.optimizers_dict = {}
            return
        s = self.settings
        if 'back_end' in self.models_dict:
            trainable = [p for p in self.task_backend.parameters() if p.requires_grad]
            self.optimizers_dict = {'optimizer_voxel': AdamW(trainable, lr=s.lr_voxel)}
        else:
            trainable = [p for p in self.model_recon.parameters() if p.requires_grad]
            self.optimizers_dict = {'optimizer_recon': AdamW(trainable, lr=s.lr_recon)}

    def _latents(self, event):
        s = self.settings
        self.reconstructor.last_states_for_each_channel = {'grayscale': None}
        for i in range(s.nr_events_data_b):
            _, _, latent = self.reconstructor.update_reconstruction(event, channel_slice=(i * s.input_channels_b, s.input_channels_b),
                                                                    need_latents=(i == s.nr_events_data_b - 1))
        return latent

    def _latents_fp32(self, event, latents_only=False):
        """fp32 latents of the last sub-window.  latents_only (the training step): the encoder-only E2VID step, same bits.
        The encoder latents are views of the sequence's own cat(x, h) state buffers.  Every call starts from empty states, so these
        buffers are allocated by this call, and it drops the states before it returns: the returned views are then the only
        references, no later call can reach (let alone write) the buffers, and the caching allocator cannot hand them out again
        while a view lives.  Within the call only earlier sub-windows are overwritten, whose latents nobody keeps."""
        s = self.settings
        rec = self.reconstructor_fp32
        rec.last_states_for_each_channel = {'grayscale': None}
        for i in range(s.nr_events_data_b):
            _, _, latent = rec.update_reconstruction(event, channel_slice=(i * s.input_channels_b, s.input_channels_b),
                                                     latents_only=latents_only)
        rec.last_states_for_each_channel = {'grayscale': None}
        return latent

    def _step_precision(self, precision):
        """Arithmetic of one training step: `precision`, or the trainer's train_precision for None.  The event students in fp32
        need the fp32 reconstructor, which only a trainer built with train_precision / eval_precision: fp32 has (the rule of
        val_logits); frame2recon needs nothing beyond its model (deeplabv3_resnet50.forward_fp32_train)."""
        precision = self.train_precision if precision is None else precision
        if precision not in ('bf16', 'fp32'):
            raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
        if precision == 'fp32' and self.settings.config_option in ('recon2voxel', 'frame2voxel') and \
                getattr(self, 'reconstructor_fp32', None) is None:
            raise RuntimeError("this trainer was built without train_precision: fp32")
        return precision

    def _train_latents(self, event, precision=None):
        """Detached latents of the frozen front end in the arithmetic of the training step."""
        precision = self.train_precision if precision is None else precision
        latent = self._latents_fp32(event, latents_only=True) if precision == 'fp32' else self._latents(event)
        return {k: v.detach() for k, v in latent.items()}

    def _set_modes(self):
        s = self.settings
        for name, m in self.models_dict.items():
            m.train()
            if name == 'front_sensor_b' and not s.unfrozen_e2vid:
                m.eval()

    def front_step(self, batch):
        """Frozen half of a step: the recurrent E2VID encoder (frozen in every fine-tune / linear-probe YAML) depends on no weight
        the optimiser touches, so BaseTrainer.trainEpoch enqueues it for batch i+1 on its own HIP stream BEFORE the trainable half
        of batch i (decoder forward / backward / AdamW, bound by HBM) and it runs under it.  Returns None when there is nothing
        frozen to run ahead (frame2recon, unfrozen_e2vid): the step then runs whole in train_step.
        train_precision fp32 takes the same route: the latents of batch i (saved by the decoder's fp32 conv backward) are views
        of buffers that front_step(batch i + 1) cannot reach (_latents_fp32), allocated on the front stream and handed to the main
        stream with the same event / record_stream pair; the kernels' workspaces are kept per stream (hip._workspace)."""
        s = self.settings
        if s.config_option not in ('recon2voxel', 'frame2voxel') or s.unfrozen_e2vid or not batch[0].is_cuda:
            return None
        self._set_modes()
        if getattr(self, '_front_stream', None) is None:
            self._front_stream = torch.cuda.Stream(device=self.device)
        F, main = self._front_stream, torch.cuda.current_stream(self.device)
        F.wait_stream(main)
        with torch.cuda.stream(F):
            latent = self._train_latents(batch[0])
            self.reconstructor.last_states_for_each_channel = {'grayscale': None}
            done = torch.cuda.Event()
            done.record(F)
        return latent, done

    def task_train_step(self, batch, front=None, precision=None):
        """Forward and loss of one step.  precision: 'bf16' / 'fp32' for this call, None for the trainer's train_precision (a
        `front` handed in was computed by front_step in train_precision).  frame2recon takes fp32 only through this argument: the
        YAML key still refuses it at construction."""
        s = self.settings
        precision = self._step_precision(precision)
        if front is not None and precision != self.train_precision:
            raise ValueError(f"front_step computed its latents in {self.train_precision}; a {precision} step computes its own")
        losses, t_loss = {}, 0.
        self._set_modes()
        gt = batch[1]
        if s.config_option in ('recon2voxel', 'frame2voxel'):
            if front is not None:
                latent, done = front
                main = torch.cuda.current_stream(self.device)
                main.wait_event(done)
                for v in latent.values():
                    if torch.is_tensor(v):
                        v.record_stream(main)
            else:
                latent = self._train_latents(batch[0], precision)
            if precision == 'fp32':
                pred, _ = self.task_backend.forward_fp32_train(latent)
            else:
                pred, _ = self.task_backend(latent)
            labels = f.interpolate(gt.float().unsqueeze(1), size=(self.input_height, self.input_width), mode='nearest').squeeze(1).long()
            loss = self.task_loss(pred[1], labels) * s.weight_task_loss
            losses['semseg_sensor_b_loss'] = loss.detach()
        else:
            if precision == 'fp32':
                logits, _ = self.model_recon.forward_fp32_train(batch[2])
            else:
                logits, _ = self.model_recon(batch[2])
            loss = self.task_loss(logits, gt) * s.weight_task_loss
            losses['semseg_recon_loss'] = loss.detach()
        return t_loss + loss, losses, {}

    def train_step(self, batch, front=None, precision=None):
        precision = self._step_precision(precision)      # refused before the gradients are cleared
        for opt in self.optimizers_dict.values():
            opt.zero_grad()
        self.grad_reducer.prepare()          # N > 1: gradients accumulate straight into the all-reduce buckets
        t_loss, losses, outputs = self.task_train_step(batch, front=front, precision=precision)
        t_loss.backward()
        self.grad_reducer()
        for opt in self.optimizers_dict.values():
            opt.step()
        return losses, outputs, t_loss.detach()

    def val_logits(self, batch, precision=None):
        """Class logits of one validation batch in `precision` (default: the trainer's eval_precision).  'fp32' runs the E2VID
        encoder through the fp32 reconstructor and the decoder through SemSegE2VID.forward_fp32 (trainers built with
        eval_precision: fp32 only), or, frame2recon, deeplabv3_resnet50.forward_fp32 on the eval-mode network (any trainer; the
        modules' train / eval flags are put back); it shares no state with the bf16 path or the training step."""
        s = self.settings
        precision = self.eval_precision if precision is None else precision
        if precision not in ('bf16', 'fp32'):
            raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
        if s.config_option not in ('recon2voxel', 'frame2voxel'):
            model = self.models_dict['model_recon']
            if precision == 'bf16':
                return model(batch[2])[0]
            modes = [(m, m.training) for m in model.modules()]
            model.eval()
            try:
                return model.forward_fp32(batch[2])[0]
            finally:
                for m, training in modes:
                    m.training = training
        if precision == 'fp32':
            if getattr(self, 'reconstructor_fp32', None) is None:
                raise RuntimeError("this trainer was built without eval_precision: fp32")
            return self.models_dict['back_end'].forward_fp32(self._latents_fp32(batch[0]))[0][1]
        return self.models_dict['back_end'](self._latents(batch[0]))[0][1]

    def val_step(self, batch, sensor, i_batch, vis_reconstr_idx, file_path):
        gt = batch[1]
        pred = self.val_logits(batch)
        losses = {'semseg_' + sensor + '_loss': self.task_loss(pred, gt).detach()}
        self.metrics_semseg_b.update_batch(pred.argmax(dim=1), gt)
        return losses, None
