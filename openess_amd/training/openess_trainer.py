"""OpenESSModel (training/openess_trainer.py:78-656), the default branch of train.py: two DeepLabv3 students
(frame + reconstruction) trained jointly with T2E pseudo-label losses, an L1 feature-consistency loss, a cosine
logit-consistency loss and the superpixel InfoNCE loss.

Only the `frame2recon` option with `if_spatial_contrastive: True` is runnable in the reference
(openess_trainer.py:478-529): `recon2voxel` references an undefined `superpixels` (:379 vs :408-409) and
`frame2voxel` computes an unused contrastive value while trainEpoch reads a key that was never written
(:464-475, :307-308).  Those two branches raise NotImplementedError here instead of being silently "fixed".
The MaskCLIP tower the reference constructs (:107-114) is never called by any of its steps; it is built here (frozen,
`models_dict['model_clip']`) when the three files it needs exist, and is available as an online teacher
(`self.model_clip(frame) -> logits`), see openess_amd/models/maskclip_model.py."""
import contextlib
import os

import torch
import torch.nn.functional as f

from .. import hip
from ..models.deeplabv3 import deeplabv3_resnet50
from ..utils.loss_functions import NCELoss, TaskLoss
from ..utils.optim import AdamW          # torch.optim.AdamW with its step on the multi-tensor HIP kernel
from .base_trainer_ov import BaseTrainer


class OpenESSModel(BaseTrainer):
    pool_superpixel_size = 30        # superpixel_size hard-coded in the pooling of openess_trainer.py:506 (base trainer: host-side row count)
    # the 256-channel full-resolution features of both students are only consumed by the L1 consistency loss and the superpixel
    # pooling: both work on the OS16 maps (hip.UpsampledFeature: one upsampled difference, one pooling matrix); False = tensors
    lazy_features = True
    # True: the two students' forward (and, through autograd, backward) passes on two HIP streams.  Measured at the BASELINE size over
    # five alternating pairs of runs (round 5): 300 vs 294 event-frames/s with a +-30 run-to-run spread -- no gain to show, so
    # the default stays one stream; the switch and its bit-equality test remain.
    two_streams = False

    def __init__(self, settings, train=True):
        # `train_precision` / `eval_precision` (optional YAML keys, clip block): arithmetic of train_step / val_step, 'bf16' (storage;
        # fp32 accumulation) or 'fp32' (the reference's); refused here, before anything is built
        self.train_precision = getattr(settings, 'train_precision', 'bf16')
        if self.train_precision not in ('bf16', 'fp32'):
            raise ValueError(f"train_precision must be 'bf16' or 'fp32', got {self.train_precision!r}")
        self.eval_precision = getattr(settings, 'eval_precision', 'bf16')
        if self.eval_precision not in ('bf16', 'fp32'):
            raise ValueError(f"eval_precision must be 'bf16' or 'fp32', got {self.eval_precision!r}")
        super().__init__(settings, train)

    def init_fn(self):
        """openess_trainer.py:84-86: models, then optimisers, then the loss objects."""
        s = self.settings
        if s.config_option != 'frame2recon':
            raise NotImplementedError("OpenESSModel: only config_option 'frame2recon' is runnable in the reference "
                                      "(openess_trainer.py:360-535); see the module docstring")
        self.buildModels()
        self.createOptimizerDict()
        self.task_loss = TaskLoss(losses=list(s.task_loss), gamma=2.0, num_classes=s.semseg_num_classes, ignore_index=255)
        self.nce_loss = NCELoss(temperature=0.07)
        self.l1_loss = torch.nn.L1Loss()

    def buildModels(self):
        """openess_trainer.py:104-225: the two DeepLabv3 students and, when its three files exist, the frozen MaskCLIP tower."""
        s = self.settings
        mk = lambda: deeplabv3_resnet50(num_classes=s.semseg_num_classes, text_embeddings_path='',
                                        output_stride=s.output_stride, pretrained_backbone=s.pretrained_backbone)
        self.model_recon, self.model_frame = mk(), mk()
        self.models_dict = {'model_recon': self.model_recon, 'model_frame': self.model_frame}
        self.model_recon.lazy_feats = self.model_frame.lazy_feats = bool(self.lazy_features)
        paths = [getattr(s, k, None) for k in ('text_embeddings_path', 'visual_projs_path', 'maskclip_checkpoint')]
        if all(p and os.path.isfile(p) for p in paths):                     # openess_trainer.py:107-114
            from ..models.maskclip_model import maskClipFeatureExtractor
            self.model_clip = maskClipFeatureExtractor(text_embeddings_path=paths[0], visual_projs_path=paths[1],
                                                       text_categories=s.semseg_num_classes, maskclip_checkpoint=paths[2])
            self.models_dict['model_clip'] = self.model_clip
        for m in self.models_dict.values():
            m.to(self.device)

    def createOptimizerDict(self):
        """openess_trainer.py:228-258: optimizer_recon / optimizer_frame."""
        if not self.is_training:
            self.optimizers_dict = {}
            return
        s = self.settings
        self.optimizers_dict = {
            'optimizer_recon': AdamW([p for p in self.model_recon.parameters() if p.requires_grad], lr=s.lr_recon),
            'optimizer_frame': AdamW([p for p in self.model_frame.parameters() if p.requires_grad], lr=s.lr_frame)}

    def _step_precision(self, precision):
        """Arithmetic of one training step: `precision`, or the trainer's train_precision for None (the rule of _supervised.py)."""
        precision = self.train_precision if precision is None else precision
        if precision not in ('bf16', 'fp32'):
            raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
        if precision == 'fp32' and self.two_streams:
            raise NotImplementedError("two_streams with fp32: the fp32 convolution workspaces are kept per stream and the "
                                      "combination is untested; run the fp32 step on one stream")
        return precision

    def task_train_step(self, batch, precision=None):
        """Forward and losses of one step.  precision: 'bf16' / 'fp32' for this call, None for the trainer's train_precision.
        fp32: both students through deeplabv3_resnet50.forward_fp32_train, the same loss nodes on fp32 operands;
        with lazy_features the L1 consistency is hip.upsampled_l1_mean on the two maps at the network's stride."""
        s = self.settings
        precision = self._step_precision(precision)
        losses, t_loss = {}, 0.
        for m in self.models_dict.values():
            m.train()
        frame, recon, pl, superpixels = batch[0], batch[2], batch[3], batch[4]
        if precision == 'fp32':
            want = 'lazy' if self.lazy_features else True
            fwd_frame = lambda x: self.model_frame.forward_fp32_train(x, want_feats=want)
            fwd_recon = lambda x: self.model_recon.forward_fp32_train(x, want_feats=want)
        else:
            fwd_frame, fwd_recon = self.model_frame, self.model_recon
        side = None
        if self.two_streams and frame.is_cuda:
            # The two students share no data until the consistency losses.  Their small-map layers (OS16: 140-560 workgroups per
            # launch on 256 CUs) leave most of the chip idle, so the frame student runs on a second HIP stream next to the
            # reconstruction student; autograd replays each node on the stream of its forward, so the two backward passes
            # interleave the same way.  Same kernels, same buffers, ordered by events: results are bit-identical.
            from .. import engine
            engine.PackedWeight.refresh_stale(self.device)        # on THIS stream, before the fork: no repack from the side stream
            if getattr(self, '_side_stream', None) is None:
                self._side_stream = torch.cuda.Stream(device=self.device)
            side, main = self._side_stream, torch.cuda.current_stream(self.device)
            side.wait_stream(main)
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            logits_frame, feat_frame = fwd_frame(frame)
            l_frame = self.task_loss(logits_frame, pl) * s.weight_task_loss
        logits_recon, feat_recon = fwd_recon(recon)
        l_recon = self.task_loss(logits_recon, pl) * s.weight_task_loss
        if side is not None:
            main.wait_stream(side)
            for t in (logits_frame, getattr(feat_frame, 'x', feat_frame), l_frame):
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(main)
        losses['semseg_frame_loss'] = l_frame.detach()
        t_loss = t_loss + l_frame
        losses['semseg_recon_loss'] = l_recon.detach()
        t_loss = t_loss + l_recon
        if precision == 'fp32' and isinstance(feat_frame, hip.UpsampledFeature):
            l = hip.upsampled_l1_mean(feat_frame, feat_recon)                # nn.L1Loss (:497) without the 2.3 GB difference
        else:
            l = hip.l1_mean(feat_frame, feat_recon)                          # nn.L1Loss (:497)
        losses['cons_feat_loss'] = l.detach()
        t_loss = t_loss + l
        l = hip.cosine_mean_loss(logits_frame, logits_recon)                 # mean(1 - cosine_similarity) (:501)
        losses['cons_pred_loss'] = l.detach()
        t_loss = t_loss + l
        if getattr(s, 'if_spatial_contrastive', False):
            sps = self.pool_superpixel_size                               # superpixel_size hard-coded to 30 (:506)
            # row count from the loader (host side, last item of a prepared batch): no device sync here
            S = batch[-1] if len(batch) > 5 and isinstance(batch[-1], int) else None
            if isinstance(feat_recon, hip.UpsampledFeature):
                # both maps are pooled over the same superpixels from the same geometry: one pooling matrix serves the four products
                if S is None:
                    off = torch.arange(0, superpixels.shape[0] * sps, sps, device=superpixels.device)[:, None, None]
                    S = int((superpixels + off).max().item()) + 1
                m = hip.pool_matrix(superpixels, feat_recon.x.shape[2:], sps, S, feat_recon.align_corners)
                k = feat_recon.pool(superpixels, sps, S, matrix=m)
                q = feat_frame.pool(superpixels, sps, S, matrix=m)
            else:
                k = hip.superpixel_pool(feat_recon, superpixels, sps, S=S)
                q = hip.superpixel_pool(feat_frame, superpixels, sps, S=S)
            l = self.nce_loss(k, q)
            losses['contrastive_nce_loss'] = l.detach()
            t_loss = t_loss + l
        return t_loss, losses, {}

    def train_step(self, batch, precision=None):
        precision = self._step_precision(precision)      # refused before the gradients are cleared
        for opt in self.optimizers_dict.values():
            opt.zero_grad()
        self.grad_reducer.prepare()
        t_loss, losses, outputs = self.task_train_step(batch, precision=precision)
        t_loss.backward()
        self.grad_reducer()
        for opt in self.optimizers_dict.values():
            opt.step()
        return losses, outputs, t_loss.detach()

    def val_logits(self, batch, precision=None):
        """Class logits of one validation batch in `precision` (default: the trainer's eval_precision).  'fp32' runs
        deeplabv3_resnet50.forward_fp32 on the eval-mode network and puts the modules' train / eval flags back (the rule of
        SupervisedTrainer.val_logits); it shares no state with the bf16 path or the training step."""
        precision = self.eval_precision if precision is None else precision
        if precision not in ('bf16', 'fp32'):
            raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
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

    def val_step(self, batch, sensor, i_batch, vis_reconstr_idx, file_path):
        pred = self.val_logits(batch)
        losses = {'semseg_' + sensor + '_loss': self.task_loss(pred, batch[1]).detach()}
        self.metrics_semseg_b.update_batch(pred.argmax(dim=1), batch[1])
        return losses, None
