"""BaseTrainer (training/base_trainer_ov.py:20-590): loader construction, epoch / validation loops, checkpoint
hook, cosine LR.  Same overridable methods and attribute names (models_dict, optimizers_dict, lr_schedulers,
train_loader_sensor_b, val_loader_sensor_b, epoch_count, step_count, metrics_semseg_b).

MI355X-specific: `prepare_batch` takes the loader's RAW event columns and runs the batched HIP voxelizer on
the device (the reference voxelizes per sample in CPU loader workers and ships 901 MB of voxels per batch over
an unpinned H2D copy, base_trainer_ov.py:166-173 / pretrain_trainer.py:428-432); when torch.distributed is
initialised the step all-reduces gradients (training/ddp.py) and the sampler shards by rank."""
import math

import torch
import torch.distributed as dist
from torch.utils.data import DataLoader, Subset

from .. import hip
from ..config.settings import ONLINE_SLIC, dataset_superpixel_sources
from ..DSEC.dataset.sequence_ov import ONLINE_E2VID, voxelize_raw_batch
from ..evaluation.metrics import MetricsSemseg
from ..utils.saver import CheckpointSaver
from .ddp import GradAllReduce, broadcast_module_states, shard_indices


def online_slic_segments(settings, pool_size):
    """`superpixel_sources: 'online_slic'`: SLIC's n_segments for this run, None for every other source.  The
    refusals of the key: recon2voxel has no RGB frame to segment, and more segments than the pooling size would let one sample's
    ids run into the next sample's rows."""
    if getattr(settings, 'superpixel_sources', '') != ONLINE_SLIC:
        if getattr(settings, 'online_slic_connectivity', False):
            raise ValueError("online_slic_connectivity: True needs superpixel_sources: online_slic, got "
                             f"{getattr(settings, 'superpixel_sources', '')!r}")
        return None
    if settings.config_option == 'recon2voxel':
        raise ValueError("superpixel_sources: online_slic needs an RGB frame in the batch (config_option frame2voxel or frame2recon); "
                         "recon2voxel has none")
    n = getattr(settings, 'online_slic_segments', None)
    n = int(pool_size) if n is None else int(n)
    if n < 1 or n > pool_size:
        raise ValueError(f"online_slic_segments = {n} must be between 1 and the pooling size {pool_size} (superpixel_size): the "
                         f"pooling offsets sample b's ids by b * {pool_size}")
    return n


def online_slic_rows(H, W, n_segments, pool_size, connectivity):
    """Rows a sample's online SLIC labels can reach on an H x W frame, from the shapes alone: the K = ny nx centres, or with the
    connectivity pass its label bound (hip.slic_connectivity_sizes, about 2 K).  More than the pooling size is refused: sample
    b's ids are offset by b * pool_size."""
    ny, nx, _ = hip.slic_lattice(H, W, n_segments)
    K = ny * nx
    if not connectivity:
        if K > pool_size:
            raise ValueError(f"online_slic: a {(H, W)} frame with {n_segments} segments gives {K} centres, more than the pooling size "
                             f"{pool_size}")
        return K
    bound = hip.slic_connectivity_sizes(H, W, K)[2]
    if bound > pool_size:
        raise ValueError(f"online_slic_connectivity: a {(H, W)} frame with {n_segments} segments ({K} centres) can give {bound} labels "
                         f"after the connectivity pass, more than the pooling size {pool_size}: online_slic_segments must be about "
                         f"half the pooling size")
    return bound


def online_maskclip_refine(settings):
    """`online_maskclip_refine: True` (clip block): the online MaskCLIP teacher's labels come from the refined
    forward.  None when the key is off, else the tower's {'pd_thresh', 'ks_thresh'} (validated by Settings and again by
    MaskClipHead).  Refused without `pl_sources: online_maskclip`: there is no teacher to refine."""
    if not getattr(settings, 'online_maskclip_refine', False):
        return None
    if getattr(settings, 'pl_sources', '') != 'online_maskclip':
        raise ValueError(f"online_maskclip_refine: True needs pl_sources: online_maskclip, got {getattr(settings, 'pl_sources', '')!r}")
    return {'pd_thresh': getattr(settings, 'online_maskclip_pd_thresh', 0.5), 'ks_thresh': getattr(settings, 'online_maskclip_ks_thresh', 1.0)}


def online_recon_options(settings):
    """`recon_sources: 'online_e2vid'` (clip block): frame2recon's reconstructed image comes from the sample's
    events, inside prepare_batch.  None when the key is absent (the PNG tree), else {'precision', 'model'}.  The refusals of the
    key, each before anything is built: another config_option (only frame2recon reads a reconstruction next to a frame;
    recon2voxel stays on the PNG tree), DDD17 (its loader carries no raw events beside the frame), an unknown precision, a model
    file that does not exist ('random' is accepted, as e2vid.run_reconstruction.load_model accepts it), auto-HDR (its
    window belongs to a sequence, not to a shuffled batch), and e2vid_config.flip (the image would be rotated against the frame)."""
    import os
    src = getattr(settings, 'recon_sources', None)
    if src is None:
        return None
    if src != ONLINE_E2VID:
        raise ValueError(f"recon_sources must be {ONLINE_E2VID!r} or absent (the reconstructions/ tree), got {src!r}")
    if settings.config_option != 'frame2recon':
        raise ValueError(f"recon_sources: {ONLINE_E2VID} serves config_option frame2recon, got {settings.config_option!r}")
    if settings.dataset_name_b != 'DSEC_events':
        raise ValueError(f"recon_sources: {ONLINE_E2VID} serves DSEC_events, got {settings.dataset_name_b!r}")
    precision = getattr(settings, 'online_recon_precision', 'bf16')
    if precision not in ('bf16', 'fp32'):
        raise ValueError(f"online_recon_precision must be 'bf16' or 'fp32', got {precision!r}")
    model = getattr(settings, 'online_recon_model', None) or settings.path_to_model
    if model != 'random' and not os.path.isfile(model):
        raise ValueError(f"online_recon_model: E2VID checkpoint {model!r} not found ('random' builds seeded random weights)")
    if getattr(settings.e2vid_config, 'auto_hdr', False):
        raise ValueError(f"recon_sources: {ONLINE_E2VID} has no auto_hdr: its window is a property of a sequence, not of a batch")
    if getattr(settings.e2vid_config, 'flip', False):
        raise ValueError(f"recon_sources: {ONLINE_E2VID} cannot run with e2vid_config.flip: the reconstructed image would be rotated "
                         "by 180 degrees against the teacher's frame (hot_pixels_file is served)")
    return {'precision': precision, 'model': model}


def text_classes_options(settings):
    """`text_classes` (clip block): the text embeddings come from the class names, computed by CLIP's text tower
    on the GPU.  None when the key is absent, else {'classes', 'checkpoint', 'bpe', 'templates'}.  Refused, each before anything
    is built: the key without its two paths, together with a non-empty text_embeddings_path (two sources for one tensor), a
    path that is no file (the templates' included), a class count other than semseg_num_classes."""
    import os
    classes = getattr(settings, 'text_classes', None)
    if classes is None:
        return None
    ckpt, bpe = getattr(settings, 'clip_text_checkpoint', None), getattr(settings, 'clip_bpe_path', None)
    if not ckpt or not bpe:
        raise ValueError("text_classes needs clip_text_checkpoint (CLIP weights) and clip_bpe_path (the BPE merges file)")
    if getattr(settings, 'text_embeddings_path', None):
        raise ValueError(f"text_classes and text_embeddings_path ({settings.text_embeddings_path!r}) both name the text embeddings: "
                         "give one of them")
    templates = getattr(settings, 'text_templates', 'single')
    for key, path in (('clip_text_checkpoint', ckpt), ('clip_bpe_path', bpe)) + \
            ((('text_templates', templates),) if templates not in ('single', 'none') else ()):
        if not os.path.isfile(path):
            raise ValueError(f"{key}: {path!r} not found")
    if len(classes) != settings.semseg_num_classes:
        raise ValueError(f"text_classes names {len(classes)} classes, semseg_num_classes is {settings.semseg_num_classes}")
    return {'classes': classes, 'checkpoint': ckpt, 'bpe': bpe, 'templates': templates}


def write_text_embeddings(settings, options, device, rank=0):
    """The embeddings of `options` (text_classes_options) -> a file every text_embeddings_path consumer loads; the setting then
    names it, so every model receives them through the mechanism that exists.  The file lies in the run's log directory when
    there is one, else it is a temporary file."""
    import os
    import tempfile
    from ..models.clip_text import compute_text_embeddings
    emb = compute_text_embeddings(options['checkpoint'], options['bpe'], options['classes'], options['templates'], device)
    if getattr(settings, 'timestr', None) and os.path.isdir(os.path.dirname(settings.ckpt_dir)):
        path = os.path.join(os.path.dirname(settings.ckpt_dir), 'text_embeddings.pt' if rank == 0 else f'text_embeddings.rank{rank}.pt')
    else:
        fd, path = tempfile.mkstemp(prefix='openess_text_embeddings_', suffix='.pt')
        os.close(fd)
    torch.save(emb, path)
    settings.logger.info("text embeddings of %d classes from %s written to %s", emb.shape[0], options['checkpoint'], path)
    settings.text_embeddings_path = path
    return path


def online_recon_image(rec, post, vox, n, C, aug):
    """The voxels [B, n C, H, W] of n sub-windows -> the augmented student image fp32 [B, 3, H, W]: the frozen
    E2VID behind the ImageReconstructor `rec` over the sub-windows from empty states, leaving empty states -- sub-windows
    0 .. n - 2 with their latents dropped (bf16: fused head + skewed schedule; fp32: encoders only), the decoder once, on the last
    one -- then `post`.process_u8 on the cropped image and hip.recon_augment with the per-sample columns of `aug`."""
    fp32 = rec.precision == 'fp32'
    rec.last_states_for_each_channel = {'grayscale': None}
    for i in range(n - 1):
        kw = {'latents_only': True} if fp32 else {'need_latents': False}
        rec.update_reconstruction(vox, channel_slice=(i * C, C), **kw)
    img, _, _ = rec.update_reconstruction(vox, channel_slice=((n - 1) * C, C), reconstruct=True)
    rec.last_states_for_each_channel = {'grayscale': None}        # the sequence ends with the batch
    if rec.crop.needs_pad:
        img = img[:, :, rec.crop.iy0:rec.crop.iy1, rec.crop.ix0:rec.crop.ix1]
    u8 = post.process_u8(img[:, :1])
    return hip.recon_augment(u8, [int(bool(f)) for f in aug['flip']], aug['brightness'], aug['contrast'], aug['noise_seed'])


class BaseTrainer(object):
    is_training = True
    online_slic_segments = None      # SLIC's n_segments under `superpixel_sources: online_slic`, set by __init__
    online_recon = None              # {'precision', 'model'} under `recon_sources: online_e2vid`, set by __init__

    def __init__(self, settings, train=True):
        self.settings = settings
        self.is_training = bool(train)           # reference: every trainer's __init__(settings, train=True) (pretrain_trainer.py:82-83)
        # before anything is built: what `superpixel_sources: online_slic` cannot serve is refused here
        self.online_slic_segments = online_slic_segments(settings, self.pooling_size())
        online_maskclip_refine(settings)         # `online_maskclip_refine: True` without its teacher is refused here too
        self.online_recon = online_recon_options(settings)      # and what `recon_sources: online_e2vid` cannot serve
        text_classes = text_classes_options(settings)           # and `text_classes` without what it needs
        if not torch.cuda.is_available():
            raise RuntimeError("openess_amd trainers need the GPU (no CPU fallback in the product path)")
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.do_val_training_epoch = True
        self._png_pending = []                   # (slot, status tensor, file names) of device-decoded PNG maps not yet checked
        self._png_batches = 0                    # batches that queued at least one status vector since the last check
        # Precision contract (INTEGRATION.md "Precision"): the reference's `use_amp` switches torch.autocast(fp16) + GradScaler
        # (pretrain_trainer.py:344-353).  Here the flag is accepted and changes nothing: the arithmetic of the training step is bf16
        # storage of activations / activation gradients / MFMA weight operands with fp32 accumulation, or -- with
        # `train_precision: fp32` (DESIGN.md K19 stage 2/3, K20 frame2voxel pre-training) -- fp32 throughout; fp32 master weights,
        # optimiser state and losses either way;
        # no loss scaling is needed (bf16 has fp32's exponent range).  Say once what the run really does.
        use_amp = getattr(settings, 'use_amp', False)
        if getattr(self, 'train_precision', 'bf16') == 'fp32':
            msg = ("numeric mode: train_precision fp32 -- fp32 activations, gradients and MFMA operands (f32-input MFMA), fp32 "
                   "weights, optimiser state and losses; YAML use_amp={} is accepted and has no effect (no fp16-autocast mode, no "
                   "GradScaler)".format(use_amp))
        else:
            msg = ("numeric mode: bf16 storage / fp32 accumulate (MFMA), fp32 master weights and losses; YAML use_amp={} is "
                   "accepted and has no effect (no fp16-autocast mode; fp32 training is train_precision: fp32)".format(use_amp))
        settings.logger.info(msg)
        if self.rank_hint() == 0:
            print(msg)
        self.metrics_semseg_b = MetricsSemseg(settings.semseg_num_classes, settings.semseg_ignore_label,
                                              settings.semseg_class_names)
        # `text_classes`: before any trainer's buildModels (every init_fn starts with it), the embeddings are
        # computed and settings.text_embeddings_path names them; without the key nothing happens
        if text_classes is not None:
            write_text_embeddings(settings, text_classes, self.device, self.rank)
        self.init_fn()
        self.createDataLoaders()
        self.models_dict = {k: v.to(self.device) for k, v in self.models_dict.items()}
        if self.online_recon:
            self.build_online_recon()
        self.saver = CheckpointSaver(save_dir=settings.ckpt_dir)
        self.epoch_count = self.step_count = 0
        self.checkpoint = None
        if settings.resume_training:
            self.checkpoint = self.saver.load_checkpoint(self.models_dict, self.optimizers_dict,
                                                         checkpoint_file=settings.resume_ckpt_file, load_optimizer=False)
            self.epoch_count, self.step_count = self.checkpoint['epoch'], self.checkpoint['step_count']
        elif getattr(settings, 'load_pretrained_weights', False):
            self.saver.load_pretrained_weights(self.models_dict, self.models_dict.keys(), settings.pretrained_file,
                                               settings.frozen_backbone)
            settings.logger.info('Pretrained checkpoints loaded from {}'.format(settings.pretrained_file))
        if self.world > 1:
            broadcast_module_states(self.models_dict.values())
        self.grad_reducer = GradAllReduce([p for m in self.models_dict.values() for p in m.parameters()], self.world)
        self.epoch = self.epoch_count
        # cosine schedule with T_max = epochs * iterations but stepped once per EPOCH (base_trainer_ov.py:68-75,375-376)
        total_steps = settings.num_epochs * len(self.train_loader_sensor_b)
        self.lr_schedulers = {k: torch.optim.lr_scheduler.CosineAnnealingLR(v, T_max=max(total_steps, 1))
                              for k, v in self.optimizers_dict.items()}

    def pooling_size(self):
        """Rows per sample of the superpixel pooling: OpenESSModel pools with its own hard-coded size."""
        return getattr(self, 'pool_superpixel_size', None) or getattr(self.settings, 'superpixel_size', 100)

    def build_online_recon(self):
        """`recon_sources: online_e2vid`: a frozen E2VIDRecurrent of the trainer's own behind an ImageReconstructor
        of the requested precision, and the PostProcessor of settings.e2vid_config (reference defaults: unsharp 0.3, sigma 1,
        Imin 0, Imax 1).  The model is not entered in models_dict: never trained, never saved, checkpoint layouts untouched.
        Building it leaves the torch generators where they were ('random' seeds one)."""
        from types import SimpleNamespace
        from ..e2vid.image_reconstructor import ImageReconstructor, PostProcessor
        from ..e2vid.run_reconstruction import load_model
        s = self.settings
        with torch.random.fork_rng(devices=[self.device]):
            model = load_model(self.online_recon['model'])
        for p in model.parameters():
            p.requires_grad = False
        self.recon_model = model.to(self.device).eval()
        opts = SimpleNamespace(**dict(vars(s.e2vid_config), precision=self.online_recon['precision']))
        self.recon_reconstructor = ImageReconstructor(self.recon_model, s.img_size_b[0], s.img_size_b[1], s.nr_temporal_bins_b,
                                                      self.device, opts)
        self.recon_postprocessor = PostProcessor(self.device, s.e2vid_config)

    def voxelize_events(self, ev, split):
        """Collated raw events with explicit sub-window offsets -> [B, nr_events_data * C, H, W] on this stream."""
        ds = self._voxel_ds[split]
        if hasattr(ds, 'voxelize_batch'):
            return ds.voxelize_batch(ev, self.device)
        s = self.settings
        (H, W), crop = self.sensor_geometry                         # the synthetic provider: one rectify map, held by the trainer
        return voxelize_raw_batch(ev, self.device, self.rectify_maps, s.nr_temporal_bins_b, H, W, crop, s.nr_events_data_b)

    def reconstruct_online(self, ev, split):
        """Slot 2 under `recon_sources: online_e2vid`: collated raw events + the recon's augmentation columns -> the fp32
        [B, 3, H, W] image the student reads.  Voxelizer, the frozen E2VID over the sub-windows from empty states (the decoder
        runs once, on the last one), PostProcessor.process_u8, hip.recon_augment: all enqueued on the current stream (the ingest
        stream, under the previous step), nothing is waited for.  Validation batches take the same route with everything off."""
        s = self.settings
        vox = self.voxelize_events(ev, split)
        aug, B = ev['aug'], vox.shape[0]
        if split != 'train':
            aug = {'flip': [False] * B, 'brightness': [1.0] * B, 'contrast': [1.0] * B, 'noise_seed': [0] * B}
        return online_recon_image(self.recon_reconstructor, self.recon_postprocessor, vox, s.nr_events_data_b, s.input_channels_b, aug)

    @staticmethod
    def rank_hint():
        return dist.get_rank() if dist.is_initialized() else 0

    # ------------------------------------------------------------------ hooks for subclasses
    def init_fn(self):
        pass

    def train_step(self, batch):
        raise NotImplementedError

    def val_step(self, batch, sensor, i_batch, vis_reconstr_idx, file_path):
        raise NotImplementedError

    def trainEpoch(self):
        for m in self.models_dict.values():
            m.train()
        n = len(self.train_loader_sensor_b)
        batches = self.device_batches(self.train_loader_sensor_b)
        front_step = getattr(self, 'front_step', None)
        if front_step is not None and getattr(self.settings, 'pipeline_steps', True):
            # trainers with a frozen front half (OpenESSPretrainModel): front(batch i+1) is enqueued before the trainable half of
            # batch i, so that it runs under it (same results; settings.pipeline_steps: False = one step after the other)
            def results():
                prev = None
                for batch in batches:
                    fr = front_step(batch)
                    if prev is not None:
                        yield self.train_step(prev[0], front=prev[1])
                    prev = (batch, fr)
                if prev is not None:
                    yield self.train_step(prev[0], front=prev[1])
            outs = results()
        else:
            outs = (self.train_step(batch) for batch in batches)
        for i_batch, out in enumerate(outs):
            if i_batch % 20 == 0 and self.rank == 0:
                self.log_train(i_batch, n, out[0])
            self.step_count += 1
            self.check_png_status()
        self.check_png_status(force=True)

    def device_batches(self, loader, split='train'):
        """Ingest pipeline (north_star: "straight from pinned host event buffers"): yields device batches whose host -> device
        copies AND voxelization were enqueued on a SIDE HIP stream.  The generator hands batch i to the caller, the caller
        enqueues step i on the current stream, and only then is batch i+1 pulled from the DataLoader (pinned by its pin
        thread) and its copies + voxelizer launches enqueued on the side stream -- the host runs ahead of the GPU, so they
        execute under step i.  The current stream waits on one event per batch; tensors produced on the side stream are
        handed to the consumer stream with record_stream, so the caching allocator cannot recycle them early.
        `settings.ingest_prefetch: False` (or a CPU-only debug run) falls back to the in-order path."""
        release = getattr(loader, 'consumed_after', None)       # PinnedRingLoader: the slot returns to the workers after our copies
        if not getattr(self.settings, 'ingest_prefetch', True):
            for sample_batched in loader:
                batch = self.prepare_batch(sample_batched, split)
                if release is not None:
                    done = torch.cuda.Event()
                    done.record(torch.cuda.current_stream(self.device))
                    release(done)
                yield batch
            return
        if getattr(self, '_ingest_stream', None) is None:
            self._ingest_stream = torch.cuda.Stream(device=self.device)
        side = self._ingest_stream
        side.wait_stream(torch.cuda.current_stream(self.device))       # once: everything set up so far (rectify maps, weights)
        it = iter(loader)

        def produce():
            try:
                sample_batched = next(it)
            except StopIteration:
                return None
            with torch.cuda.stream(side):           # NOT ordered after the step just enqueued on the current stream: that is the overlap
                batch = self.prepare_batch(sample_batched, split)
                ready = torch.cuda.Event()
                ready.record(side)
                if release is not None:
                    release(ready)
            return batch, ready

        try:
            nxt = produce()
            while nxt is not None:
                batch, ready = nxt
                main = torch.cuda.current_stream(self.device)
                main.wait_event(ready)
                for t in batch:
                    if torch.is_tensor(t) and t.is_cuda:
                        t.record_stream(main)
                yield batch                              # the caller enqueues step i here ...
                nxt = produce()                          # ... and batch i+1 is copied + voxelized under it
        finally:
            # also on an early `break` of the consumer (GeneratorExit) or an exception in its step: a prefetched batch's copies and
            # voxelizer launches may still be in flight on the side stream, and the next user of the main stream must be ordered
            # after them
            torch.cuda.current_stream(self.device).wait_stream(side)

    _PNG_STATUS_TEXT = {1: 'bad signature', 2: 'bad IHDR', 3: 'unsupported (not 8-bit gray / palette, or interlaced)', 4: 'bad zlib header',
                        5: 'bad DEFLATE block', 6: 'bad Huffman code', 7: 'stream overrun', 8: 'size mismatch', 9: 'bad filter type'}

    def check_png_status(self, force=False):
        """device_png: a file the GPU decoder could not decode became an all-255 map (for a superpixel slot 255 is an ordinary id,
        not an ignore value), so training on it must not pass silently.  Every decoded slot's status vector is queued by
        prepare_batch; here they are reduced with ONE device sync per `settings.png_check_every` batches (default 50) and at epoch
        end, and a bad file raises with its slot, path and reason."""
        pend = self._png_pending
        every = int(getattr(self.settings, 'png_check_every', 50))
        if not pend or (not force and self._png_batches < every):      # counted in BATCHES, whatever the number of PNG slots per batch
            return
        self._png_pending = []
        self._png_batches = 0
        allst = torch.cat([st.reshape(-1) for _, st, _ in pend])
        if not bool((allst != 0).any()):                           # the one sync
            return
        bad = []
        for slot, st, paths in pend:
            for j, code in enumerate(st.tolist()):
                if code:
                    bad.append(f"batch slot {slot}, sample {paths[j] if paths else j}: {self._PNG_STATUS_TEXT.get(code, code)}")
        raise RuntimeError("device_png: undecodable label / pseudo-label / superpixel PNG(s) were replaced by all-255 maps:\n  "
                           + "\n  ".join(bad[:20]) + "\nRe-encode them as 8-bit grayscale or turn device_png off.")

    def log_train(self, i_batch, n, losses):
        msg = 'epoch: [{0}][{1}/{2}], '.format(self.epoch_count, i_batch, n) + ', '.join(
            "{}: {:.5f}".format(k, float(v)) for k, v in losses.items())
        print(msg)
        self.settings.logger.info(msg)

    def resetValidationStatistics(self):
        self.metrics_semseg_b.reset()

    # ------------------------------------------------------------------ data
    def getDataloader(self, dataset_name):
        """Dataset selector (base_trainer_ov.py:83-90)."""
        if getattr(self.settings, 'synthetic_data', False):
            from ..datasets.synthetic_events import SyntheticEvents
            return SyntheticEvents
        if dataset_name == 'DDD17_events':
            from ..datasets.ddd17_events_loader import DDD17Events
            return DDD17Events
        if dataset_name == 'DSEC_events':
            from ..datasets.DSEC_events_loader import DSECEvents
            return DSECEvents
        raise ValueError(dataset_name)

    def createDataLoaders(self):
        s = self.settings
        builder = self.getDataloader(s.dataset_name_b)
        from ..datasets.synthetic_events import SyntheticEvents, collate
        if builder is SyntheticEvents:
            sensor_hw = (s.img_size_b[0] + (40 if s.dataset_name_b == 'DSEC_events' else 60), s.img_size_b[1])
            crop = sensor_hw[0] - s.img_size_b[0]
            common = dict(sensor_hw=sensor_hw, crop_rows=crop, nr_events_data=s.nr_events_data_b,
                          nr_events_window=s.nr_events_window_b, nr_bins=s.nr_temporal_bins_b,
                          num_classes=s.semseg_num_classes, config_option=s.config_option,
                          superpixel_size=getattr(s, 'superpixel_size', 100))
            n_train = getattr(s, 'synthetic_length', 2 * s.batch_size_b * self.world)
            if self.online_recon:
                common.update(recon_sources=ONLINE_E2VID)
            train_ds = builder(length=n_train, mode='train', pool=getattr(s, 'synthetic_pool', 0),
                               superpixel_sources='' if self.online_slic_segments else None,
                               **({'recon_augmentation': bool(s.data_augmentation_train)} if self.online_recon else {}), **common)
            val_ds = builder(length=max(s.batch_size_b, 2), mode='val', **common)
        elif s.dataset_name_b == 'DSEC_events':
            train_ds, val_ds = self.createDSECDataset(
                s.dataset_name_b, s.dataset_path_b, s.batch_size_b, s.nr_events_data_b, s.delta_t_per_data_b, s.nr_events_window_b,
                s.data_augmentation_train, s.event_representation_b, s.nr_temporal_bins_b, s.require_paired_data_train_b,
                s.require_paired_data_val_b, s.separate_pol_b, s.normalize_event_b, s.semseg_num_classes, s.fixed_duration_b,
                s.config_option, getattr(s, 'pl_sources', ''), dataset_superpixel_sources(s), s.skip_ratio,
                getattr(s, 'if_sam_distillation', False))
        else:
            train_ds, val_ds = self.createDDD17EventsDataset(
                s.dataset_name_b, s.dataset_path_b, s.split_train_b, s.batch_size_b, s.nr_events_data_b, s.delta_t_per_data_b,
                s.nr_events_window_b, s.data_augmentation_train, s.event_representation_b, s.nr_temporal_bins_b,
                s.require_paired_data_train_b, s.require_paired_data_val_b, s.separate_pol_b, s.normalize_event_b, s.fixed_duration_b,
                s.config_option, getattr(s, 'pl_sources', ''), dataset_superpixel_sources(s), s.skip_ratio,
                getattr(s, 'if_sam_distillation', False))
        self.sensor_geometry = (train_ds.sensor_hw, train_ds.crop_rows) if hasattr(train_ds, 'sensor_hw') else None
        self.rectify_maps = torch.from_numpy(train_ds.rectify_map[None]).to(self.device) if hasattr(train_ds, 'rectify_map') else None
        self._voxel_ds = {'train': train_ds, 'val': val_ds}            # un-wrapped datasets: Subset has no voxelize_batch
        if self.world > 1:
            train_ds = Subset(train_ds, shard_indices(len(train_ds), self.rank, self.world).tolist())
        # settings.ring_loader (default on with worker processes): the workers collate straight into a pinned shared ring
        # (datasets/ring_loader.py: one host copy per byte instead of the DataLoader's three); False = torch's DataLoader
        if getattr(s, 'ring_loader', True) and s.num_cpu_workers > 0 and len(train_ds) >= s.batch_size_b:
            from ..datasets.ring_loader import PinnedRingLoader
            self.train_loader_sensor_b = PinnedRingLoader(train_ds, batch_size=s.batch_size_b, shuffle=True, drop_last=True,
                                                          num_workers=s.num_cpu_workers)
        else:
            self.train_loader_sensor_b = DataLoader(train_ds, batch_size=s.batch_size_b, num_workers=s.num_cpu_workers,
                                                    pin_memory=True, shuffle=True, drop_last=True, collate_fn=collate)
        self.val_loader_sensor_b = DataLoader(val_ds, batch_size=s.batch_size_b, num_workers=s.num_cpu_workers,
                                              pin_memory=True, shuffle=False, drop_last=False, collate_fn=collate)

    # The reference's two dataset factories (base_trainer_ov.py:93-183, 187-276) with their positional signatures.  They return the
    # (train, validation) DATASETS; createDataLoaders wraps them (ring loader / DataLoader, sharding), where the reference builds its
    # two torch DataLoaders inside the factory.
    def createDSECDataset(self, dataset_name, dsec_dir, batch_size, nr_events_data, delta_t_per_data, nr_events_window, augmentation,
                          event_representation, nr_bins_per_data, require_paired_data_train, require_paired_data_val, separate_pol,
                          normalize_event, semseg_num_classes, fixed_duration, config_option, pl_sources, superpixel_sources,
                          skip_ratio, if_sam_distillation):
        builder = self.getDataloader(dataset_name)
        kw = dict(dsec_dir=dsec_dir, nr_events_data=nr_events_data, delta_t_per_data=delta_t_per_data, nr_events_window=nr_events_window,
                  event_representation=event_representation, nr_bins_per_data=nr_bins_per_data, separate_pol=separate_pol,
                  normalize_event=normalize_event, semseg_num_classes=semseg_num_classes, fixed_duration=fixed_duration,
                  config_option=config_option, pl_sources=pl_sources, device_png=getattr(self.settings, 'device_png_decode', False))
        if self.online_recon:
            kw['recon_sources'] = ONLINE_E2VID          # slot 2 then carries raw events, no reconstructions/ file is opened
        train = builder(augmentation=augmentation, mode='train', require_paired_data=require_paired_data_train,
                        superpixel_sources=superpixel_sources, skip_ratio=skip_ratio, if_sam_distillation=if_sam_distillation,
                        **({'sam_feature_sources': self.settings.sam_feature_sources}
                           if getattr(self.settings, 'sam_feature_sources', '') else {}), **kw)
        val = builder(augmentation=False, mode='val', require_paired_data=require_paired_data_val, superpixel_sources='', skip_ratio=2,
                      if_sam_distillation=False, **kw)                                              # :137-157: never augmented, every 2nd sample
        return train, val

    def createDDD17EventsDataset(self, dataset_name, root, split_train, batch_size, nr_events_data, delta_t_per_data, nr_events_per_data,
                                 augmentation, event_representation, nr_bins_per_data, require_paired_data_train,
                                 require_paired_data_val, separate_pol, normalize_event, fixed_duration, config_option, pl_sources,
                                 superpixel_sources, skip_ratio, if_sam_distillation):
        builder = self.getDataloader(dataset_name)
        kw = dict(event_representation=event_representation, nr_events_data=nr_events_data, delta_t_per_data=delta_t_per_data,
                  nr_bins_per_data=nr_bins_per_data, separate_pol=separate_pol, normalize_event=normalize_event,
                  fixed_duration=fixed_duration, nr_events_per_data=nr_events_per_data, config_option=config_option,
                  pl_sources=pl_sources, superpixel_sources=superpixel_sources, skip_ratio=skip_ratio,
                  if_sam_distillation=if_sam_distillation)
        train = builder(root, split=split_train, augmentation=augmentation, require_paired_data=require_paired_data_train, **kw)
        val = builder(root, split='valid', augmentation=False, require_paired_data=require_paired_data_val, **kw)    # :232-250
        return train, val

    def prepare_batch(self, sample_batched, split='train'):
        """Host batch -> device batch.  A raw-event dict becomes the B x (nr_events_data*C) x H x W voxel tensor
        via ONE batched launch sequence of the HIP voxelizer (rectification, time normalisation, crop fused)."""
        s = self.settings
        first = sample_batched[0]
        if len(sample_batched) != 7:            # datasets.synthetic_events.collate emits the 7-slot layout for every dataset
            raise ValueError(f"prepare_batch expects collate's 7-slot batch, got {len(sample_batched)} items")
        rest = [hip.h2d_async(t, self.device) if torch.is_tensor(t) else t for t in sample_batched[1:]]
        if any(isinstance(t, dict) and 'png_bytes' in t for t in rest):
            self._png_batches += 1
        for i, t in enumerate(rest):            # undecoded 8-bit PNG maps (device_png): one batched GPU decode per slot, flips included
            if isinstance(t, dict) and 'png_bytes' in t:
                maps, status = hip.png_decode_gray8_batch(hip.h2d_async(t['png_bytes'], self.device), t['png_lengths'],
                                                          t['hw'][0], t['hw'][1], t['flip'])
                rest[i] = maps
                # per slot: device tensor, non-zero = that map was filled with the ignore index.  Kept (with the file names) for
                # check_png_status(), which runs off the hot path -- one .any() sync per `png_check_every` batches and at epoch end
                self._png_pending.append((i + 1, status, list(sample_batched[-1]) if isinstance(sample_batched[-1], (list, tuple)) else None))
        if isinstance(rest[1], dict) and 'aug' in rest[1]:
            # recon_sources: online_e2vid (K27): the reconstruction from the sample's events, on this stream -- the ingest stream
            rest[1] = self.reconstruct_online(rest[1], split)
        ds = self._voxel_ds[split]
        if isinstance(first, dict) and 'events_list' in first:            # DDD17: int64 [N,4] rows per sample
            first = ds.voxelize_batch(first['events_list'], self.device, flips=first.get('flip'))
        elif isinstance(first, dict) and 'seg_offsets' in first:          # DSEC: raw columns + explicit sub-window offsets
            first = ds.voxelize_batch(first, self.device)
        elif isinstance(first, dict):
            (H, W), crop = self.sensor_geometry
            C, nwin = s.nr_temporal_bins_b, s.nr_events_data_b
            counts = first['events_per_sample'].tolist()
            if any(n % nwin for n in counts):
                # the reference drops the remainder: nr_events_temp = nr_events_loaded // nr_events_data (sequence_ov.py:302)
                keep, base = [], 0
                for n in counts:
                    keep.append(torch.arange(base, base + (n // nwin) * nwin))
                    base += n
                keep = torch.cat(keep)
                first = {k: (v[keep] if k != 'events_per_sample' else v) for k, v in first.items()}
            offs = [0]
            for n in counts:
                per, base = n // nwin, offs[-1]
                offs.extend([base + per * (i + 1) for i in range(nwin)])
            seg = torch.tensor(offs, dtype=torch.int64)
            B = len(counts)
            dev = {k: hip.h2d_async(first[k], self.device) for k in ('x', 'y', 't', 'p')}
            seg_map = torch.zeros(B * nwin, dtype=torch.int32, device=self.device)
            vox = hip.voxelize_dsec_raw(dev['x'], dev['y'], dev['t'], dev['p'], self.rectify_maps, seg_map, seg, C, H, W,
                                        crop_rows=crop)
            first = vox.view(B, nwin * C, H - crop, W)
        else:
            first = hip.h2d_async(first, self.device)
        sp = rest[3] if len(rest) > 3 and torch.is_tensor(rest[3]) else None
        S = None
        if self.online_slic_segments and split == 'train' and getattr(s, 'if_spatial_contrastive', False):
            # superpixel_sources: online_slic (K24): SLIC of the frame the step sees (already flipped and augmented on the host), on
            # this stream -- the ingest stream, under the previous step.  Labels are 0 .. K - 1 with K from the shapes alone (with
            # online_slic_connectivity below the pass's label bound, from the shapes too), so the row count needs no read-back
            frame = first if s.config_option == 'frame2recon' else rest[1]
            sps = self.pooling_size()
            connected = bool(getattr(s, 'online_slic_connectivity', False))
            rows = online_slic_rows(frame.shape[2], frame.shape[3], self.online_slic_segments, sps, connected)
            rest[3] = hip.slic_superpixels(frame, self.online_slic_segments, enforce_connectivity=connected)
            S = (frame.shape[0] - 1) * sps + rows
        elif sp is not None and getattr(s, 'if_spatial_contrastive', False):
            # host-side row count: no device sync in the step (OpenESSModel pools with its own hard-coded size)
            sps = self.pooling_size()
            if torch.is_tensor(sample_batched[4]):
                S = int((sample_batched[4] + torch.arange(sample_batched[4].shape[0])[:, None, None] * sps).max()) + 1
            else:
                # device_png: the ids only exist on the device.  The row count is data dependent (S = max id + 1 exactly as
                # sparse_coo_tensor sizes it, pretrain_trainer.py:450-453), so one read-back is unavoidable -- it happens HERE, on
                # the ingest stream under the previous step, instead of inside the step
                off = torch.arange(0, sp.shape[0] * sps, sps, device=sp.device)[:, None, None]
                S = int((sp + off).max().item()) + 1
        return (first, *rest, S)

    # ------------------------------------------------------------------ loops (base_trainer_ov.py:358-448)
    def _epoch_loop(self, validate, single_ckpt):
        s = self.settings
        for _ in range(self.epoch_count, s.num_epochs):
            self.trainEpoch()
            if (self.epoch_count % s.val_epoch_step) == 0:
                if validate:
                    self.valEpochs()
                if s.save_checkpoint and self.rank == 0:
                    save = self.saver.save_checkpoint_model_single if single_ckpt else self.saver.save_checkpoint_model
                    save(self.models_dict, self.epoch_count, self.step_count)
            for opt in self.optimizers_dict:
                self.lr_schedulers[opt].step()
            self.epoch_count += 1

    def training(self):
        self._epoch_loop(validate=True, single_ckpt=True)

    def pretraining(self):
        self._epoch_loop(validate=False, single_ckpt=False)

    def valEpochs(self):
        self.resetValidationStatistics()
        with torch.no_grad():
            for m in self.models_dict.values():
                m.eval()
            summary = self.valEpoch(self.val_loader_sensor_b, 'sensor_b')
            self.resetValidationStatistics()
        return summary

    def valEpoch(self, data_loader, sensor_name):
        cumulative = {}
        for i_batch, sample_batched in enumerate(data_loader):
            batch = self.prepare_batch(sample_batched, 'val')
            out = self.val_step(batch[:-4], sensor_name, i_batch, -1, sample_batched[-1])
            for k, v in out[0].items():
                cumulative[k] = cumulative.get(k, 0) + v
        self.check_png_status(force=True)          # device_png: undecodable maps of the validation set raise here
        if self.world > 1 and self.metrics_semseg_b.metrics_acc is not None:      # 968-byte confusion-matrix sum
            dist.all_reduce(self.metrics_semseg_b.metrics_acc)
        metrics = self.metrics_semseg_b.get_metrics_summary()
        self.settings.logger.info('')
        for k, v in metrics.items():
            if k != 'cm':
                self.settings.logger.info(" '{}': '{:.2f}'%.".format(k, v.item()))
        self.settings.logger.info('')
        self.last_val_metrics = metrics
        return metrics
