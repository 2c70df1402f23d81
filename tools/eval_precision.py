#!/usr/bin/env python3
"""bf16 versus fp32 validation of the segmentation networks: builds the fine-tune trainer from a settings
file, optionally loads a checkpoint, and runs the validation split twice from the same weights -- the bf16 kernels the trainers
validate with by default, and the fp32 path: E2VID and SemSegE2VID in fp32 (`eval_precision: fp32`; frame2voxel, recon2voxel) or
DeepLabv3-R50 in fp32 (--config-option frame2recon).  Prints one JSON line:

  bf16 / fp32:      mIoU and accuracy (per cent) of each path,
  argmax_agreement: share of labelled pixels on which the two paths predict the same class (all of them, no margin filter),
  logits_rel_rms:   RMS of (bf16 logits - fp32 logits) over RMS of the fp32 logits,
  bf16_ms / fp32_ms: milliseconds per validation batch (HIP events, the first --warmup batches excluded).

    python tools/eval_precision.py [--settings tests/configs/finetune_dsec_synthetic.yaml] [--checkpoint FILE] [--batches N]
                                   [--config-option frame2voxel | recon2voxel | frame2recon]

Random-initialised weights (no checkpoint) give near-tied logits, so their agreement figure says little about a trained
network; the figure that matters is the one from a trained checkpoint."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import train  # noqa: E402
from openess_amd.config.settings import Settings  # noqa: E402
from openess_amd.evaluation.metrics import MetricsSemseg  # noqa: E402

DEFAULT = os.path.join(ROOT, "tests", "configs", "finetune_dsec_synthetic.yaml")


def build(settings_file, checkpoint=None, config_option='frame2voxel', ckpt_dir=None):
    train.seed_everything()
    s = Settings(settings_file, generate_log=False)
    s.config_option = config_option
    s.if_finetuning, s.if_supervised_only = True, False
    # the event networks build their fp32 reconstructor under the key; frame2recon needs none (val_logits(..., 'fp32') runs
    # deeplabv3_resnet50.forward_fp32 on any trainer) and its trainer refuses the key
    s.eval_precision = 'bf16' if config_option == 'frame2recon' else 'fp32'
    if ckpt_dir is not None:
        s.ckpt_dir = ckpt_dir
    if checkpoint:
        s.resume_training, s.resume_ckpt_file = True, checkpoint
    trainer, _ = train.build_trainer(s)
    return trainer, s


def evaluate(trainer, s, batches=None, warmup=1):
    K, ignore = s.semseg_num_classes, s.semseg_ignore_label
    met = {p: MetricsSemseg(K, ignore, s.semseg_class_names) for p in ('bf16', 'fp32')}
    ms = {'bf16': 0.0, 'fp32': 0.0}
    agree = torch.zeros(2, dtype=torch.float64, device=trainer.device)           # agreeing, labelled
    sq = torch.zeros(2, dtype=torch.float64, device=trainer.device)              # |bf16 - fp32|^2, |fp32|^2
    timed = n = 0
    with torch.no_grad():
        for m in trainer.models_dict.values():
            m.eval()
        for i, sample in enumerate(trainer.val_loader_sensor_b):
            if batches is not None and i >= batches:
                break
            batch = trainer.prepare_batch(sample, 'val')[:-4]
            gt, logits, ev = batch[1], {}, {}
            for p in ('bf16', 'fp32'):
                ev[p] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[p][0].record()
                logits[p] = trainer.val_logits(batch, p)
                ev[p][1].record()
                met[p].update_batch(logits[p].argmax(dim=1), gt)
            a, b = logits['bf16'].argmax(dim=1), logits['fp32'].argmax(dim=1)
            lab = gt != ignore
            agree += torch.stack([((a == b) & lab).sum(), lab.sum()]).double()
            d = logits['bf16'].double() - logits['fp32'].double()
            sq += torch.stack([(d * d).sum(), (logits['fp32'].double() ** 2).sum()])
            torch.cuda.synchronize()
            if i >= warmup:
                timed += 1
                for p in ms:
                    ms[p] += ev[p][0].elapsed_time(ev[p][1])
            n += 1
    out = {"metric": "eval_precision", "batches": n, "timed_batches": timed}
    for p in ('bf16', 'fp32'):
        summary = met[p].get_metrics_summary()
        out[p] = {"miou": float(summary['miou']), "acc": float(summary['acc'])}
        out[p + "_ms"] = round(ms[p] / timed, 3) if timed else None
    agree, sq = agree.cpu(), sq.cpu()
    out["labelled_pixels"] = int(agree[1])
    out["argmax_agreement"] = float(agree[0] / agree[1].clamp(min=1))
    out["logits_rel_rms"] = float((sq[0] / sq[1].clamp(min=1e-300)).sqrt())
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default=DEFAULT)
    ap.add_argument("--checkpoint", default=None, help="checkpoint written by the trainers' saver (default: seeded random weights)")
    ap.add_argument("--config-option", default="frame2voxel", choices=("frame2voxel", "recon2voxel", "frame2recon"))
    ap.add_argument("--batches", type=int, default=None, help="stop after this many validation batches (default: the whole split)")
    ap.add_argument("--warmup", type=int, default=1, help="batches left out of the timing")
    a = ap.parse_args(argv)
    trainer, s = build(a.settings, a.checkpoint, a.config_option)
    out = evaluate(trainer, s, a.batches, a.warmup)
    out["settings"] = os.path.relpath(a.settings, ROOT) if os.path.abspath(a.settings).startswith(ROOT) else a.settings
    out["checkpoint"] = a.checkpoint
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
