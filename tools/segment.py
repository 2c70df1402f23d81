#!/usr/bin/env python3
"""Segment a validation split or an event recording with a trained stage-2/3 network: label PNGs, colour PNGs
and, on request, confidence maps, rendered by hip.segment_render from openess_amd.inference.Segmenter.

    python tools/segment.py -o OUT [--settings YAML] [--config-option frame2voxel | recon2voxel | frame2recon]
                            [--checkpoint FILE] [--precision bf16 | fp32] [--min-conf 0] [--alpha 0.5] [--max-frames N]
                            [--save-confidence] [--png-encoder host | gpu] [--tta flip] [--tta-scales 0.75,1,1.25]
                            [--split val | -i events.txt [-N EVENTS] [--skipevents N] [--stateful] [--overlay recon]]
                            [--classes "road,car|vehicle,person" | --classes FILE [--merge max | mean] [--templates single]
                            [--clip-text-checkpoint FILE] [--bpe FILE]]

  --split val (default)  the validation loader of the settings file; one file per sample, named after the sample's file_path stem.
                         Where the split has labels, the written labels feed MetricsSemseg: with --min-conf 0 the confusion matrix
                         is the one val_step accumulates over the same split (pixels ignored under --min-conf are left out).
  -i events.txt          the text format run_reconstruction reads (`width height`, then `t x y p` rows), event students only; the
                         sensor size must equal the settings' shape.  Windows of nr_events_window (or -N) events; each group of
                         nr_events_data windows becomes one event tensor (the DSEC loader's VoxelGrid per window, no rectification)
                         and one frame.  --stateful feeds one window per prediction and carries the recurrent states.
  --overlay recon        blend the colours over the E2VID image of the last window (event students).

  --png-encoder gpu      the label and colour PNGs are encoded on the device (hip.png_encode_files) and written
                         as they come; host (default): the maps cross to the host and Pillow encodes them.  The same pixels.

  --tta flip             every prediction is the mean class probability of the input and of its mirror image (DESIGN.md K39,
                         hip.ensemble_render); with --stateful the mirrored recording carries recurrent states of its own.
  --tta-scales           frame2recon: the image is also rescaled by these factors (a list holding 1; with --tta flip each scale
                         twice, at most 8 views).  Labels, mIoU and accuracy are the ensemble's.  Not with --classes.

  --classes              an open vocabulary: a comma list, or a file with one class per line; `a|b` gives one
                         class several names.  CLIP's text tower (--clip-text-checkpoint, --bpe; default: the settings' keys)
                         embeds every name under --templates.  --merge max (default): a class's value is the largest of its
                         names' logits; --merge mean: its names are pooled into one embedding.  Not for linear-probe checkpoints.
                         The split's labels are in another vocabulary: no mIoU is reported.

Writes OUT/vocabulary.json (class id, names, colour), OUT/labels/<stem>.png (8-bit class ids, 255 below --min-conf: what hip.png_decode_gray8_batch and the loaders read as
pseudo-labels), OUT/color/<stem>.png (RGB) and, with --save-confidence, OUT/confidence/<stem>.npy (float32).  Prints one JSON
line: source, frames, ms per frame by part (network and render on the device, write on the host), and mIoU / accuracy where labels
exist."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT = os.path.join(ROOT, "tests", "configs", "finetune_dsec_synthetic.yaml")
EVENT_OPTIONS = ("frame2voxel", "recon2voxel")


def build_parser():
    ap = argparse.ArgumentParser(description="Segment a validation split or an event recording")
    ap.add_argument("--settings", default=DEFAULT)
    ap.add_argument("--config-option", default="frame2voxel", choices=EVENT_OPTIONS + ("frame2recon",))
    ap.add_argument("--checkpoint", default=None, help="checkpoint written by the trainers' saver (default: the weights the trainer builds)")
    ap.add_argument("--precision", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--split", default=None, choices=("val",), help="the settings file's validation loader (the default source)")
    ap.add_argument("-i", "--input_file", default=None, help="events text file (width height / t x y p)")
    ap.add_argument("-N", "--window_size", default=None, type=int, help="events per window (default: nr_events_window)")
    ap.add_argument("--skipevents", default=0, type=int)
    ap.add_argument("--stateful", action="store_true", help="one window per prediction, recurrent states carried (-i only)")
    ap.add_argument("--overlay", default=None, choices=("recon",), help="blend the colours over the E2VID image (event students)")
    ap.add_argument("--alpha", default=0.5, type=float, help="weight of the colour in the blend")
    ap.add_argument("--min-conf", default=0.0, type=float, help="labels below this confidence become 255")
    ap.add_argument("--max-frames", default=None, type=int)
    ap.add_argument("--save-confidence", action="store_true")
    ap.add_argument("--png-encoder", default="host", choices=("host", "gpu"), help="who encodes the label and colour PNGs: Pillow (default) or the GPU")
    ap.add_argument("--classes", default=None, help="open vocabulary: comma list or file, one class per line; a|b = two names of one class")
    ap.add_argument("--merge", default=None, choices=("max", "mean"), help="several names of a class: largest logit (default) or pooled embedding")
    ap.add_argument("--templates", default=None, help="single (default), none, or a file with one template containing {} per line")
    ap.add_argument("--clip-text-checkpoint", default=None, help="CLIP weights for --classes (default: the settings' clip_text_checkpoint)")
    ap.add_argument("--bpe", default=None, help="BPE merges file for --classes (default: the settings' clip_bpe_path)")
    ap.add_argument("--tta", default=None, choices=("flip",), help="average the class probabilities with those of the mirrored input")
    ap.add_argument("--tta-scales", default=None, help="comma list of image scales holding 1, e.g. 0.75,1,1.25 (frame2recon only)")
    ap.add_argument("-o", "--output", required=True)
    return ap


def parse_tta(ap, a, s):
    """--tta / --tta-scales checked without a GPU: (flip, scales) as Segmenter.predict takes them"""
    from openess_amd.inference import tta_views
    flip, scales = a.tta == "flip", (1.0,)
    if a.tta_scales is not None:
        if a.config_option != "frame2recon":
            ap.error("--tta-scales needs --config-option frame2recon (the event students' reconstructor is built for one size)")
        try:
            scales = tuple(float(v) for v in a.tta_scales.split(","))
        except ValueError:
            ap.error(f"--tta-scales: a comma list of numbers, got {a.tta_scales!r}")
        if bool(getattr(s, "if_linear_probing", False)) and not getattr(s, "if_finetuning", False) and scales != (1.0,):
            ap.error("--tta-scales: a linear probe acts on the full-resolution logits of one size; --tta flip works")
    try:
        views = tta_views(flip, scales)
    except ValueError as e:
        ap.error(f"--tta-scales: {e}")
    if len(views) > 1 and a.classes is not None:
        ap.error("--tta / --tta-scales with --classes: the ensemble render takes no grouped classes yet (a follow-up)")
    return flip, scales, len(views)


def parse_vocabulary(ap, a, s):
    """--classes and what goes with it, checked without a GPU: None, or the keyword arguments of Segmenter.set_vocabulary"""
    given = [f for f, v in (("--merge", a.merge), ("--templates", a.templates), ("--clip-text-checkpoint", a.clip_text_checkpoint),
                            ("--bpe", a.bpe)) if v is not None]
    if a.classes is None:
        if given:
            ap.error(f"{given[0]} needs --classes")
        return None
    from openess_amd.models.clip_text import parse_classes
    try:
        classes = parse_classes(a.classes)
    except ValueError as e:
        ap.error(str(e))
    if len(classes) > 255:
        ap.error(f"--classes: at most 255 classes, got {len(classes)}")
    if bool(getattr(s, "if_linear_probing", False)) and not getattr(s, "if_finetuning", False):
        ap.error("--classes: a linear-probe checkpoint keeps its vocabulary (the probe's K x K conv is tied to the trained classes)")
    ckpt = a.clip_text_checkpoint or getattr(s, "clip_text_checkpoint", None)
    bpe = a.bpe or getattr(s, "clip_bpe_path", None)
    if not ckpt or not bpe:
        ap.error("--classes needs --clip-text-checkpoint and --bpe (or clip_text_checkpoint / clip_bpe_path in the settings file)")
    for flag, path in (("--clip-text-checkpoint", ckpt), ("--bpe", bpe)) + ((("--templates", a.templates),) if a.templates not in (None, "single", "none") else ()):
        if not os.path.isfile(path):
            ap.error(f"{flag}: file not found: {path}")
    return dict(classes=classes, merge=a.merge or "max", templates=a.templates or "single", clip_text_checkpoint=ckpt, clip_bpe_path=bpe)


def check_args(ap, a):
    """Argument errors that need no GPU and no model; returns the Settings."""
    from openess_amd.config.settings import Settings
    if a.input_file is not None and a.split is not None:
        ap.error("--split and -i name two sources: give one")
    if a.input_file is None:
        for flag, given in (("--stateful", a.stateful), ("-N", a.window_size is not None), ("--skipevents", a.skipevents != 0)):
            if given:
                ap.error(f"{flag} needs -i (an event recording)")
    if a.input_file is not None and a.config_option not in EVENT_OPTIONS:
        ap.error(f"-i serves the event students {EVENT_OPTIONS}, not {a.config_option}")
    if a.overlay == "recon" and a.config_option not in EVENT_OPTIONS:
        ap.error(f"--overlay recon needs an event student {EVENT_OPTIONS}")
    if not 0.0 <= a.alpha <= 1.0:
        ap.error("--alpha must lie in 0 ... 1")
    if not a.min_conf >= 0.0:
        ap.error("--min-conf must be >= 0")
    if a.max_frames is not None and a.max_frames < 1:
        ap.error("--max-frames must be positive")
    if a.window_size is not None and a.window_size < 1:
        ap.error("-N must be positive")
    if not os.path.isfile(a.settings):
        ap.error(f"settings file not found: {a.settings}")
    s = Settings(a.settings, generate_log=False)
    if a.input_file is not None:
        if not os.path.isfile(a.input_file):
            ap.error(f"events file not found: {a.input_file}")
        with open(a.input_file) as f:
            head = f.readline().split()
        if len(head) != 2 or not all(v.isdigit() for v in head):
            ap.error(f"{a.input_file}: the first line must be `width height`")
        width, height = int(head[0]), int(head[1])
        if [height, width] != [int(v) for v in s.img_size_b]:
            ap.error(f"{a.input_file}: sensor size {height} x {width} is not the settings' shape {list(s.img_size_b)}")
    a.tta_flip, a.tta_scale_list, a.tta_views = parse_tta(ap, a, s)
    a.vocabulary = parse_vocabulary(ap, a, s)
    return s


class Writer:
    def __init__(self, out, save_confidence, png_encoder="host"):
        self.png_encoder = png_encoder
        self.dirs = {k: os.path.join(out, k) for k in ("labels", "color") + (("confidence",) if save_confidence else ())}
        for d in self.dirs.values():
            os.makedirs(d, exist_ok=True)
        self.seconds, self.frames = 0.0, 0

    def write(self, stems, out):
        """out: the Segmenter's dict on the device; one file set per sample"""
        import numpy as np
        from PIL import Image
        t0 = time.perf_counter()
        on_gpu = self.png_encoder == "gpu"
        if on_gpu and stems:
            # the files are encoded on the device (K37); only their bytes cross, and they are written as they are
            from openess_amd import hip
            for key, sub in (('labels', 'labels'), ('rgb', 'color')):
                for stem, data in zip(stems, hip.png_encode_files(out[key].contiguous())):
                    with open(os.path.join(self.dirs[sub], stem + ".png"), "wb") as f:
                        f.write(data)
        elif not on_gpu:
            labels, rgb = out['labels'].cpu().numpy(), out['rgb'].cpu().numpy()
        conf = out['conf'].cpu().numpy() if 'confidence' in self.dirs else None
        for j, stem in enumerate(stems):
            if not on_gpu:
                Image.fromarray(labels[j]).save(os.path.join(self.dirs['labels'], stem + ".png"))
                Image.fromarray(rgb[j]).save(os.path.join(self.dirs['color'], stem + ".png"))
            if conf is not None:
                np.save(os.path.join(self.dirs['confidence'], stem + ".npy"), conf[j])
        self.seconds += time.perf_counter() - t0
        self.frames += len(stems)


def _timed(seg, fn):
    """(result, [network ms, render ms] on the device) of fn(), a call of the Segmenter's predict / predict_events"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    render = seg.render_events[0].elapsed_time(seg.render_events[1])
    return out, [e0.elapsed_time(e1) - render, render]


def _tta(a):
    """the Segmenter's flip / scales keywords; none at all without --tta / --tta-scales: the plain call as it always was"""
    return dict(flip=a.tta_flip, scales=a.tta_scale_list) if a.tta_views > 1 else {}


def run_val(seg, a, writer):
    import torch
    from openess_amd.evaluation.metrics import MetricsSemseg
    s, tr = seg.settings, seg.trainer
    # a custom vocabulary: the split's labels are in another one, nothing to score
    met = (MetricsSemseg(s.semseg_num_classes, s.semseg_ignore_label, s.semseg_class_names)
           if s.semseg_label_val_b and a.vocabulary is None else None)
    ms = [0.0, 0.0]
    for sample in tr.val_loader_sensor_b:
        if a.max_frames is not None and writer.frames >= a.max_frames:
            break
        batch = tr.prepare_batch(sample, 'val')[:-4]
        stems = [os.path.splitext(os.path.basename(str(p)))[0] for p in sample[-1]]
        want_overlay = a.overlay == "recon"
        out, dt = _timed(seg, lambda: seg.predict(batch, min_conf=a.min_conf, background='recon' if want_overlay else None, alpha=a.alpha,
                                                  **_tta(a)))
        ms = [ms[0] + dt[0], ms[1] + dt[1]]
        keep = len(stems) if a.max_frames is None else min(len(stems), a.max_frames - writer.frames)
        if met is not None and torch.is_tensor(batch[1]):
            gt, pred = batch[1][:keep], out['labels'][:keep]
            # a prediction ignored under --min-conf is no class: its pixel is left out of the confusion matrix
            met.update_batch(pred, torch.where(pred == s.semseg_ignore_label, torch.full_like(gt, s.semseg_ignore_label), gt))
        writer.write(stems[:keep], {k: v[:keep] for k, v in out.items()})
    tr.check_png_status(force=True)
    res = {"network_render_ms": ms}
    if met is not None and met.metrics_acc is not None:
        summary = met.get_metrics_summary()
        res.update(miou=float(summary['miou']), acc=float(summary['acc']), confusion=summary['cm'].tolist())
    return res


def event_tensors(path, s, window, skipevents, group, device):
    """fp32 [1, group * C, H, W] tensors of consecutive groups of `group` windows (an incomplete last group is dropped)"""
    import numpy as np
    import torch
    from openess_amd.DSEC.dataset.representations import VoxelGrid
    from openess_amd.e2vid.utils.event_readers import FixedSizeEventReader
    H, W = (int(v) for v in s.img_size_b)
    vox = VoxelGrid(s.nr_temporal_bins_b, H, W, normalize=bool(s.normalize_event_b))
    grids = []
    for ev in FixedSizeEventReader(path, num_events=window, start_index=skipevents):
        t = ev[:, 0] - ev[0, 0]
        t = t / t[-1] if t[-1] > 0 else t                       # the DSEC loader's normalisation of a window's stamps to 0 ... 1
        cols = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).to(device) for c in (ev[:, 1], ev[:, 2], ev[:, 3], t)]
        grids.append(vox.convert(*cols).reshape(-1, H, W))
        if len(grids) == group:
            yield torch.cat(grids, 0)[None].contiguous()
            grids = []


def run_events(seg, a, writer):
    s = seg.settings
    window = a.window_size if a.window_size is not None else int(s.nr_events_window_b)
    group = 1 if a.stateful else int(s.nr_events_data_b)
    ms, k = [0.0, 0.0], 0
    seg.reset()
    for ev in event_tensors(a.input_file, s, window, a.skipevents, group, seg.device):
        if a.max_frames is not None and k >= a.max_frames:
            break
        out, dt = _timed(seg, lambda: seg.predict_events(ev, stateful=a.stateful, min_conf=a.min_conf, alpha=a.alpha,
                                                    background='recon' if a.overlay == "recon" else None, **_tta(a)))
        ms = [ms[0] + dt[0], ms[1] + dt[1]]
        writer.write(['frame_{:010d}'.format(k)], out)
        k += 1
    return {"network_render_ms": ms, "events_per_window": window, "windows_per_frame": group}


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    check_args(ap, a)
    import torch
    from openess_amd.inference import Segmenter
    seg = Segmenter(a.settings, a.config_option, a.checkpoint, a.precision)
    if a.vocabulary is not None:
        seg.set_vocabulary(**a.vocabulary)
    writer = Writer(a.output, a.save_confidence, a.png_encoder)
    with open(os.path.join(a.output, "vocabulary.json"), "w") as f:
        json.dump(seg.vocabulary, f, indent=1)
    res = run_events(seg, a, writer) if a.input_file is not None else run_val(seg, a, writer)
    n = max(writer.frames, 1)
    out = {"metric": "segment", "source": a.input_file if a.input_file is not None else "val", "config_option": a.config_option,
           "precision": a.precision, "stateful": bool(a.stateful), "min_conf": a.min_conf, "frames": writer.frames,
           "ms_per_frame": {"network": round(res["network_render_ms"][0] / n, 3), "render": round(res.pop("network_render_ms")[1] / n, 3), "write": round(1e3 * writer.seconds / n, 3)},
           "output": a.output, "checkpoint": a.checkpoint, "classes": seg.num_classes,
           "vocabulary": None if a.vocabulary is None else {"merge": a.vocabulary["merge"], "templates": a.vocabulary["templates"]}, "device": torch.cuda.get_device_name(0)}
    out["tta"] = {"flip": a.tta_flip, "scales": list(a.tta_scale_list), "views": a.tta_views}
    if a.png_encoder == "gpu":
        out["png_encoder"] = "gpu"
    out.update(res)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
