"""Offline SLIC superpixels through the GPU kernels, in the on-disk format of the reference's
data_preparation/superpixel_segmenter_dsec_slic.py:

    python tools/write_slic_superpixels.py --root DATA --num_segments 100 [--dataset DSEC|DDD17] [--batch 8] [--enforce-connectivity]
                                           [--png-encoder host|gpu]

DSEC:  every <seq>/images_aligned/left/<name>.png under DATA -> <seq>/sp_slic_rgb/left/<name>_slic_<n>.png
DDD17: every <dir>/images_aligned/<name>.png under DATA      -> <dir>/sp_slic_rgb/<name>_slic_<n>.png
uint8 grayscale PNGs of the cluster indices; files that exist are skipped.  The file-based `superpixel_sources: sp_slic_rgb` of
this project and of the reference read them.  Frames are read with Pillow and go to the GPU in batches of one size.
--enforce-connectivity appends SLIC's connectivity pass (skimage's default, which the reference's files were written with): the
labels then run up to hip.slic_connectivity_sizes' bound, about twice the centres, and a frame size whose bound exceeds the
256 values of a uint8 map is refused.  Not skimage bit for bit: fp32 arithmetic, and a component of max_size pixels or more
stays whole (hip.slic_superpixels).
--png-encoder gpu encodes the maps on the device (hip.png_encode_files) and writes the bytes as they come; host
(default) takes the maps to the host and encodes them with Pillow.  The same pixels either way."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def find_tasks(root, dataset, n):
    """[(image path, output path)] of the outputs that do not exist yet, in sorted order."""
    want = os.path.join("images_aligned", "left") if dataset == 'DSEC' else "images_aligned"
    tasks = []
    for d, dirs, files in sorted(os.walk(root)):
        dirs.sort()
        if not d.endswith(os.sep + want) and d != os.path.join(root, want):
            continue
        out_dir = os.path.join(d[:-len(want)], "sp_slic_rgb", "left") if dataset == 'DSEC' else os.path.join(d[:-len(want)], "sp_slic_rgb")
        for fn in sorted(files):
            if fn.lower().endswith(".png"):
                out = os.path.join(out_dir, fn[:-4] + f"_slic_{n}.png")
                if not os.path.exists(out):
                    tasks.append((os.path.join(d, fn), out))
    return tasks


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", required=True, help="dataset root")
    ap.add_argument("--num_segments", type=int, default=100)
    ap.add_argument("--dataset", choices=("DSEC", "DDD17"), default="DSEC")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--enforce-connectivity", action="store_true", help="append SLIC's connectivity pass (skimage's default)")
    ap.add_argument("--png-encoder", default="host", choices=("host", "gpu"), help="who encodes the PNGs: Pillow (default) or the GPU")
    args = ap.parse_args(argv)
    import torch
    from PIL import Image
    from openess_amd import hip
    if not os.path.isdir(args.root):
        raise SystemExit(f"{args.root} is not a directory")
    if not 1 <= args.num_segments <= hip.SLIC_MAX_CENTERS:
        raise SystemExit(f"--num_segments must be in 1 .. {hip.SLIC_MAX_CENTERS} (uint8 maps, {hip.SLIC_MAX_CENTERS} centres)")
    tasks = find_tasks(args.root, args.dataset, args.num_segments)
    if not tasks:
        print("No images to process. All outputs may already exist.")
        return 0
    written = 0

    def flush(batch):
        if args.enforce_connectivity:
            H, W = batch[0][0].shape[:2]
            ny, nx, _ = hip.slic_lattice(H, W, args.num_segments)
            bound = hip.slic_connectivity_sizes(H, W, ny * nx)[2]
            if bound > hip.SLIC_MAX_CENTERS:
                raise SystemExit(f"{batch[0][1]}: a {H} x {W} frame with {args.num_segments} segments can give {bound} labels after the "
                                 f"connectivity pass, more than the {hip.SLIC_MAX_CENTERS} values of a uint8 map")
        frames = torch.from_numpy(np.stack([b[0] for b in batch])).cuda(non_blocking=True)
        frames = frames.permute(0, 3, 1, 2).float() * (1.0 / 255.0)                 # a channels-last view: the kernel takes strides
        labels = hip.slic_superpixels(frames, args.num_segments, enforce_connectivity=args.enforce_connectivity)
        labels = labels.to(torch.uint8)
        if args.png_encoder == "gpu":
            for (_, out), data in zip(batch, hip.png_encode_files(labels.contiguous())):
                os.makedirs(os.path.dirname(out), exist_ok=True)
                with open(out, "wb") as f:
                    f.write(data)
            return len(batch)
        for (_, out), seg in zip(batch, labels.cpu().numpy()):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            Image.fromarray(seg).save(out)
        return len(batch)

    pending = []
    for path, out in tasks:
        img = np.asarray(Image.open(path).convert("RGB"))
        if pending and (pending[0][0].shape != img.shape or len(pending) == args.batch):
            written += flush(pending)
            pending = []
        pending.append((img, out))
    if pending:
        written += flush(pending)
    print(f"wrote {written} superpixel maps ({args.num_segments} segments) under {args.root}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
