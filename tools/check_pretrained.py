#!/usr/bin/env python3
"""The check to run before a long job: do the pretrained weights the YAML names load, and do they run on these kernels?

Resolves the three sources the way the trainers do (openess_amd/training/pretrained.py) -- the E2VID front end
(`e2vid_checkpoint`, else path_to_model), the image teacher (`image_weights` from `image_weights_path`, else
weights/<image_weights>.pt) and the DeepLabv3 student's `pre_trained_backbone` -- and prints one JSON line per network:
  key / file / found        the YAML key, the file it names (null: the YAML names none) and whether it exists
  missing / unexpected      keys of a non-strict load (the trainers load strictly: both must be empty for a run to start)
  tensors / parameters      what the file brought
  bf16 / fp32               {finite, mean, std} of one forward on a seeded input in either arithmetic: the E2VID latents of one
                            event window from empty states (all levels, concatenated), the teacher's features (train-mode
                            BatchNorm, as the trainers run it, on a copy per precision), the DeepLabv3 logits (eval mode)
  rel_rms                   |bf16 - fp32|_rms / |fp32|_rms
A file that is named and absent prints found: false and runs nothing (with `require_pretrained: True` it is the trainers'
FileNotFoundError).  Real weights meet the bf16 kernels here first: a range problem shows as finite: false or a large rel_rms.

    python tools/check_pretrained.py --settings FILE [--height 64] [--width 96] [--batch 2]"""
import argparse
import copy
import json
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openess_amd.config.settings import Settings  # noqa: E402
from openess_amd.training import pretrained  # noqa: E402


def _stats(t):
    t = t.double()
    return {"finite": bool(torch.isfinite(t).all()), "mean": float(t.mean()), "std": float(t.std())}


def _compare(res, bf16, fp32):
    bf16, fp32 = bf16.double().reshape(-1), fp32.double().reshape(-1)
    res["bf16"], res["fp32"] = _stats(bf16), _stats(fp32)
    res["rel_rms"] = float(((bf16 - fp32).pow(2).sum() / fp32.pow(2).sum()).sqrt())
    return res


def _load(res, module, state_dict):
    state_dict = dict(state_dict)
    bad = module.load_state_dict(state_dict, strict=False)
    res["missing"], res["unexpected"] = sorted(bad.missing_keys), sorted(bad.unexpected_keys)
    res["tensors"], res["parameters"] = len(state_dict), sum(int(v.numel()) for v in state_dict.values())


def check_e2vid(s, B, H, W, device, gen):
    from openess_amd.e2vid.image_reconstructor import ImageReconstructor
    from openess_amd.e2vid.model.model import E2VIDRecurrent
    key, path = pretrained.e2vid_path(s)
    res = {"network": "e2vid", "key": key, "file": path, "found": os.path.isfile(path)}
    source = pretrained.e2vid_source(path, key, s.nr_temporal_bins_b, True, s.require_pretrained)     # fp32 runs below too
    if source is None:
        return res
    config, state_dict = source
    model = E2VIDRecurrent(config)
    _load(res, model, state_dict)
    model.to(device).eval()
    ev = torch.randn(B, model.num_bins, H, W, generator=gen) * (torch.rand(B, model.num_bins, H, W, generator=gen) > 0.7)
    ev = ev.to(device).contiguous()
    out = {}
    for precision in ("bf16", "fp32"):
        rec = ImageReconstructor(model, H, W, model.num_bins, device, SimpleNamespace(precision=precision))
        _, _, latent = rec.update_reconstruction(ev, **({"latents_only": True} if precision == "fp32" else {}))
        out[precision] = torch.cat([latent[k].float().reshape(-1) for k in sorted(latent)])
    return _compare(res, out["bf16"], out["fp32"])


def check_teacher(s, B, H, W, device, gen):
    from openess_amd.models.image_model import DilationFeatureExtractor, adapt_weights
    name, given = getattr(s, "image_weights", None), getattr(s, "image_weights_path", None)
    if name in pretrained.NO_WEIGHTS:
        return {"network": "teacher", "key": "image_weights", "file": None, "found": False}
    path = pretrained.teacher_path(name, given, s.require_pretrained)
    res = {"network": "teacher", "key": "image_weights_path" if given else "image_weights", "image_weights": name,
           "file": path or given or os.path.join("weights", f"{name}.pt"), "found": path is not None}
    if path is None:
        return res
    net = DilationFeatureExtractor(None)
    weights = adapt_weights(name, path)
    weights.pop("fc.weight", None), weights.pop("fc.bias", None)          # as ResNetEncoder.load_state_dict
    _load(res, net.encoder, weights)
    net.to(device).train()
    nets = {"bf16": net, "fp32": copy.deepcopy(net)}                      # separate running statistics
    img = torch.rand(B, 3, H, W, generator=gen).to(device)
    with torch.no_grad():
        return _compare(res, nets["bf16"](img), nets["fp32"].forward_fp32(img))


def check_deeplab(s, B, H, W, device, gen):
    from openess_amd.models.deeplabv3 import deeplabv3_resnet50
    named = s.pretrained_backbone
    if not named:
        return {"network": "deeplabv3", "key": "pre_trained_backbone", "file": None, "found": False}
    path = pretrained.backbone_path(named, s.require_pretrained)
    res = {"network": "deeplabv3", "key": "pre_trained_backbone", "file": named, "found": bool(path)}
    if not path:
        return res
    net = deeplabv3_resnet50(num_classes=s.semseg_num_classes, text_embeddings_path='', output_stride=s.output_stride,
                             pretrained_backbone='')
    _load(res, net, torch.load(path, map_location='cpu')['model_recon'])
    net.to(device).eval()
    img = torch.rand(B, 3, H, W, generator=gen).to(device)
    with torch.no_grad():
        return _compare(res, net(img)[0], net.forward_fp32(img)[0])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--settings", required=True, help="the training YAML")
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=96)
    ap.add_argument("--batch", type=int, default=2)
    a = ap.parse_args(argv)
    if a.height % 32 or a.width % 32:
        ap.error("height and width must be multiples of 32 (DeepLabv3's output stride)")
    s = Settings(a.settings, generate_log=False)
    device = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator().manual_seed(1205)
    results = []
    for check in (check_e2vid, check_teacher, check_deeplab):
        results.append(check(s, a.batch, a.height, a.width, device, gen))
        print(json.dumps(results[-1]))
    return results


if __name__ == "__main__":
    main()
