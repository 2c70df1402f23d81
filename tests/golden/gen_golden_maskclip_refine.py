#!/usr/bin/env python
"""Golden vectors of MaskCLIP's refinement, produced by RUNNING the reference's own code on the CPU:
`MaskClipHead.refine_output` (models/maskclip_model.py:224-250) and `TransformerEncoderLayer.forward(x, return_qkv=True)`
(:519-541), imported from /root/reference (or $OPENESS_REFERENCE) by file path and run unbound on a SimpleNamespace, in float64
and in float32.

Import stubs (absent third-party modules ONLY; the reference file runs unmodified): `mmcv`, `mmcv.utils`, `mmcv.cnn`,
`mmcv.cnn.bricks.transformer`, `mmcv.runner`, `mmseg.ops`, `mmseg.utils`, with `BaseModule = nn.Module`, `ModuleList =
nn.ModuleList`, `FFN = MultiheadAttention = nn.Module` and every other imported name None.

Inputs come from tests/maskclip_refine_cases.py (seeded); a case is redrawn with the next seed until the margins of that file
hold, so that no threshold decision can differ between float64 and float32 and NO pixel or class is left out of a comparison.
Writes tests/golden/maskclip_refine.npz: per case `output`, `k`, `thresholds`, `ref64`, `ref32`, `attempt`; once, the small last
layer's operands and its float64 keys `layer/k64`.  Data only."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
REF = os.environ.get("OPENESS_REFERENCE", "/root/reference")

from tests import maskclip_refine_cases as rc  # noqa: E402


class _Anything(types.ModuleType):
    """a stub module: the names the reference file needs as bases are classes, every other name is None"""
    _named = {"BaseModule": nn.Module, "ModuleList": nn.ModuleList, "FFN": nn.Module, "MultiheadAttention": nn.Module}

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return self._named.get(name)


def load_reference():
    for name in ("mmcv", "mmcv.utils", "mmcv.cnn", "mmcv.cnn.bricks", "mmcv.cnn.bricks.transformer", "mmcv.runner", "mmseg", "mmseg.ops",
                 "mmseg.utils"):
        sys.modules.setdefault(name, _Anything(name))
    spec = importlib.util.spec_from_file_location("ref_maskclip_model", os.path.join(REF, "models", "maskclip_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_refine(mod, output, k, pd, ks, dtype):
    ns = types.SimpleNamespace(pd_thresh=pd, ks_thresh=ks)
    with torch.no_grad():
        return mod.MaskClipHead.refine_output(ns, output.to(dtype).clone(), None if k is None else k.to(dtype).clone())


class _Identity:
    """stands in for the attention / FFN modules of the layer's OTHER branch (x itself is not what the fixture stores)"""

    def __call__(self, y, identity=None):
        return identity


def run_layer_k(mod, ops, dtype=torch.float64):
    C = rc.LAYER["C"]
    mha = nn.MultiheadAttention(C, 1, bias=True).to(dtype)
    norm1 = nn.LayerNorm(C, eps=1e-6).to(dtype)
    with torch.no_grad():
        mha.in_proj_weight.copy_(ops["in_w"]), mha.in_proj_bias.copy_(ops["in_b"])
        mha.out_proj.weight.copy_(ops["out_w"]), mha.out_proj.bias.copy_(ops["out_b"])
        norm1.weight.copy_(ops["ln1_w"]), norm1.bias.copy_(ops["ln1_b"])
    attn = _Identity()
    attn.attn = mha
    ns = types.SimpleNamespace(norm1=norm1, norm2=lambda v: v, attn=attn, ffn=_Identity())
    with torch.no_grad():
        _, q, k, v = mod.TransformerEncoderLayer.forward(ns, ops["x"].to(dtype).clone(), True)
    return k


def main():
    mod = load_reference()
    blob = {}
    for name, (K, H, W, C, pd, ks, k_bf16) in rc.CASES.items():
        for attempt in range(200):
            output, k = rc.draw(name, attempt)
            m = rc.margins(output, pd, ks)
            if rc.margins_hold(name, m):
                break
        else:
            raise AssertionError(f"{name}: no seed met the margins")
        ref64 = run_refine(mod, output, k, pd, ks, torch.float64)
        ref32 = run_refine(mod, output, k, pd, ks, torch.float32)
        assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32 and tuple(ref64.shape) == (rc.N, K, H, W)
        err32 = rc.rel_max(ref32, ref64)
        print(f"{name}: attempt {attempt}, margins {m}, reference fp32 vs float64 {err32:.3e}")
        assert err32 < 1e-5, "a threshold decision differs between the precisions"
        blob.update({f"{name}/output": output.numpy(), f"{name}/k": k.numpy(), f"{name}/thresholds": np.array([pd, ks], np.float64),
                     f"{name}/ref64": ref64.numpy(), f"{name}/ref32": ref32.numpy(), f"{name}/attempt": np.array(attempt)})
    ops = rc.layer_operands()
    blob.update({f"layer/{key}": v.numpy() for key, v in ops.items()})
    blob["layer/k64"] = run_layer_k(mod, ops).numpy()
    np.savez_compressed(rc.GOLDEN, **blob)
    print(f"wrote {rc.GOLDEN}: {os.path.getsize(rc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
