#!/usr/bin/env python3
"""Golden vectors for the ConvGRU E2VID front end (K28), produced by running the reference's E2VIDRecurrent (imported from
/root/reference) with 'recurrent_block_type': 'convgru' and seeded weights keyed by parameter name (tests/synth.py:
fill_by_name).  Only the events, the expected outputs (compact form, tests/synth.py: compact) and the sorted state_dict key
list are stored -- no weights, no code.  Stand-alone:  python tests/golden/gen_golden_convgru.py"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(1, REF)
from tests.synth import compact, fill_by_name  # noqa: E402

CFG = {'num_bins': 5, 'skip_type': 'sum', 'recurrent_block_type': 'convgru', 'num_encoders': 3,
       'base_num_channels': 32, 'num_residual_blocks': 2, 'use_upsample_conv': False, 'norm': 'BN'}


def main():
    torch.set_num_threads(4)
    spec = importlib.util.spec_from_file_location("ref_data_util", os.path.join(REF, "datasets/data_util.py"))
    du = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(du)
    from e2vid.model.model import E2VIDRecurrent
    m = E2VIDRecurrent(CFG).eval()
    keys = sorted(m.state_dict().keys())
    fill_by_name(m, 11)
    rng = np.random.default_rng(77)                   # the G7 events of gen_golden_nets.py: seeded, masked-sparse
    B, H, W = 2, 32, 48
    ev = (rng.normal(0, 1, (B, 15, H, W)) * (rng.uniform(0, 1, (B, 15, H, W)) > 0.7)).astype(np.float32)
    states = None
    with torch.no_grad():
        for i in range(3):
            x = du.normalize_voxel_grid(torch.from_numpy(ev[:, 5 * i:5 * i + 5].copy()))
            img, states, latent = m(x, states)
    out = {"events": ev, "img": img.numpy(), "keys": np.array(keys)}
    for k, v in latent.items():
        out[f"latent{k}"] = v.numpy()
    for i, s in enumerate(states):                    # a ConvGRU state is the hidden state itself
        out[f"state{i}"] = s.numpy()
    small = {}
    for k, v in out.items():
        if k in ("events", "img", "keys") or np.asarray(v).size <= 20000:
            small[k] = v
        else:
            sub, ssum, sabs = compact(v)
            small[k + "__sub"], small[k + "__sum"], small[k + "__abs"] = sub, ssum, sabs
            small[k + "__shape"] = np.array(np.asarray(v).shape)
    path = os.path.join(HERE, "e2vid_convgru.npz")
    np.savez_compressed(path, **small)
    print("e2vid_convgru.npz:", len(small), "arrays", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
