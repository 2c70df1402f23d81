#!/usr/bin/env python3
"""Golden vectors for SURVEY row f4 (E2VID post-processing), produced by RUNNING the reference's own code on the CPU:
  * `PostProcessor.process`   e2vid/image_reconstructor.py:126-140
    = UnsharpMaskFilter (e2vid/utils/inference_utils.py:234-252) -> IntensityRescaler (:90-129) -> ImageFilter (:255-272, off)
  * `gkern`                   e2vid/utils/inference_utils.py:38-46
Import stubs and the no-op CudaTimer: those of gen_golden_e2vid_pre.py (absent third-party modules only; the reference files run
unmodified).

Every case is a sequence of T calls on ONE PostProcessor (T = 1 for fixed bounds):
  case_<name>_in      fp32 [T, N, 1, H, W]   frames handed to process()
  case_<name>_opts    float64 [6]            unsharp_mask_amount, unsharp_mask_sigma, Imin, Imax, auto_hdr, auto_hdr_median_filter_size
  case_<name>_u8      uint8 [T, N, H, W]     the bytes behind the returned byte / 255
  case_<name>_bounds  float64 [T, 2]         the rescaler's (Imin, Imax) after each call
  gkern_sigma, gkern_w                       gkern(5, sigma) for the sigmas used
Run:  python tests/golden/gen_golden_e2vid_post.py"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden_e2vid_pre import _NoTimer, install_stubs  # noqa: E402

# name -> (amount, sigma, Imin, Imax, auto_hdr, filter_size, T, N, H, W, frame kind)
CASES = {
    "a03_s10": (0.3, 1.0, 0.0, 1.0, 0, 10, 1, 1, 37, 53, "noise"),
    "a03_s06": (0.3, 0.6, 0.0, 1.0, 0, 10, 1, 1, 37, 53, "noise"),
    "a03_s25": (0.3, 2.5, 0.0, 1.0, 0, 10, 1, 1, 37, 53, "noise"),
    "a0_s10": (0.0, 1.0, 0.0, 1.0, 0, 10, 1, 1, 37, 53, "noise"),
    "a0_s25": (0.0, 2.5, 0.0, 1.0, 0, 10, 1, 1, 37, 53, "noise"),
    "a1_s10": (1.0, 1.0, 0.0, 1.0, 0, 10, 1, 1, 37, 53, "noise"),
    "a1_s06": (1.0, 0.6, 0.0, 1.0, 0, 10, 1, 1, 37, 53, "noise"),
    "a1_s25": (1.0, 2.5, 0.0, 1.0, 0, 10, 1, 1, 37, 53, "noise"),
    "bounds_a03": (0.3, 1.0, 0.1, 0.85, 0, 10, 1, 1, 37, 53, "noise"),
    "bounds_a1_s25": (1.0, 2.5, 0.1, 0.85, 0, 10, 1, 1, 37, 53, "noise"),
    "small_5x7": (0.3, 1.0, 0.0, 1.0, 0, 10, 1, 1, 5, 7, "noise"),
    "small_5x7_bounds": (1.0, 0.6, 0.1, 0.85, 0, 10, 1, 1, 5, 7, "noise"),
    "n2": (0.3, 1.0, 0.0, 1.0, 0, 10, 1, 2, 37, 53, "noise"),
    "hdr_f10": (0.3, 1.0, 0.0, 1.0, 1, 10, 14, 1, 37, 53, "smooth"),
    "hdr_f3": (0.3, 1.0, 0.0, 1.0, 1, 3, 14, 1, 37, 53, "smooth"),
    "hdr_f0": (0.3, 1.0, 0.0, 1.0, 1, 0, 14, 1, 37, 53, "smooth"),
    "hdr_f3_n2": (0.3, 1.0, 0.0, 1.0, 1, 3, 8, 2, 37, 53, "smooth"),
    "hdr_f10_a0": (0.0, 1.0, 0.0, 1.0, 1, 10, 14, 1, 37, 53, "smooth"),
}
GKERN_SIGMAS = (0.5, 0.6, 1.0, 2.5)


def frames(rng, kind, T, N, H, W):
    """noise: uniform [-0.2, 1.2] (exercises the clamp).  smooth: low-frequency frames spanning [lo, hi] with lo in (0.05, 0.4) and
    hi in (0.6, 0.8), so that the sharpened min / max fall inside the auto-HDR clip ranges and the medians move from call to call.
    Values are multiples of 2^-12 (the fixture compresses 2x better; the arithmetic under test is unchanged)."""
    if kind == "noise":
        return np.round(rng.uniform(-0.2, 1.2, (T, N, 1, H, W)) * 4096).astype(np.float32) / 4096
    yy, xx = np.meshgrid(np.arange(H) / max(H - 1, 1), np.arange(W) / max(W - 1, 1), indexing="ij")
    out = np.empty((T, N, 1, H, W), np.float32)
    for t in range(T):
        for n in range(N):
            fx, fy, ph = rng.uniform(0.5, 1.5), rng.uniform(0.5, 1.5), rng.uniform(0, 2 * np.pi)
            u = 0.5 + 0.5 * np.sin(2 * np.pi * (fx * xx + fy * yy) + ph)
            u = (u - u.min()) / (u.max() - u.min())
            lo, hi = rng.uniform(0.05, 0.4), rng.uniform(0.6, 0.8)
            out[t, n, 0] = lo + (hi - lo) * u + rng.normal(0, 0.002, (H, W))
    return np.round(out * 4096) / 4096


def main():
    install_stubs()
    import e2vid.image_reconstructor as ir
    import e2vid.utils.inference_utils as iu
    iu.CudaTimer = ir.CudaTimer = _NoTimer
    torch.set_num_threads(4)
    rng = np.random.default_rng(1209)
    out = {"gkern_sigma": np.array(GKERN_SIGMAS, np.float64),
           "gkern_w": np.stack([iu.gkern(5, s).numpy() for s in GKERN_SIGMAS]).astype(np.float32),
           "cases": np.array(list(CASES))}
    for name, (a, s, imin, imax, auto, fsize, T, N, H, W, kind) in CASES.items():
        opts = SimpleNamespace(unsharp_mask_amount=a, unsharp_mask_sigma=s, Imin=imin, Imax=imax, auto_hdr=bool(auto),
                               auto_hdr_median_filter_size=fsize, bilateral_filter_sigma=0.0)
        post = ir.PostProcessor(torch.device("cpu"), opts)
        x = frames(rng, kind, T, N, H, W)
        u8 = np.empty((T, N, H, W), np.uint8)
        bounds = np.empty((T, 2), np.float64)
        for t in range(T):
            f = post.process(torch.from_numpy(x[t].copy())).numpy()
            b = np.rint(f * 255.0).astype(np.uint8)
            assert np.array_equal((torch.from_numpy(b).float() / 255).numpy(), f), name
            u8[t] = b[:, 0]
            bounds[t] = float(post.intensity_rescaler.Imin), float(post.intensity_rescaler.Imax)
        out[f"case_{name}_in"] = x
        out[f"case_{name}_opts"] = np.array([a, s, imin, imax, auto, fsize], np.float64)
        out[f"case_{name}_u8"] = u8
        out[f"case_{name}_bounds"] = bounds
        if auto:
            print(name, "Imin", np.round(bounds[:, 0], 4).tolist(), "Imax", np.round(bounds[:, 1], 4).tolist())
    path = os.path.join(HERE, "e2vid_post.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
