"""K34: the SAM distillation loss of the frame2recon pre-training step (training/pretrain_trainer.py:481-482, 519-529), restated in
torch on the CPU, and the cases the kernel tests and tools/exp_sam_distill_bounds.py share.

    M        = max(H, W)
    sam_up   = F.interpolate(feat_sam, size=(M, M), mode='bilinear', align_corners=False)[:, :, :H, :]
    loss_sam = mean(1 - F.cosine_similarity(sam_up, feat_recon, dim=1))

`distill` is those lines on a full-resolution feature; `from_map` puts DeepLabv3's own upsampling of the stride-level map in front
(models/deeplabv3.py:184) and returns the loss, its gradient on the map by autograd, and the smallest interpolated norm of either
side.  float64 is the reference; the same code in float32 is what the test bounds are measured from."""
import functools

import torch
import torch.nn.functional as F

# (B, C, (h, w) of the student map, (H, W) of the output, (hs, ws) of the SAM map)
CASES = (
    (1, 4, (1, 1), (1, 1), (1, 1)),             # smallest
    (1, 4, (1, 1), (3, 5), (2, 2)),             # size-1 map dims, rows cropped from M = 5
    (2, 8, (3, 4), (9, 13), (5, 5)),            # non-integer scales
    (2, 12, (4, 4), (8, 8), (3, 3)),            # H == W, no crop
    (2, 256, (2, 3), (24, 32), (64, 64)),       # M = 32 < 64: the SAM map is down-sampled
    (1, 256, (4, 5), (55, 80), (64, 64)),       # the step's channel count and SAM grid
    (1, 1024, (2, 2), (4, 6), (2, 2)),          # the channel cap
)
ALIGN_CASE = 2                                  # also run with align_corners=True on the student side
MIN_NORM = 1e-3                                 # every interpolated vector is this far from the eps clamp (a condition on the inputs)
SLICE_OFFSET, SLICE_EXTRA = 8, 24               # the channel-slice variant: channels [8, 8 + C) of C + 24


def distill(sam, feat, eps=1e-8):
    """the reference's lines on a full-resolution feature [B, C, H, W]; returns (loss, sam_up)"""
    H, W = feat.shape[2:]
    M = max(H, W)
    sam_up = F.interpolate(sam, size=(M, M), mode='bilinear', align_corners=False)[:, :, :H, :]
    return torch.mean(1 - F.cosine_similarity(sam_up, feat, dim=1, eps=eps)), sam_up


def from_map(sam, amap, size, align=False, dtype=torch.float64, eps=1e-8):
    """loss, d loss / d amap, min interpolated norm; all computed in `dtype` on the CPU"""
    a = amap.detach().to('cpu', dtype).requires_grad_(True)
    feat = F.interpolate(a, size=tuple(size), mode='bilinear', align_corners=align)
    loss, sam_up = distill(sam.detach().to('cpu', dtype), feat, eps)
    loss.backward()
    norms = torch.minimum(sam_up.detach().norm(dim=1).min(), feat.detach().norm(dim=1).min())
    return loss.detach(), a.grad, float(norms)


def inputs(i, bf16=False):
    """(sam fp32, student map fp32 -- holding bf16-representable values when bf16 --, size) of case i, seeded"""
    B, C, (h, w), size, (hs, ws) = CASES[i]
    g = torch.Generator().manual_seed(3400 + i)
    amap = torch.randn(B, C, h, w, generator=g)
    sam = 1 + 0.5 * torch.randn(B, C, hs, ws, generator=g)
    if bf16:
        amap = amap.bfloat16().float()
    return sam, amap, size


@functools.lru_cache(maxsize=None)
def case(i, bf16=False, align=False):
    """the case's inputs with its float64 reference, computed once and shared; do not modify the tensors"""
    sam, amap, size = inputs(i, bf16)
    loss, grad, min_norm = from_map(sam, amap, size, align)
    assert min_norm > MIN_NORM, (i, min_norm)
    return dict(sam=sam, map=amap, size=size, align=align, loss=loss, grad=grad, min_norm=min_norm)


def variants():
    """(case index, align) pairs of the kernel tests"""
    return [(i, False) for i in range(len(CASES))] + [(ALIGN_CASE, True)]


def fp32_figures(bf16):
    """torch fp32 against float64 on every variant: (worst |loss32 - loss64|, worst max|g32 - g64| / max|g64|) and the rows"""
    rows, worst = [], [0.0, 0.0]
    for i, align in variants():
        c = case(i, bf16, align)
        loss32, grad32, _ = from_map(c['sam'], c['map'], c['size'], align, torch.float32)
        el = float((loss32.double() - c['loss']).abs())
        eg = float((grad32.double() - c['grad']).abs().max() / c['grad'].abs().max())
        rows.append((i, align, el, eg))
        worst = [max(worst[0], el), max(worst[1], eg)]
    return tuple(worst), rows
