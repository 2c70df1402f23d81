"""float64 restatement of one ConvGRU step (e2vid/model/submodules.py:239-253 of the reference) on given operands, in torch on
the CPU.  Weights are in the reference's own layout: [C, Cx + C, k, k] over cat(x, h), biases [C].  Every function converts
its operands to float64; nothing is read from the reference tree."""
import torch
import torch.nn.functional as F


def _d(t):
    return t.detach().to('cpu', torch.float64)


def gates(x, h_conv, h, wu, bu, wr, br):
    """u = sigmoid(conv(cat(x, h_conv), wu) + bu), r = sigmoid(conv(cat(x, h_conv), wr) + br), r * h.  h_conv is the hidden state
    the convolution multiplies (the bf16 copy on the bf16 path), h the one the reset gate scales (the fp32 master there); the
    reference has one tensor for both.  x, h*: [B, C, H, W].  Returns (u, r * h)."""
    x, h_conv, h = _d(x), _d(h_conv), _d(h)
    s = torch.cat([x, h_conv], 1)
    pad = wu.shape[-1] // 2
    u = torch.sigmoid(F.conv2d(s, _d(wu), _d(bu), padding=pad))
    r = torch.sigmoid(F.conv2d(s, _d(wr), _d(br), padding=pad))
    return u, r * h


def blend(x, rh, h, u, wo, bo):
    """h' = h (1 - u) + tanh(conv(cat(x, rh), wo) + bo) u."""
    x, rh, h, u = _d(x), _d(rh), _d(h), _d(u)
    o = torch.tanh(F.conv2d(torch.cat([x, rh], 1), _d(wo), _d(bo), padding=wo.shape[-1] // 2))
    return h * (1 - u) + o * u


def step(x, h, wu, bu, wr, br, wo, bo, h_conv=None, round_rh=None):
    """One whole step.  h_conv: see gates (default h).  round_rh: a function applied to r * h before the out gate convolves it
    (the bf16 path stores it in bf16).  Returns (h', u, r * h as convolved)."""
    u, rh = gates(x, h if h_conv is None else h_conv, h, wu, bu, wr, br)
    if round_rh is not None:
        rh = _d(round_rh(rh))
    return blend(x, rh, h, u, wo, bo), u, rh
