"""float64 restatement of one ConvLSTM step (e2vid/model/submodules.py:199-214 of the reference) on given operands, in torch on
the CPU, and of the unfused gate kernel (oess_convlstm_gates_bf16) on given gates.  Tensors are in the reference's own layout:
x [B, Cx, H, W], h and the cell [B, C, H, W], Gates.weight [4C, Cx + C, k, k] over cat(x, h), bias [4C]; gate order in, remember,
out, cell.  The convolution is written out tap by tap (tests/test_convlstm_host.py holds it to torch's own).  Every function
converts its operands to float64; nothing is read from the reference tree."""
import torch


def _d(t):
    return t.detach().to('cpu', torch.float64)


def bf(t):
    """bf16 rounding, kept in fp32."""
    return t.detach().float().bfloat16().float()


def conv_same(s, w, b):
    """'same' stride-1 cross-correlation of s [B, Cin, H, W] with w [N, Cin, k, k] plus bias, in float64, one tap at a time."""
    s, w = _d(s), _d(w)
    B, Cin, H, W = s.shape
    k = w.shape[-1]
    pad = k // 2
    p = torch.zeros(B, Cin, H + 2 * pad, W + 2 * pad, dtype=torch.float64)
    p[:, :, pad:pad + H, pad:pad + W] = s
    out = _d(b).view(1, -1, 1, 1).repeat(B, 1, H, W)
    for dy in range(k):
        for dx in range(k):
            out += torch.einsum('nc,bchw->bnhw', w[:, :, dy, dx], p[:, :, dy:dy + H, dx:dx + W])
    return out


def cell_update(gates, c):
    """submodules.py:205-212 on the pre-activations `gates` [B, 4C, H, W] and the previous cell (None: zero).  (cell, hidden)."""
    gi, gr, go, gc = _d(gates).chunk(4, 1)
    cell = torch.sigmoid(gi) * torch.tanh(gc)
    if c is not None:
        cell = torch.sigmoid(gr) * _d(c) + cell
    return cell, torch.sigmoid(go) * torch.tanh(cell)


def step(x, h, c, w, b, rounded=True):
    """One step.  rounded: the operands as the bf16 kernels multiply them: x, h and the weight rounded to bf16; the bias and the
    previous cell stay fp32.  h = None and c = None: the zero-state form (the x half of the weight alone, no previous cell).
    Returns (cell, hidden) in float64."""
    q = bf if rounded else (lambda t: t)
    Cx = x.shape[1]
    if h is None:
        s, w = q(x), w[:, :Cx]
    else:
        s = torch.cat([q(x), q(h)], 1)
    return cell_update(conv_same(s, q(w), b), c)


def gates_kernel(gates, c):
    """The unfused gate kernel on given bf16 gates [B, 4C, H, W] (values exactly as stored) and the fp32 previous cell (None:
    zero).  Returns (cell, hidden) in float64."""
    return cell_update(gates, c)
