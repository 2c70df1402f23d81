"""float64 restatement of MaskCLIP's refinement (MaskClipHead.refine_output, models/maskclip_model.py:224-250 of the reference)
and of the last encoder layer's keys (TransformerEncoderLayer.forward with return_qkv, :519-533), written from the reference's
text and held to the reference's own float64 output in tests/golden/maskclip_refine.npz by tests/test_maskclip_refine_cases.py.
Two forms of the smoothing: explicit (the L x L weight matrix) and factored (k (k^T P / n^2), what the kernels compute), and two
deliberate mutations the fixture must tell apart.  Nothing here needs a GPU."""
import torch
import torch.nn.functional as F


def refine(output, k, pd_thresh=0.5, ks_thresh=1.0, form="explicit", normalize_dim=1, dtype=torch.float64):
    """output [N, K, H, W], k [N, H W, C] or None -> the refined output, in `dtype` arithmetic.
    form: 'explicit' (k^ k^T) @ P or 'factored' k (k^T P) / n^2.  normalize_dim=2 is the mutation that normalises every token
    over its channels instead of every channel over the tokens."""
    x = torch.as_tensor(output).to(dtype).clone()
    n, K, H, W = x.shape
    if pd_thresh > 0:
        conf = torch.softmax(x * 100, dim=1).reshape(n, K, -1).max(dim=-1).values
        x[(conf < pd_thresh)[:, :, None, None].expand(n, K, H, W)] = -100
    if k is None or not ks_thresh > 0:
        return x
    p = torch.softmax(x * 100, dim=1).reshape(n, K, -1).transpose(-2, -1)              # [N, L, K]
    kd = torch.as_tensor(k).to(dtype)
    if form == "explicit":
        kn = kd / kd.norm(dim=normalize_dim, keepdim=True).clamp_min(1e-12)
        smoothed = (kn @ kn.transpose(-2, -1)) @ p
    else:
        assert form == "factored" and normalize_dim == 1
        nrm = kd.norm(dim=1, keepdim=True).clamp_min(1e-12)                            # [N, 1, C]
        smoothed = kd @ ((kd.transpose(-2, -1) @ p) / (nrm * nrm).transpose(-2, -1))
    sel = p.max(dim=-1, keepdim=True).values < ks_thresh
    return torch.where(sel, smoothed, p).transpose(-2, -1).reshape(n, K, H, W)


def last_layer_k(x, ln1_w, ln1_b, in_w, in_b, out_w, out_b, eps=1e-6, residual=False, dtype=torch.float64):
    """k = out_proj(W_k ln1(x) + b_k) + b_o for tokens x [B, T, C]: rows C:2C of in_proj, no residual (`residual=True` is the
    mutation that treats k like v) and no final norm."""
    x, ln1_w, ln1_b, in_w, in_b, out_w, out_b = (torch.as_tensor(t).to(dtype) for t in (x, ln1_w, ln1_b, in_w, in_b, out_w, out_b))
    C = x.shape[-1]
    y = F.layer_norm(x, (C,), ln1_w, ln1_b, eps)
    k = F.linear(F.linear(y, in_w[C:2 * C], in_b[C:2 * C]), out_w, out_b)
    return k + x if residual else k
