"""Shared cases of the fp32 ViT token kernels' tests (openess_amd/csrc/vit_f32.hip: attention on the f32-input MFMA, LayerNorm on
its two routes; oess_linear_tokens_f32 of conv_f32.hip; tests/test_hip_vit_f32.py on the GPU, tests/test_vit_f32_cases.py on the
CPU) and of the CPU measurement that sets their bounds (tools/exp_maskclip_fp32_bounds.py).  The builders of
tests/vit_token_cases.py are used unchanged, their operands cast to fp32:

  * float64 references (vit_token_cases.attention64 and layer_norm64, gelu64 here);
  * an fp32 CPU model of the attention kernel's rounding points, written from the header of vit_f32.hip and not by calling it
    (attention_model_f32), with the three one-line mutations the exact cases are there to catch; an fp32 model of the LayerNorm
    kernels' summation order (layer_norm_model_f32, with the one-pass variance the large-mean families are there to fail); the
    token GEMM's k-ordered fp32 chain (linear_chain_f32);
  * the case lists, and the bounds as 4.0 * FIGURE constants: a FIGURE is what the model or torch fp32 shows against float64 on
    the CPU; nothing a kernel produced went into one.

Nothing here needs a GPU."""
import functools
import math

import torch
import torch.nn.functional as F

from tests import vit_token_cases as vc

SCALE, AK, NAN_TAIL_ROWS, SENTINEL = vc.SCALE, vc.AK, vc.NAN_TAIL_ROWS, vc.SENTINEL
ATT_L, ATT_BH, ATT_FULL = vc.ATT_L, vc.ATT_BH, vc.ATT_FULL
ATT_STRIDE_L, ATT_STRIDE_BH = vc.ATT_STRIDE_L, vc.ATT_STRIDE_BH
ATT_STRIDE_EXTRA = 4              # floats: qkv row stride 3 C + 4 keeps the rows 16-byte aligned
ATT_OUT_COLS = 64                 # out is the leading C columns of a [B L, C + 64] sentinel-filled buffer
ATT_BOUNDED_L, ATT_BOUNDED_FAMILIES = vc.ATT_BOUNDED_L, vc.ATT_BOUNDED_FAMILIES
MUTATIONS = ("mask_gt", "natural_v_rows", "no_zero_fill")

# ---- LayerNorm
LN_EPS = vc.LN_EPS
LN_C = (1, 4, 63, 64, 65, 100, 768, 772, 2044, 2047, 2048)
LN_ROWS = vc.LN_ROWS                                  # the kernels have no grid-stride loop: one wave per row
LN_FAMILIES = vc.LN_FAMILIES
# (C, layout, route): vit_token_cases.LN_CASES re-expressed for 4-float vectors (place_layernorm)
LN_CASES = ([(C, "dense", "vec" if C % 4 == 0 else "scalar") for C in LN_C] +
            [(768, "x_stride_769", "scalar"), (768, "y_stride_770", "scalar"), (768, "gamma_offset_1", "scalar"),
             (768, "beta_offset_1", "scalar"), (768, "strides_772_776", "vec"), (4, "strides_772_776", "vec")])

# ---- token GEMM
LIN_ROWS = (1, 127, 129, 257, 300)
LIN_CIN = (16, 24, 768)
LIN_COUT = (11, 40, 64, 96)

# ---- tower (tests/test_hip_maskclip_fp32.py): (img_size, image, B)
TOWER_CASES = (((32, 32), (48, 80), 2), ((32, 48), (40, 70), 2), ((32, 48), (100, 150), 1))
TOWER_MARGIN = 1e-4               # argmax is compared where the top-two margin is >= this fraction of max |logit|
TOWER_LEFT_OUT_CAP = 0.01

# ---- figures: the largest value of each measure on the CPU (tools/exp_maskclip_fp32_bounds.py prints them, tests/test_vit_f32_cases.py
# re-measures the kernel-level ones and holds them to these constants), and the bounds, four times them
ATT_FIGURES = {  # (family, L): attention_model_f32 against float64
               ("randn1.5", 9): 5.707e-07, ("randn1.5", 65): 1.150e-06, ("randn1.5", 129): 1.431e-06, ("randn1.5", 257): 1.628e-06, ("randn1.5", 1121): 1.948e-06,
               ("randn4", 9): 3.144e-06, ("randn4", 65): 8.206e-06, ("randn4", 129): 1.577e-05, ("randn4", 257): 1.275e-05, ("randn4", 1121): 1.525e-05,
               ("ascending", 9): 1.015e-07, ("ascending", 65): 6.948e-07, ("ascending", 129): 7.535e-07, ("ascending", 257): 1.754e-06, ("ascending", 1121): 1.000e-05,
               ("descending", 9): 1.185e-07, ("descending", 65): 4.896e-07, ("descending", 129): 1.066e-06, ("descending", 257): 2.179e-06, ("descending", 1121): 1.102e-05,}
LN_FIGURES = {"randn": 1.19e-7, "large_mean": 1.51e-7, "large_mean_sparse": 1.61e-7, "constant": 0.0, "single": 1.20e-7}
GELU_FIGURE = 2.39e-7
TOWER_LOGIT_FIGURES = (6.49e-7, 8.02e-7, 8.46e-7)
TOWER_VMAP_FIGURES = (7.88e-7, 6.02e-7, 7.68e-7)
ATT_BOUNDS = {f: 4.0 * v for f, v in ATT_FIGURES.items()}
LN_BOUNDS = {f: 4.0 * v for f, v in LN_FIGURES.items()}
GELU_BOUND = 4.0 * GELU_FIGURE
TOWER_LOGIT_BOUNDS = tuple(4.0 * v for v in TOWER_LOGIT_FIGURES)
TOWER_VMAP_BOUNDS = tuple(4.0 * v for v in TOWER_VMAP_FIGURES)

_gen = vc._gen
embed, split_heads, attention64, attention_err = vc.embed, vc.split_heads, vc.attention64, vc.attention_err
exact_shapes = vc.exact_shapes


# --------------------------------------------------------------------------------------------- attention cases
@functools.lru_cache(maxsize=None)
def exact_case(family, B, L, heads):
    """selection_case / constant_v_case of vit_token_cases with the operands and the expectation cast to fp32.  Selection: the
    other weights are < e^-30, far below half an fp32 ulp of |v| >= 0.5.  Constant V: L w and L are exact in fp32 and the
    division returns w."""
    c = vc.EXACT_CASES[family](B, L, heads)
    return {"qkv": c["qkv"].float(), "expect": c["expect"].float(), "B": B, "L": L, "heads": heads}


@functools.lru_cache(maxsize=None)
def bounded_case(family, L):
    """vit_token_cases.bounded_case drawn in fp32 and NOT rounded to bf16: randn 1.5 / randn 4, and keys ordered so that every
    query's best score of a 64-key tile rises (every tile rescales) or falls from tile to tile (asserted in float64)."""
    B, L, heads = vc.bounded_shape(L)
    C = heads * 64
    if family.startswith("randn"):
        g = _gen("bounded_f32", family, L)
        return {"qkv": torch.randn(B * L, 3 * C, generator=g) * float(family[5:]), "B": B, "L": L, "heads": heads}
    tile = torch.arange(L) // AK
    if family == "descending":
        tile = tile.flip(0)
    ntiles = (L + AK - 1) // AK
    for attempt in range(32):
        g = _gen("bounded_f32", family, L, attempt)
        u = (torch.randint(0, 2, (heads, 64), generator=g) * 2 - 1).float()
        q = 0.5 * torch.randn(B, L, heads, 64, generator=g) + 0.5 * u
        k = 0.5 * torch.randn(B, L, heads, 64, generator=g) + tile.float()[None, :, None, None] * u
        v = torch.randn(B, L, heads, 64, generator=g) * 1.5
        qkv = torch.cat([t.reshape(B * L, C) for t in (q, k, v)], dim=1).contiguous()
        qh, kh, _ = split_heads(qkv.double(), B, L, heads)
        s = qh @ kh.transpose(-1, -2)
        best = torch.stack([s[..., t * AK:(t + 1) * AK].max(dim=-1).values for t in range(ntiles)], dim=-1)
        d = best[..., 1:] - best[..., :-1]
        if bool((d > 0).all()) if family == "ascending" else bool((d < 0).all()):
            return {"qkv": qkv, "B": B, "L": L, "heads": heads}
    raise AssertionError(f"no seed ordered the tile maxima: {family} L={L}")


# V row that the A lane of a k-step reads when it walks the tile in NATURAL order (rows 2 e, 2 e + 1 of a 32-key block) while
# score register e of lane half hi holds key 8 (e >> 2) + 4 hi + (e & 3): the weight of key _KEY_OF_ROW[r] lands on V row r
_KEY_OF_ROW = torch.tensor([32 * (r >> 5) + 8 * (((r & 31) >> 1) >> 2) + 4 * (r & 1) + (((r & 31) >> 1) & 3) for r in range(AK)])


def attention_model_f32(qkv, B, L, heads, scale=SCALE, mutate=None):
    """fp32 model of the kernel's rounding points (header of vit_f32.hip): keys in tiles of 64, rows past L zero-filled and their
    scores set to -inf; S in fp32; running max m; p = exp((s - m) scale) in fp32, never rounded further; p summed into l separately
    for the two half-waves (key bit 2) and joined at the end; o += p V in fp32 per 32-key block; o and l rescaled by
    exp((m_old - m) scale) when the max moves; o / l by a true division.  (The kernel's products are k-ordered fma chains, torch's
    are blocked sums: the exact cases do not depend on the order, the bounded ones see it inside their factor of four.)
    mutate: 'mask_gt' masks key > L instead of key >= L; 'natural_v_rows' reads the V rows of a k-step in natural order instead of
    the order of the score registers; 'no_zero_fill' leaves the rows loaded from past L as they are (NaN behind the buffer)."""
    assert mutate is None or mutate in MUTATIONS
    q, k, v = split_heads(qkv.float(), B, L, heads)
    out = torch.empty(B, heads, L, 64)
    slot = torch.arange(AK)
    halves = [((slot >> 2) & 1) == hi for hi in (0, 1)]
    ninf = torch.tensor(-math.inf)
    for b in range(B):
        for h in range(heads):
            m = torch.full((L,), -math.inf)
            l = torch.zeros(L, 2)
            o = torch.zeros(L, 64)
            for k0 in range(0, L, AK):
                n = min(AK, L - k0)
                fill = math.nan if mutate == "no_zero_fill" else 0.0
                kt, vt = torch.full((AK, 64), fill), torch.full((AK, 64), fill)
                kt[:n], vt[:n] = k[b, h, k0:k0 + n], v[b, h, k0:k0 + n]
                s = q[b, h] @ kt.T                                                    # [L, 64] by key
                masked = (k0 + slot > L) if mutate == "mask_gt" else (k0 + slot >= L)
                s = torch.where(masked[None], ninf, s)
                m_new = torch.maximum(m, s.max(dim=1).values)
                resc = torch.exp((m - m_new) * scale)
                p = torch.exp((s - m_new[:, None]) * scale)
                l = l * resc[:, None] + torch.stack([p[:, hv].sum(dim=1) for hv in halves], dim=1)
                pa = p[:, _KEY_OF_ROW] if mutate == "natural_v_rows" else p
                o = o * resc[:, None]
                for d in range(0, AK, 32):
                    o = o + vc._mm_keep_nan(pa[:, d:d + 32], vt[d:d + 32])
                m = m_new
            out[b, h] = o / (l[:, 0] + l[:, 1])[:, None]
    return out.permute(0, 2, 1, 3).reshape(B * L, heads * 64)


# --------------------------------------------------------------------------------------------- LayerNorm
def layernorm_route(C, x_row_stride, y_row_stride, *addresses):
    """the dispatch of oess_layernorm_f32 restated: 16-byte accesses need C % 4 == 0, both row strides % 4 == 0 (floats) and the
    four pointers (x, y, gamma, beta; byte addresses) 16-byte aligned"""
    assert len(addresses) == 4
    vec = C % 4 == 0 and x_row_stride % 4 == 0 and y_row_stride % 4 == 0 and all(a % 16 == 0 for a in addresses)
    return "vec" if vec else "scalar"


def layernorm_inputs(C, rows, family):
    """the families of vit_token_cases.layernorm_inputs drawn in fp32 (not rounded to bf16, except where the family is made of
    bf16 values: constant, single): x [rows, C], gamma in [0.5, 1.5), beta ~ 0.1 randn"""
    g = _gen("layernorm_f32", C, rows, family)
    if family == "randn":
        x = torch.randn(rows, C, generator=g)
    elif family == "large_mean":                          # row mean 100, spread 0.25: E[x^2] - mean^2 loses the variance's digits
        x = 100.0 + 0.25 * torch.randn(rows, C, generator=g)
    elif family == "large_mean_sparse":                   # 100 with one element in 16 half a unit away: sigma ~ 0.125
        step = torch.randint(0, 2, (rows, C), generator=g).float() - 0.5
        x = 100.0 + step * (torch.rand(rows, C, generator=g) < 1.0 / 16.0)
    elif family == "constant":                            # variance 0: the output is beta, eps decides
        x = vc._bf16_values((rows, 1), g).float().mul(torch.tensor([1.0, 32.0])[torch.randint(0, 2, (rows, 1), generator=g)]).expand(rows, C)
    elif family == "single":                              # one non-zero element per row
        x = torch.zeros(rows, C)
        x[torch.arange(rows), torch.randint(0, C, (rows,), generator=g)] = vc._bf16_values((rows,), g).float()
    else:
        raise ValueError(family)
    return x.contiguous(), torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1


def place_layernorm(x, gamma, beta, layout, device="cpu"):
    """The operands of a case on `device` the way `layout` names: x view, gamma, beta, out view, out buffer.  Gaps of the input
    buffer hold NaN, the output buffer is prefilled with SENTINEL."""
    rows, C = x.shape
    xs = ys = C
    goff = boff = 0
    if layout == "x_stride_769":
        xs = C + 1
    elif layout == "y_stride_770":
        ys = C + 2
    elif layout == "strides_772_776":
        xs, ys = C + 4, C + 8
    elif layout == "gamma_offset_1":
        goff = 1
    elif layout == "beta_offset_1":
        boff = 1
    else:
        assert layout == "dense", layout
    xbuf = torch.full((rows, xs), math.nan, dtype=torch.float32, device=device)
    xbuf[:, :C] = x.to(device)
    ybuf = torch.full((rows, ys), SENTINEL, dtype=torch.float32, device=device)
    gbuf = torch.zeros(C + 4, device=device)
    bbuf = torch.zeros(C + 4, device=device)
    gbuf[goff:goff + C], bbuf[boff:boff + C] = gamma.to(device), beta.to(device)
    # torch reports any stride for a one-row view: as_strided pins the one the case names
    xv = torch.as_strided(xbuf, (rows, C), (xs, 1))
    yv = torch.as_strided(ybuf, (rows, C), (ys, 1))
    return xv, gbuf[goff:goff + C], bbuf[boff:boff + C], yv, ybuf


def route_of(xv, gv, bv, yv):
    xs = xv.stride(0) if xv.shape[0] > 1 else xv.shape[1]                    # what the wrapper passes for a single row
    ys = yv.stride(0) if yv.shape[0] > 1 else yv.shape[1]
    return layernorm_route(xv.shape[1], xs, ys, xv.data_ptr(), yv.data_ptr(), gv.data_ptr(), bv.data_ptr())


layer_norm64 = vc.layer_norm64


def layernorm_err(y, x, gamma, beta, eps=LN_EPS):
    """largest |y - ref64| / (|ref64| + kappa_r |gamma_c| + |beta_c|), kappa_r = max|x_r| / sigma_r with sigma_r floored by
    sqrt(eps): an error of the mean of u max|x| is u kappa in normalised units, the other roundings are relative to the terms"""
    ref = layer_norm64(x, gamma, beta, eps)
    xd, gd, bd = x.double().cpu(), gamma.double().cpu(), beta.double().cpu()
    sigma = xd.var(dim=1, unbiased=False, keepdim=True).sqrt().clamp_min(math.sqrt(eps))
    kappa = xd.abs().max(dim=1, keepdim=True).values / sigma
    den = ref.abs() + kappa * gd.abs() + bd.abs()
    return float(((y.double().cpu() - ref).abs() / den.clamp_min(1e-300)).max())


def layer_norm_model_f32(x, gamma, beta, eps=LN_EPS, route="vec", one_pass=False):
    """fp32 model of the two kernels: one wave per row, a lane adds its own channels in order (scalar route: channels lane,
    lane + 64, ...; vector route: the 4 channels of chunk lane, lane + 64, ...), the wave joins by an xor butterfly; two passes
    (mean, then squared deviations); 1 / sqrt(var + eps); (x - mean) rstd gamma + beta without contraction.
    one_pass: the variance as E[x^2] - mean^2 from the same lane sums instead -- what the large-mean families are there to fail."""
    rows, C = x.shape
    xf, gf, bf = x.float(), gamma.float(), beta.float()
    per = 4 if route == "vec" else 1
    assert route in ("vec", "scalar") and C % per == 0
    step = 64 * per
    n = (C + step - 1) // step
    pad = n * step - C
    valid = torch.cat([torch.ones(C, dtype=torch.bool), torch.zeros(pad, dtype=torch.bool)]).reshape(n, 64, per)

    def lanes(t):
        return torch.cat([t, torch.zeros(rows, pad)], dim=1).reshape(rows, n, 64, per)

    def lane_sum(t):
        s = torch.zeros(rows, 64)
        for i in range(n):
            for k in range(per):
                s = s + t[:, i, :, k]
        return vc._wave_sum(s)

    xl = lanes(xf)
    mean = lane_sum(xl) / float(C)
    if one_pass:
        var = (lane_sum(xl * xl) / float(C) - mean * mean).clamp_min(0.0)
    else:
        d = torch.where(valid[None], xl - mean[:, :, None, None], torch.zeros(()))
        var = lane_sum(d * d) / float(C)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    return (xf - mean) * rstd * gf + bf


def layernorm_torch_f32(x, gamma, beta, eps=LN_EPS):
    return F.layer_norm(x.float(), (x.shape[1],), gamma.float(), beta.float(), eps)


# --------------------------------------------------------------------------------------------- token GEMM
def linear_shapes():
    return [(r, ci, co) for r in LIN_ROWS for ci in LIN_CIN for co in LIN_COUT]


@functools.lru_cache(maxsize=None)
def linear_int_case(rows, Cin, Cout):
    """small-integer operands: every product and partial sum is an integer below 2^24, so fp32 in any order is exact"""
    g = _gen("linear_int", rows, Cin, Cout)
    x = torch.randint(-4, 5, (rows, Cin), generator=g)
    w = torch.randint(-3, 4, (Cout, Cin), generator=g)
    b = torch.randint(-50, 51, (Cout,), generator=g)
    r = torch.randint(-50, 51, (rows, Cout), generator=g)
    assert Cin * 12 + 100 < (1 << 24)
    return {"x": x.float(), "w": w.float(), "b": b.float(), "r": r.float(), "y": (x @ w.T).float(), "y_br": (x @ w.T + b + r).float()}


@functools.lru_cache(maxsize=None)
def linear_gelu_case(rows, Cin, Cout):
    g = _gen("linear_gelu", rows, Cin, Cout)
    return {"x": torch.randn(rows, Cin, generator=g), "w": torch.randn(Cout, Cin, generator=g) / math.sqrt(Cin),
            "b": torch.randn(Cout, generator=g) * 0.5, "r": torch.randn(rows, Cout, generator=g)}


def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v * math.sqrt(0.5)))


def linear_gelu_err(y, c, with_br):
    """largest |y - gelu64(v64)| / (sum_k |x_k w_k| + |b| + |r| + |gelu64|): GELU's slope is at most 1.13, so an error of the
    pre-activation passes through nearly unchanged and is relative to the magnitudes summed"""
    x, w = c["x"].double(), c["w"].double()
    v = x @ w.T
    mag = x.abs() @ w.abs().T
    if with_br:
        v = v + c["b"].double() + c["r"].double()
        mag = mag + c["b"].double().abs() + c["r"].double().abs()
    ref = gelu64(v)
    return float(((y.double().cpu() - ref).abs() / (mag + ref.abs())).max())


def linear_chain_f32(c, with_br):
    """the kernel's arithmetic on the CPU: a k-ordered fp32 chain per output (product and sum rounded separately here, fused in
    the MFMA: no more accurate than it), then bias, residual and the fp32 erf GELU"""
    x, w = c["x"], c["w"]
    acc = torch.zeros(x.shape[0], w.shape[0])
    for k in range(x.shape[1]):
        acc = acc + x[:, k:k + 1] * w[None, :, k]
    if with_br:
        acc = acc + c["b"]
        acc = acc + c["r"]
    return 0.5 * acc * (1.0 + torch.erf(acc * 0.70710678))


# --------------------------------------------------------------------------------------------- tower
def tower_pair(img_size, K=11, seed=0, mirror=True):
    """the oracle - mirror pair of tests/test_hip_maskclip.py::_pair (same seeds, same fills); mirror=False: the oracle alone (CPU)"""
    from oracle.maskclip import maskClipFeatureExtractor as Oracle
    torch.manual_seed(seed)
    o = Oracle(K, img_size=img_size)
    with torch.no_grad():
        for n, p in o.named_parameters():
            if n.endswith('cls_token') or n.endswith('pos_embed'):
                p.normal_(0, 0.3)
            elif 'ln' in n and n.endswith('weight'):
                p.uniform_(0.7, 1.3)
            elif n.endswith('bias'):
                p.normal_(0, 0.1)
        o.decoder.text_embeddings.copy_(torch.nn.functional.normalize(torch.randn(K, 512), dim=1))
    if not mirror:
        return o.eval(), None
    from openess_amd.models.maskclip_model import maskClipFeatureExtractor as Mirror
    m = Mirror(text_categories=K, img_size=img_size)
    assert list(m.state_dict().keys()) == list(o.state_dict().keys())
    m.load_state_dict(o.state_dict())
    return o.eval(), m.cuda().eval()


def tower_image(case):
    _, hw, B = TOWER_CASES[case]
    torch.manual_seed(5)
    return torch.rand(B, 3, *hw)


@functools.lru_cache(maxsize=None)
def tower_reference(case):
    """(oracle, image, float64 logits, float64 v_map) of a tower case, computed once"""
    import copy
    o, _ = tower_pair(TOWER_CASES[case][0], mirror=False)
    img = tower_image(case)
    o64 = copy.deepcopy(o).double()
    with torch.no_grad():
        ref = o64(img.double())
        _, v = o64.encoder(img.double())
    return o, img, ref, v


def rel_max(x, ref):
    """max|d| / max|ref64|"""
    return float((x.double().cpu() - ref).abs().max() / ref.abs().max())


def argmax_check(logits, ref):
    """(pixels that disagree among those whose float64 top-two margin is >= TOWER_MARGIN of the largest |logit|, fraction left out)"""
    top = ref.topk(2, dim=1).values
    keep = (top[:, 0] - top[:, 1]) >= TOWER_MARGIN * ref.abs().max()
    bad = (logits.argmax(1).cpu() != ref.argmax(1)) & keep
    return int(bad.sum()), 1.0 - float(keep.double().mean())
