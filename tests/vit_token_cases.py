"""Shared cases of the ViT token kernels' tests (openess_amd/csrc/vit_ops.hip: LayerNorm on its two routes, the MFMA flash
attention for head dimension 64; tests/test_hip_vit_tokens.py on the GPU, tests/test_vit_token_cases.py on the CPU) and of the CPU
measurement that sets their bounds (tools/exp_vit_token_bounds.py):

  * float64 references of both operations on the bf16 operands (layer_norm64, attention64);
  * fp32 CPU models of the kernels' rounding points, written from the header of vit_ops.hip and not by calling it
    (layer_norm_model, attention_model): they prove that the exact cases below are exact for a correct implementation and
    measure how far correct bf16 / fp32 arithmetic sits from float64;
  * exact attention cases whose result is known bit for bit (selection_case, constant_v_case), float64-bounded ones
    (bounded_case) and the LayerNorm cases with the route each must take (layernorm_route restates the dispatch).

Nothing here needs a GPU."""
import functools
import math

import torch

SEED = 7411                       # every case derives its generator from this, its family and its shape
SCALE = 0.125                     # 1 / sqrt(64): the only scale hip.attention_d64 passes
AK = 64                           # keys per tile of the kernel
NAN_TAIL_ROWS = 64                # rows of NaN behind the B L rows of a qkv buffer: a tail tile reaches at most 63 rows past
SENTINEL = -24576.0               # bf16-exact; fills what a kernel must not write

# ---- attention shapes
ATT_L = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 72, 73, 127, 128, 129, 192, 193, 257)
ATT_BH = ((1, 1), (3, 2), (2, 12))
ATT_FULL = (1, 1121, 12)          # (B, L, heads): the full-size token count
ATT_STRIDE_L = (33, 129)          # with heads = 2, B = 2: qkv row stride 3 C + 8, out a column slice
ATT_STRIDE_BH = (2, 2)
ATT_BOUNDED_L = (9, 65, 129, 257, 1121)
ATT_BOUNDED_FAMILIES = ("randn1.5", "randn4", "ascending", "descending")
MIN_GAP = 30.0                    # selection: winner over runner-up, after the scale
MAX_CONST_SCORE = -40.0           # constant-V: every real score, after the scale
MUTATIONS = ("mask_gt", "identity_perm", "no_v_zero")

# ---- LayerNorm shapes
LN_EPS = 1e-6
LN_VEC_C = (8, 64, 512, 768, 2040, 2048)
LN_SCALAR_C = (1, 63, 65, 100, 772, 2047)
LN_ROWS = (1, 5, 77)
LN_FAMILIES = ("randn", "large_mean", "large_mean_sparse", "constant", "single")
LN_GRID_ROWS = 4 * 65536 + 5      # the only row count that enters the grid-stride loop (the grid is capped at 65536 blocks of 4 rows)
# (C, layout, route): layout names how the operands sit in memory (place_layernorm)
LN_CASES = ([(C, "dense", "vec") for C in LN_VEC_C] + [(C, "dense", "scalar") for C in LN_SCALAR_C] +
            [(768, "x_stride_772", "scalar"), (768, "gamma_offset_1", "scalar"), (768, "beta_offset_1", "scalar"),
             (768, "y_stride_772", "scalar"), (768, "strides_776_784", "vec"), (8, "strides_776_784", "vec")])
LN_GRID_CASES = ((8, "dense", "vec"), (7, "dense", "scalar"))

# ---- bounds: four times the largest figure of the fp32 models against float64 (tools/exp_vit_token_bounds.py prints both;
# DESIGN.md carries them; tests/test_vit_token_cases.py re-measures and holds them to the figures)
ATT_MODEL_FIGURE = 3.10e-3         # largest over the four families: randn 4 at L = 1121 (3.092e-3)
LN_MODEL_FIGURE = 1.99            # randn, scalar route, the grid-stride case (1.987): a bf16 half-ulp is up to 2^-8, twice the first term
ATT_BOUND = 4.0 * ATT_MODEL_FIGURE
LN_BOUND = 4.0 * LN_MODEL_FIGURE


def _gen(*key):
    h = SEED
    for k in key:
        for ch in str(k):
            h = (h * 1000003 + ord(ch)) % (1 << 31)
    return torch.Generator().manual_seed(h)


def _bf16_values(shape, g):
    """random bf16 values with 0.5 <= |v| < 4, never zero: sign * (128 .. 255) / 128 * 2^(-1 .. 1)"""
    mant = torch.randint(128, 256, shape, generator=g).double() / 128.0
    exp = torch.randint(-1, 2, shape, generator=g).double()
    sign = torch.randint(0, 2, shape, generator=g).double() * 2.0 - 1.0
    v = sign * mant * torch.pow(torch.tensor(2.0, dtype=torch.float64), exp)
    assert bool((v.bfloat16().double() == v).all())
    return v


def _pack_qkv(q, k, v):
    """[B, L, heads, 64] x 3 -> nn.MultiheadAttention's packed [B L, 3 C] in bf16; the values must be bf16-exact"""
    B, L, heads, _ = q.shape
    qkv = torch.cat([t.reshape(B * L, heads * 64) for t in (q, k, v)], dim=1).double()
    out = qkv.bfloat16()
    assert bool((out.double() == qkv).all())
    return out


def split_heads(qkv, B, L, heads):
    """packed [>= B L, 3 C] -> q, k, v as [B, heads, L, 64] (same dtype)"""
    C = heads * 64
    return tuple(t.reshape(B, L, heads, 64).permute(0, 2, 1, 3) for t in qkv[:B * L].split(C, dim=1))


def embed(t, extra_rows, extra_cols, fill, device=None):
    """`t` as the leading rows and columns of a larger buffer filled with `fill`: (buffer, view of t's shape).  The buffer's base
    is the allocator's (16-byte aligned and more); with extra_cols % 8 == 0 every row of the view stays 16-byte aligned."""
    device = t.device if device is None else device
    buf = torch.full((t.shape[0] + extra_rows, t.shape[1] + extra_cols), fill, dtype=t.dtype, device=device)
    buf[:t.shape[0], :t.shape[1]] = t.to(device)
    return buf, buf[:t.shape[0], :t.shape[1]]


# --------------------------------------------------------------------------------------------- exact attention cases
@functools.lru_cache(maxsize=None)
def selection_case(B, L, heads):
    """K rows are random +-4 vectors, Q[i] = 2 K[pi(i)], V random bf16 in 0.5 <= |v| < 4: every score is an exact integer, the
    winner leads by >= MIN_GAP after the scale (asserted from int64 dot products; reseeded until it holds), so every other weight
    is below e^-30 and the output is V[pi(i)] bit for bit."""
    for attempt in range(32):
        g = _gen("selection", B, L, heads, attempt)
        k = torch.randint(0, 2, (B, L, heads, 64), generator=g) * 8 - 4                        # int64
        pi = torch.stack([torch.stack([torch.randperm(L, generator=g) for _ in range(heads)]) for _ in range(B)])   # [B, heads, L]
        kh = k.permute(0, 2, 1, 3)                                                             # [B, heads, L, 64]
        qh = 2 * torch.gather(kh, 2, pi[..., None].expand(B, heads, L, 64))
        gap = None
        for b in range(B):
            for h in range(heads):
                s = qh[b, h] @ kh[b, h].T                                                      # int64 [L, L]
                win = s.gather(1, pi[b, h][:, None])[:, 0]
                assert bool((win == 2 * 64 * 16).all())
                if L > 1:
                    other = s.scatter(1, pi[b, h][:, None], torch.iinfo(torch.int64).min).max(dim=1).values
                    d = int((win - other).min())
                    gap = d if gap is None else min(gap, d)
        if gap is None or gap * SCALE >= MIN_GAP:
            break
    else:
        raise AssertionError("no seed gave the selection gap")
    v = _bf16_values((B, L, heads, 64), g)
    vh = v.permute(0, 2, 1, 3)
    expect = torch.gather(vh, 2, pi[..., None].expand(B, heads, L, 64)).permute(0, 2, 1, 3).reshape(B * L, heads * 64)
    return {"qkv": _pack_qkv(qh.permute(0, 2, 1, 3), k, v), "expect": expect.bfloat16(), "B": B, "L": L, "heads": heads,
            "gap": None if gap is None else gap * SCALE, "attempts": attempt + 1}


@functools.lru_cache(maxsize=None)
def constant_v_case(B, L, heads):
    """Q = s_b a_i u_h, K = -s_b 4 u_h (u_h a +-1 vector, a_i in {2, 3, 4}, s_b = (-1)^b): every real key of a batch scores the
    same -8 a_i <= -64 (scaled) against a query, V is one vector w_bh for all of them, so the output is w_bh bit for bit (L w is
    exact in fp32, L w (1 / L) rounds back to w in bf16).  A zero pad row scores 0 and a key of the next batch +8 a_i: either,
    once admitted, takes the whole softmax.  Asserted from int64 dot products."""
    g = _gen("constant_v", B, L, heads)
    u = torch.randint(0, 2, (heads, 64), generator=g) * 2 - 1
    a = torch.randint(2, 5, (B, L), generator=g)
    sb = torch.tensor([1 - 2 * (b % 2) for b in range(B)])
    q = sb[:, None, None, None] * a[:, :, None, None] * u[None, None]
    k = (-4 * sb[:, None, None, None] * u[None, None]).expand(B, L, heads, 64).contiguous()
    w = _bf16_values((B, 1, heads, 64), g)
    for b in range(B):
        for h in range(heads):
            s = q[b, :, h] @ k[b, :, h].T
            assert bool((s == s[:, :1]).all()) and float(s.max()) * SCALE <= MAX_CONST_SCORE
            if b + 1 < B:
                assert float((q[b, :, h] @ k[b + 1, :, h].T).min()) * SCALE >= -MAX_CONST_SCORE
    expect = w.expand(B, L, heads, 64).reshape(B * L, heads * 64)
    return {"qkv": _pack_qkv(q, k, w.expand(B, L, heads, 64)), "expect": expect.bfloat16(), "B": B, "L": L, "heads": heads}


EXACT_CASES = {"selection": selection_case, "constant_v": constant_v_case}


def exact_shapes():
    """(B, L, heads) of every exact case"""
    return [(B, L, heads) for (B, heads) in ATT_BH for L in ATT_L] + [ATT_FULL]


# --------------------------------------------------------------------------------------------- float64-bounded attention cases
def bounded_shape(L):
    return ATT_FULL if L == ATT_FULL[1] else (2, L, 3)


@functools.lru_cache(maxsize=None)
def bounded_case(family, L):
    """randn 1.5 / randn 4 (a peaked softmax), and keys ordered so that every query's best score of a 64-key tile rises
    (ascending: every tile rescales) or falls (descending: none after the first does) from tile to tile -- asserted in float64."""
    B, L, heads = bounded_shape(L)
    C = heads * 64
    g = _gen("bounded", family, L)
    if family.startswith("randn"):
        qkv = (torch.randn(B * L, 3 * C, generator=g) * float(family[5:])).bfloat16()
        return {"qkv": qkv, "B": B, "L": L, "heads": heads}
    tile = torch.arange(L) // AK
    if family == "descending":
        tile = tile.flip(0)
    ntiles = (L + AK - 1) // AK
    for attempt in range(32):                             # a one-key tail tile has no maximum over 64 draws to lean on: reseed until ordered
        g = _gen("bounded", family, L, attempt)
        u = (torch.randint(0, 2, (heads, 64), generator=g) * 2 - 1).float()
        q = 0.5 * torch.randn(B, L, heads, 64, generator=g) + 0.5 * u
        k = 0.5 * torch.randn(B, L, heads, 64, generator=g) + tile.float()[None, :, None, None] * u       # ~ +4 per tile after the scale
        v = torch.randn(B, L, heads, 64, generator=g) * 1.5
        qkv = torch.cat([t.reshape(B * L, C) for t in (q, k, v)], dim=1).bfloat16()
        qh, kh, _ = split_heads(qkv.double(), B, L, heads)
        s = qh @ kh.transpose(-1, -2)
        best = torch.stack([s[..., t * AK:(t + 1) * AK].max(dim=-1).values for t in range(ntiles)], dim=-1)  # [B, heads, L, ntiles]
        d = best[..., 1:] - best[..., :-1]
        if bool((d > 0).all()) if family == "ascending" else bool((d < 0).all()):
            return {"qkv": qkv, "B": B, "L": L, "heads": heads, "attempts": attempt + 1}
    raise AssertionError(f"no seed ordered the tile maxima: {family} L={L}")


# --------------------------------------------------------------------------------------------- attention references
def attention64(qkv, B, L, heads, scale=SCALE, with_scale=False):
    """softmax(Q K^T scale) V per head in float64 from the packed bf16 operands: [B L, C] float64; with_scale also returns
    sum_j p_j |v_j|, the natural scale of the two bf16 roundings."""
    q, k, v = split_heads(qkv.double(), B, L, heads)
    out = torch.empty(B, heads, L, 64, dtype=torch.float64)
    mag = torch.empty_like(out)
    for b in range(B):
        for h in range(heads):
            p = torch.softmax(q[b, h] @ k[b, h].T * scale, dim=-1)
            out[b, h] = p @ v[b, h]
            mag[b, h] = p @ v[b, h].abs()
    out, mag = (t.permute(0, 2, 1, 3).reshape(B * L, heads * 64) for t in (out, mag))
    return (out, mag) if with_scale else out


def attention_err(o, qkv, B, L, heads, scale=SCALE):
    """largest |o - ref64| / (sum_j p_j |v_j| + |ref64|) over the elements"""
    ref, mag = attention64(qkv, B, L, heads, scale, with_scale=True)
    return float(((o.double().cpu() - ref).abs() / (mag + ref.abs())).max())


_SWAP23 = torch.tensor([(r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1) for r in range(AK)])


def attention_model(qkv, B, L, heads, scale=SCALE, mutate=None):
    """fp32 model of the kernel's rounding points (header of vit_ops.hip): keys in tiles of 64, rows past L zero-filled and their
    scores set to -inf; running max m; p = exp((s - m) scale) in fp32; the UNROUNDED p summed into l, separately for the two
    half-waves (key bit 3) and joined at the end; p rounded to bf16 for the P V product, accumulated in fp32; o and l rescaled by
    exp((m_old - m) scale) when the max moves; o (1 / l) rounded to bf16.
    mutate: 'mask_gt' masks key > L instead of key >= L; 'identity_perm' stores the K rows unpermuted, so the score in k-slot j
    is that of the key with bits 2 and 3 swapped; 'no_v_zero' leaves the V rows of masked keys indeterminate (NaN)."""
    assert mutate is None or mutate in MUTATIONS
    q, k, v = split_heads(qkv.float(), B, L, heads)
    out = torch.empty(B, heads, L, 64, dtype=torch.bfloat16)
    slot = torch.arange(AK)
    halves = [((slot >> 3) & 1) == hi for hi in (0, 1)]
    ninf = torch.tensor(-math.inf)
    for b in range(B):
        for h in range(heads):
            m = torch.full((L,), -math.inf)
            l = torch.zeros(L, 2)
            o = torch.zeros(L, 64)
            for k0 in range(0, L, AK):
                n = min(AK, L - k0)
                kt = torch.zeros(AK, 64)
                vt = torch.full((AK, 64), math.nan) if mutate == "no_v_zero" else torch.zeros(AK, 64)
                kt[:n], vt[:n] = k[b, h, k0:k0 + n], v[b, h, k0:k0 + n]
                s = q[b, h] @ kt.T                                                    # [L, 64] by key
                if mutate == "identity_perm":
                    s = s[:, _SWAP23]
                masked = (k0 + slot > L) if mutate == "mask_gt" else (k0 + slot >= L)
                s = torch.where(masked[None], ninf, s)
                m_new = torch.maximum(m, s.max(dim=1).values)
                resc = torch.exp((m - m_new) * scale)
                p = torch.exp((s - m_new[:, None]) * scale)
                l = l * resc[:, None] + torch.stack([p[:, hv].sum(dim=1) for hv in halves], dim=1)
                pb = p.bfloat16().float()
                pv = torch.zeros(L, 64)
                for d in range(0, AK, 16):                                            # one MFMA k-step of 16 keys at a time
                    pv = pv + _mm_keep_nan(pb[:, d:d + 16], vt[d:d + 16])
                o = o * resc[:, None] + pv
                m = m_new
            inv = 1.0 / (l[:, 0] + l[:, 1])
            out[b, h] = (o * inv[:, None]).bfloat16()
    return out.permute(0, 2, 1, 3).reshape(B * L, heads * 64)


def _mm_keep_nan(a, b):
    """a @ b in fp32 where 0 * NaN stays NaN whatever the BLAS does with zeros"""
    r = a @ b
    r[:, ~torch.isfinite(b).all(dim=0)] = math.nan                                    # a column of b with a non-finite value
    return r


# --------------------------------------------------------------------------------------------- LayerNorm
def layernorm_route(C, x_row_stride, y_row_stride, *addresses):
    """the dispatch of oess_layernorm_bf16 restated: 16-byte accesses need C % 8 == 0, both row strides % 8 == 0 (elements) and the
    four pointers (x, y, gamma, beta; byte addresses) 16-byte aligned"""
    assert len(addresses) == 4
    vec = C % 8 == 0 and x_row_stride % 8 == 0 and y_row_stride % 8 == 0 and all(a % 16 == 0 for a in addresses)
    return "vec" if vec else "scalar"


def layernorm_inputs(C, rows, family):
    """bf16 [rows, C] input of a family, fp32 gamma in [0.5, 1.5) and beta ~ 0.1 randn"""
    g = _gen("layernorm", C, rows, family)
    if family == "randn":
        x = torch.randn(rows, C, generator=g)
    elif family == "large_mean":                          # row mean 100, spread 0.25 (bf16 steps of 0.5 up there): E[x^2] - mean^2 fails
        x = 100.0 + 0.25 * torch.randn(rows, C, generator=g)
    elif family == "large_mean_sparse":                   # 100 with one element in 16 a bf16 step away: sigma ~ 0.125, a one-pass
        step = torch.randint(0, 2, (rows, C), generator=g).float() - 0.5          # variance is wrong in its leading digits
        x = 100.0 + step * (torch.rand(rows, C, generator=g) < 1.0 / 16.0)
    elif family == "constant":                            # variance 0: the output is beta, eps decides
        x = _bf16_values((rows, 1), g).float().mul(torch.tensor([1.0, 32.0])[torch.randint(0, 2, (rows, 1), generator=g)]).expand(rows, C)
    elif family == "single":                              # one non-zero element per row
        x = torch.zeros(rows, C)
        x[torch.arange(rows), torch.randint(0, C, (rows,), generator=g)] = _bf16_values((rows,), g).float()
    else:
        raise ValueError(family)
    return x.bfloat16().contiguous(), torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1


def place_layernorm(x, gamma, beta, layout, device="cpu"):
    """The operands of a case on `device` the way `layout` names: returns x view, gamma, beta, out view, out buffer.  Gaps of the
    input buffer hold NaN, the output buffer is prefilled with SENTINEL."""
    rows, C = x.shape
    xs = ys = C
    goff = boff = 0
    if layout == "x_stride_772":
        xs = 772
    elif layout == "y_stride_772":
        ys = 772
    elif layout == "strides_776_784":
        xs, ys = C + 8, C + 16
    elif layout == "gamma_offset_1":
        goff = 1
    elif layout == "beta_offset_1":
        boff = 1
    else:
        assert layout == "dense", layout
    _, xv = embed(x, 0, xs - C, math.nan, device)
    ybuf = torch.full((rows, ys), SENTINEL, dtype=torch.bfloat16, device=device)
    yv = ybuf[:, :C]
    gbuf = torch.zeros(C + 4, device=device)
    bbuf = torch.zeros(C + 4, device=device)
    gbuf[goff:goff + C], bbuf[boff:boff + C] = gamma.to(device), beta.to(device)
    return xv, gbuf[goff:goff + C], bbuf[boff:boff + C], yv, ybuf


def route_of(xv, gv, bv, yv):
    return layernorm_route(xv.shape[1], xv.stride(0), yv.stride(0), xv.data_ptr(), yv.data_ptr(), gv.data_ptr(), bv.data_ptr())


def layer_norm64(x, gamma, beta, eps=LN_EPS):
    """nn.LayerNorm (biased variance) in float64 from the bf16 input"""
    x, gamma, beta = x.double().cpu(), gamma.double().cpu(), beta.double().cpu()
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def layernorm_err(y, x, gamma, beta, eps=LN_EPS):
    """largest |y - ref64| / (2^-9 |ref64| + 2^-18 kappa_r |gamma_c| + 2^-20 |ref64 - beta_c|), kappa_r = max|x_r| / sigma_r with
    sigma_r floored by sqrt(eps): bf16 output rounding, the fp32 mean (32 sequential adds + 6 shuffle levels ~ 38 2^-24 max|x|, in
    normalised units) and rsqrtf"""
    ref = layer_norm64(x, gamma, beta, eps)
    xd, gd, bd = x.double().cpu(), gamma.double().cpu(), beta.double().cpu()
    sigma = xd.var(dim=1, unbiased=False, keepdim=True).sqrt().clamp_min(math.sqrt(eps))
    kappa = xd.abs().max(dim=1, keepdim=True).values / sigma
    den = 2.0 ** -9 * ref.abs() + 2.0 ** -18 * kappa * gd.abs() + 2.0 ** -20 * (ref - bd).abs()
    assert bool((den > 0).all())
    return float(((y.double().cpu() - ref).abs() / den).max())


_BUTTERFLY = [torch.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)]


def _wave_sum(v):
    """[rows, 64] per-lane partial sums -> the fp32 xor-butterfly of wave_sum (every lane ends with the same value)"""
    for perm in _BUTTERFLY:
        v = v + v[:, perm]
    return v[:, :1]


def layer_norm_model(x, gamma, beta, eps=LN_EPS, route="vec", one_pass=False):
    """fp32 model of the two kernels: one wave per row, a lane adds its own channels in order (scalar route: channels lane,
    lane + 64, ...; vector route: the 8 channels of chunk lane, lane + 64, ...), the wave joins by an xor butterfly; two passes
    (mean, then squared deviations); rsqrt(var + eps); (x - mean) rstd gamma + beta without contraction, rounded to bf16.
    one_pass: the variance as E[x^2] - mean^2 from the same lane sums instead -- what the large-mean families are there to fail."""
    rows, C = x.shape
    xf, gf, bf = x.float(), gamma.float(), beta.float()
    per = 8 if route == "vec" else 1
    assert route in ("vec", "scalar") and C % per == 0
    step = 64 * per
    n = (C + step - 1) // step
    pad = n * step - C
    valid = torch.cat([torch.ones(C, dtype=torch.bool), torch.zeros(pad, dtype=torch.bool)]).reshape(n, 64, per)

    def lanes(t):                                          # [rows, C] -> [rows, n, 64, per]: element (i, lane, k) is channel (64 i + lane) per + k
        return torch.cat([t, torch.zeros(rows, pad)], dim=1).reshape(rows, n, 64, per)

    def lane_sum(t):
        s = torch.zeros(rows, 64)
        for i in range(n):
            for k in range(per):
                s = s + t[:, i, :, k]
        return _wave_sum(s)

    xl = lanes(xf)
    mean = lane_sum(xl) / float(C)
    if one_pass:
        var = (lane_sum(xl * xl) / float(C) - mean * mean).clamp_min(0.0)
    else:
        d = torch.where(valid[None], xl - mean[:, :, None, None], torch.zeros(()))
        var = lane_sum(d * d) / float(C)
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    return ((xf - mean) * rstd * gf + bf).bfloat16()
