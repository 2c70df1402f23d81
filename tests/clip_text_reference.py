"""Float64 restatement of OpenAI CLIP's text encoder and of the prompt ensemble (K29), written from the definition and not from
openess_amd/models/clip_text.py: the oracle of tests/test_hip_clip_text.py, held to HuggingFace's CLIPTextModelWithProjection in
tests/test_clip_text_reference.py.  State-dict keys are OpenAI's.  Also the shared cases of those tests and of
tools/exp_clip_text_bounds.py, and the bounds: 4.0 * FIGURE, a FIGURE being torch fp32 against this file on the CPU
(max |d| / max |ref|); nothing a kernel produced went into one.

Nothing here needs a GPU or transformers."""
import functools
import math

import torch
import torch.nn.functional as F

from tests import vit_token_cases as vc

SCALE, AK, SENTINEL = vc.SCALE, vc.AK, vc.SENTINEL
_gen = vc._gen

# ---- cases
CAUSAL_L = (1, 63, 64, 65, 77, 128, 129, 200)      # 64-key tile edges; 128: the query block edge (a later block skips later tiles)
CAUSAL_BH = ((1, 1), (1, 2), (3, 1), (3, 2))
CAUSAL_STRIDE_EXTRA = 4                             # qkv row stride 3 C + 4 floats, NaN in the gap
CAUSAL_OUT_EXTRA = 64
LEAK_CASES = ((200, 62), (200, 63), (200, 64), (200, 127), (200, 128), (77, 5))        # (L, j): keys > j are overwritten
CAUSAL_BOUNDED = ((2, 77, 8), (2, 200, 3))         # (B, L, heads), randn 1.5
EMBED_C = (64, 66, 512)
QGELU_SHAPES = ((5, 64, 256), (77, 128, 512))
EOT_CASES = ((5, 16, 128), (7, 77, 512), (3, 9, 66))            # (N, L, C)
PROMPT_GROUPS = (1, 2, 7, 1, 7)
PROMPT_D = (512, 96)
TOWER_SMALL = dict(vocab_size=64, context_length=16, width=128, heads=2, layers=2, embed_dim=96)
TOWER_REAL = dict(vocab_size=512, context_length=77, width=512, heads=8, layers=12, embed_dim=512)   # a 512-row token table
TOWER_CASES = {"small": (TOWER_SMALL, 6, 16), "real": (TOWER_REAL, 22, 77)}                           # (geometry, prompts, L)

# ---- figures (tools/exp_clip_text_bounds.py prints them): torch fp32 on the CPU against float64, max |d| / max |ref|
CAUSAL_FIGURES = {(2, 77, 8): 6.288e-07, (2, 200, 3): 7.649e-07}
QGELU_FIGURES = {(5, 64, 256): 2.349e-07, (77, 128, 512): 3.920e-07}
PROMPT_FIGURES = {512: 1.230e-07, 96: 7.657e-08}
TOWER_FIGURES = {"small": 5.591e-07, "real": 7.341e-07}
CAUSAL_BOUNDS = {k: 4.0 * v for k, v in CAUSAL_FIGURES.items()}
QGELU_BOUNDS = {k: 4.0 * v for k, v in QGELU_FIGURES.items()}
PROMPT_BOUNDS = {k: 4.0 * v for k, v in PROMPT_FIGURES.items()}
TOWER_BOUNDS = {k: 4.0 * v for k, v in TOWER_FIGURES.items()}


def rel_max(x, ref):
    """max |x - ref| / max |ref| over EVERY element"""
    return float((x.double().cpu() - ref.double()).abs().max() / ref.double().abs().max())


# --------------------------------------------------------------------------------------------- the definition, float64
def quick_gelu64(v):
    return v * torch.sigmoid(1.702 * v)


def causal_attention64(qkv, B, L, heads, scale=SCALE):
    """softmax over keys <= query of (Q K^T scale), times V, per head, float64: packed [B L, 3 C] -> [B L, C]"""
    q, k, v = vc.split_heads(qkv.double(), B, L, heads)
    s = q @ k.transpose(-1, -2) * scale
    future = torch.ones(L, L, dtype=torch.bool).triu(1)
    p = torch.softmax(s.masked_fill(future, -math.inf), dim=-1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B * L, heads * 64)


def text_hidden64(sd, ids, heads):
    """the last block's output [N, L, width] in float64 from an OpenAI-named state dict"""
    sd = {k: v.double() for k, v in sd.items()}
    N, L = ids.shape
    x = sd["token_embedding.weight"][ids] + sd["positional_embedding"][:L]
    C = x.shape[-1]
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in sd:
        p = f"transformer.resblocks.{i}."
        y = F.layer_norm(x, (C,), sd[p + "ln_1.weight"], sd[p + "ln_1.bias"], 1e-5)
        qkv = y @ sd[p + "attn.in_proj_weight"].T + sd[p + "attn.in_proj_bias"]
        a = causal_attention64(qkv.reshape(N * L, 3 * C), N, L, heads, scale=(C // heads) ** -0.5).reshape(N, L, C)
        x = x + a @ sd[p + "attn.out_proj.weight"].T + sd[p + "attn.out_proj.bias"]
        y = F.layer_norm(x, (C,), sd[p + "ln_2.weight"], sd[p + "ln_2.bias"], 1e-5)
        h = quick_gelu64(y @ sd[p + "mlp.c_fc.weight"].T + sd[p + "mlp.c_fc.bias"])
        x = x + h @ sd[p + "mlp.c_proj.weight"].T + sd[p + "mlp.c_proj.bias"]
        i += 1
    return x


def text_encode64(sd, ids, heads):
    """[N, embed_dim] float64, not normalised: ln_final, the row at argmax(ids), times text_projection"""
    x = text_hidden64(sd, ids, heads)
    C = x.shape[-1]
    x = F.layer_norm(x, (C,), sd["ln_final.weight"].double(), sd["ln_final.bias"].double(), 1e-5)
    return x[torch.arange(x.shape[0]), ids.argmax(dim=-1)] @ sd["text_projection"].double()


def prompt_mean64(e, offsets):
    """out[k] = normalize(sum in prompt order of normalize(e[n])), float64"""
    e = e.double()
    e = e / e.pow(2).sum(dim=1, keepdim=True).sqrt()
    rows = []
    for k in range(len(offsets) - 1):
        s = torch.zeros(e.shape[1], dtype=torch.float64)
        for n in range(int(offsets[k]), int(offsets[k + 1])):
            s = s + e[n]
        rows.append(s / s.pow(2).sum().sqrt())
    return torch.stack(rows)


# --------------------------------------------------------------------------------------------- the same in torch fp32 (the figures)
def causal_attention32(qkv, B, L, heads):
    q, k, v = vc.split_heads(qkv.float(), B, L, heads)
    s = q @ k.transpose(-1, -2) * SCALE
    p = torch.softmax(s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), -math.inf), dim=-1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B * L, heads * 64)


def text_encode32(sd, ids, heads):
    """the tower in torch fp32 on the CPU, op by op as the definition"""
    sd = {k: v.float() for k, v in sd.items()}
    N, L = ids.shape
    x = sd["token_embedding.weight"][ids] + sd["positional_embedding"][:L]
    C = x.shape[-1]
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in sd:
        p = f"transformer.resblocks.{i}."
        y = F.layer_norm(x, (C,), sd[p + "ln_1.weight"], sd[p + "ln_1.bias"], 1e-5)
        qkv = F.linear(y, sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"])
        a = causal_attention32(qkv.reshape(N * L, 3 * C), N, L, heads).reshape(N, L, C)
        x = x + F.linear(a, sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"])
        y = F.layer_norm(x, (C,), sd[p + "ln_2.weight"], sd[p + "ln_2.bias"], 1e-5)
        h = F.linear(y, sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"])
        h = h * torch.sigmoid(1.702 * h)
        x = x + F.linear(h, sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"])
        i += 1
    x = F.layer_norm(x, (C,), sd["ln_final.weight"], sd["ln_final.bias"], 1e-5)
    return x[torch.arange(N), ids.argmax(dim=-1)] @ sd["text_projection"]


def prompt_mean32(e, offsets):
    e = F.normalize(e.float(), dim=1, eps=0.0)
    return torch.stack([F.normalize(e[int(offsets[k]):int(offsets[k + 1])].sum(dim=0), dim=0, eps=0.0) for k in range(len(offsets) - 1)])


# --------------------------------------------------------------------------------------------- attention cases
@functools.lru_cache(maxsize=None)
def causal_selection_case(B, L, heads):
    """vit_token_cases.selection_case with the selected key drawn from 0 .. query: K rows are random +-4 vectors, Q[i] =
    2 K[pi(i)], pi(i) <= i, V random bf16-exact values in 0.5 <= |v| < 4.  Every score is an exact integer and the winner leads
    every OTHER VISIBLE key by >= MIN_GAP after the scale (asserted from int64 dot products), so the output is V[pi(i)] bit for
    bit; row 0 is V[0].  Future keys are not constrained here (test_future_keys_do_not_leak is about them)."""
    for attempt in range(32):
        g = _gen("causal_selection", B, L, heads, attempt)
        k = torch.randint(0, 2, (B, L, heads, 64), generator=g) * 8 - 4
        pi = (torch.rand(B, heads, L, generator=g) * (torch.arange(L) + 1)).long().clamp_max(torch.arange(L))
        kh = k.permute(0, 2, 1, 3)
        qh = 2 * torch.gather(kh, 2, pi[..., None].expand(B, heads, L, 64))
        s = qh @ kh.transpose(-1, -2)                                                          # int64 [B, heads, L, L]
        win = s.gather(3, pi[..., None])[..., 0]
        assert bool((win == 2 * 64 * 16).all())
        other = s.scatter(3, pi[..., None], torch.iinfo(torch.int64).min)
        other = other.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), torch.iinfo(torch.int64).min)
        gap = int((win - other.max(dim=-1).values)[..., 1:].min()) if L > 1 else None
        if gap is None or gap * SCALE >= vc.MIN_GAP:
            break
    else:
        raise AssertionError("no seed gave the selection gap")
    v = vc._bf16_values((B, L, heads, 64), g)
    expect = torch.gather(v.permute(0, 2, 1, 3), 2, pi[..., None].expand(B, heads, L, 64)).permute(0, 2, 1, 3).reshape(B * L, heads * 64)
    qkv = torch.cat([t.reshape(B * L, heads * 64) for t in (qh.permute(0, 2, 1, 3), k, v)], dim=1)
    return {"qkv": qkv.float(), "expect": expect.float(), "B": B, "L": L, "heads": heads}


def causal_exact_case(family, B, L, heads):
    if family == "selection":
        return causal_selection_case(B, L, heads)
    c = vc.constant_v_case(B, L, heads)                    # every visible key scores the same and carries the same V
    return {"qkv": c["qkv"].float(), "expect": c["expect"].float(), "B": B, "L": L, "heads": heads}


@functools.lru_cache(maxsize=None)
def causal_bounded_case(B, L, heads):
    g = _gen("causal_bounded", B, L, heads)
    return torch.randn(B * L, 3 * heads * 64, generator=g) * 1.5          # not bf16-exact


# --------------------------------------------------------------------------------------------- kernel cases
@functools.lru_cache(maxsize=None)
def qgelu_case(rows, Cin, Cout):
    g = _gen("qgelu", rows, Cin, Cout)
    return {"x": torch.randn(rows, Cin, generator=g), "w": torch.randn(Cout, Cin, generator=g) / math.sqrt(Cin),
            "b": torch.randn(Cout, generator=g) * 0.5}


def qgelu64(c):
    return quick_gelu64(c["x"].double() @ c["w"].double().T + c["b"].double())


def qgelu32(c):
    h = F.linear(c["x"], c["w"], c["b"])
    return h * torch.sigmoid(1.702 * h)


@functools.lru_cache(maxsize=None)
def qgelu_int_case(rows, Cin, Cout):
    """integer operands whose pre-activation is an exact integer; column 0 is made zero for every row (w row 0 = 0, bias 0)"""
    g = _gen("qgelu_int", rows, Cin, Cout)
    x = torch.randint(-4, 5, (rows, Cin), generator=g).float()
    w = torch.randint(-3, 4, (Cout, Cin), generator=g).float()
    b = torch.randint(-5, 6, (Cout,), generator=g).float()
    w[0], b[0] = 0.0, 0.0
    return {"x": x, "w": w, "b": b}


@functools.lru_cache(maxsize=None)
def eot_case(N, L, C):
    """ids with the maximum planted twice in some rows (the first must win), at t = 0 in one and at t = L - 1 in another"""
    g = _gen("eot", N, L, C)
    ids = torch.randint(0, 50, (N, L), generator=g)
    pos = torch.randint(0, L, (N,), generator=g)
    pos[0], pos[-1] = 0, L - 1
    ids[torch.arange(N), pos] = 63
    for n in range(0, N, 2):                              # a tie behind the first maximum
        if pos[n] + 1 < L:
            ids[n, torch.randint(int(pos[n]) + 1, L, (1,), generator=g)] = 63
    assert bool((ids.argmax(dim=1) == pos).all())
    return {"ids": ids, "pos": pos, "x": torch.randn(N * L, C, generator=g), "gamma": torch.rand(C, generator=g) + 0.5,
            "beta": torch.randn(C, generator=g) * 0.1}


@functools.lru_cache(maxsize=None)
def prompt_case(D):
    g = _gen("prompt", D)
    off = torch.tensor([0] + list(PROMPT_GROUPS)).cumsum(0)
    return {"e": torch.randn(int(off[-1]), D, generator=g) * 3.0, "offsets": off}


# --------------------------------------------------------------------------------------------- tower cases
@functools.lru_cache(maxsize=None)
def tower_state(name):
    """seeded weights of a tower case in OpenAI names, larger than the initialisation's so that every term matters"""
    geo = TOWER_CASES[name][0]
    g = _gen("tower", name)
    W, V, E, n = geo["width"], geo["vocab_size"], geo["embed_dim"], geo["layers"]
    r = lambda *s, std=1.0: torch.randn(*s, generator=g) * std
    sd = {"token_embedding.weight": r(V, W, std=0.5), "positional_embedding": r(geo["context_length"], W, std=0.3)}
    for i in range(n):
        p = f"transformer.resblocks.{i}."
        sd.update({p + "ln_1.weight": torch.rand(W, generator=g) * 0.6 + 0.7, p + "ln_1.bias": r(W, std=0.1),
                   p + "attn.in_proj_weight": r(3 * W, W, std=1.5 * W ** -0.5), p + "attn.in_proj_bias": r(3 * W, std=0.1),
                   p + "attn.out_proj.weight": r(W, W, std=W ** -0.5 * (2 * n) ** -0.5), p + "attn.out_proj.bias": r(W, std=0.1),
                   p + "ln_2.weight": torch.rand(W, generator=g) * 0.6 + 0.7, p + "ln_2.bias": r(W, std=0.1),
                   p + "mlp.c_fc.weight": r(4 * W, W, std=W ** -0.5), p + "mlp.c_fc.bias": r(4 * W, std=0.1),
                   p + "mlp.c_proj.weight": r(W, 4 * W, std=(4 * W) ** -0.5 * (2 * n) ** -0.5), p + "mlp.c_proj.bias": r(W, std=0.1)})
    sd.update({"ln_final.weight": torch.rand(W, generator=g) * 0.6 + 0.7, "ln_final.bias": r(W, std=0.1),
               "text_projection": r(W, E, std=W ** -0.5)})
    return sd


@functools.lru_cache(maxsize=None)
def tower_ids(name):
    """[N, L] ids in the tokenizer's layout: SOT (V - 2), 1 .. L - 2 tokens below V - 2, EOT (V - 1), zeros"""
    geo, N, L = TOWER_CASES[name]
    V = geo["vocab_size"]
    g = _gen("tower_ids", name)
    ids = torch.zeros(N, L, dtype=torch.int64)
    for n in range(N):
        k = 1 if n == 0 else (L - 2 if n == 1 else int(torch.randint(1, L - 1, (1,), generator=g)))
        ids[n, 0] = V - 2
        ids[n, 1:1 + k] = torch.randint(1, V - 2, (k,), generator=g)
        ids[n, 1 + k] = V - 1
    return ids


def tower_offsets(name):
    N = TOWER_CASES[name][1]
    return torch.tensor([0, 1, 3, N], dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def tower_reference(name):
    """float64 [N, embed_dim] of a tower case, computed once"""
    return text_encode64(tower_state(name), tower_ids(name), TOWER_CASES[name][0]["heads"])


# --------------------------------------------------------------------------------------------- synthetic tokenizer + checkpoint
# 256 byte symbols (id = position in bytes_to_unicode: a printable ASCII character c has id ord(c) - 33), the same with </w>
# (+ 256), then one id per merge (512 + i), <|startoftext|> = 517, <|endoftext|> = 518
SYNTH_MERGES = (("r", "o"), ("a", "d</w>"), ("ro", "ad</w>"), ("c", "a"), ("ca", "r</w>"))
SYNTH_SOT, SYNTH_EOT, SYNTH_VOCAB = 517, 518, 519
SYNTH_TOWER = dict(vocab_size=SYNTH_VOCAB, context_length=77, width=128, heads=2, layers=2, embed_dim=512)


def write_merges(path, gz=False, header=True):
    import gzip
    text = ("#version: 0.2\n" if header else "") + "".join(f"{a} {b}\n" for a, b in SYNTH_MERGES)
    with (gzip.open(path, "wb") if gz else open(path, "wb")) as f:
        f.write(text.encode("utf-8"))
    return str(path)


def write_synthetic_checkpoint(path, seed=29):
    """a seeded random text tower of SYNTH_TOWER's geometry, saved as a FULL CLIP state dict (visual.* and logit_scale beside the
    text keys, which a loader must ignore)"""
    from openess_amd.models.clip_text import CLIPTextEncoder
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        m = CLIPTextEncoder(**SYNTH_TOWER)
        with torch.no_grad():
            m.token_embedding.weight.mul_(20.0)               # the initialisation's 0.02 leaves every prompt nearly alike
            m.positional_embedding.mul_(20.0)
        sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd["visual.proj"] = torch.zeros(4, 4)
    sd["logit_scale"] = torch.tensor(4.6052)
    torch.save(sd, path)
    return str(path)
