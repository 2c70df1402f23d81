"""CLIP's text tower in fp32 on the HIP token kernels (K29): class names -> the [K, embed_dim] text embeddings every classifier
here multiplies with (`text_embeddings_path`).

The definition is OpenAI CLIP's text encoder (ViT-B/16 checkpoint): token + position embedding, `layers` pre-LN blocks of
width `width` with `heads` heads of 64 under a causal mask and a QuickGELU FFN (x sigmoid(1.702 x)), LayerNorm eps 1e-5,
`ln_final`, the row at argmax(token ids) (the end-of-text token has the largest id), times `text_projection` (x @ P, no bias).
Parameter names are those of OpenAI's state dict, so the text keys of that checkpoint load strictly.

Inference only, fp32 only: the result is computed once per run and becomes classifier weights.  Per block:
  hip.layer_norm_tokens_f32 -> hip.linear_tokens_f32 (in_proj) -> hip.attention_d64_f32(causal=True) -> linear (out_proj, + x)
  -> layer norm -> linear (c_fc, QuickGELU epilogue) -> linear (c_proj, + x)
then hip.clip_text_eot_norm on the N end-of-text rows alone and the projection as one more token GEMM.  Packed operands are
cached per parameter version (engine.PackedWeightF32), as in the image tower."""
import os

import torch
import torch.nn as nn

from .. import engine, hip

_HF_PREFIX = "text_model."


class _Attn(nn.Module):
    """parameter holder with nn.MultiheadAttention's names"""

    def __init__(self, width):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * width, width))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * width))
        self.out_proj = nn.Linear(width, width)


class _MLP(nn.Module):
    def __init__(self, width):
        super().__init__()
        self.c_fc = nn.Linear(width, 4 * width)
        self.c_proj = nn.Linear(4 * width, width)


def _linear(x, lin_w, lin_b, pw, act=None, residual=None):
    pw.get(lin_w.detach()[:, :, None, None], None if lin_b is None else lin_b.detach())
    return hip.linear_tokens_f32(x, pw.packed, pw.bias, lin_w.shape[0], act=act, residual=residual)


class ResidualAttentionBlock(nn.Module):
    def __init__(self, width, heads):
        super().__init__()
        self.heads = heads
        self.attn = _Attn(width)
        self.ln_1 = nn.LayerNorm(width, eps=1e-5)
        self.mlp = _MLP(width)
        self.ln_2 = nn.LayerNorm(width, eps=1e-5)
        self._pw32 = {k: engine.PackedWeightF32() for k in ('qkv', 'out', 'fc', 'proj')}

    def forward_fp32(self, x, N, L):
        """x: fp32 tokens [N*L, width] -> same shape"""
        a = self.attn
        y = hip.layer_norm_tokens_f32(x, self.ln_1.weight, self.ln_1.bias, self.ln_1.eps)
        qkv = _linear(y, a.in_proj_weight, a.in_proj_bias, self._pw32['qkv'])
        o = hip.attention_d64_f32(qkv, N, L, self.heads, causal=True)
        x = _linear(o, a.out_proj.weight, a.out_proj.bias, self._pw32['out'], residual=x)
        y = hip.layer_norm_tokens_f32(x, self.ln_2.weight, self.ln_2.bias, self.ln_2.eps)
        h = _linear(y, self.mlp.c_fc.weight, self.mlp.c_fc.bias, self._pw32['fc'], act='quick_gelu')
        return _linear(h, self.mlp.c_proj.weight, self.mlp.c_proj.bias, self._pw32['proj'], residual=x)


class _Transformer(nn.Module):
    def __init__(self, width, heads, layers):
        super().__init__()
        self.resblocks = nn.ModuleList([ResidualAttentionBlock(width, heads) for _ in range(layers)])


class CLIPTextEncoder(nn.Module):
    def __init__(self, vocab_size=49408, context_length=77, width=512, heads=8, layers=12, embed_dim=512):
        super().__init__()
        for name, v in (("vocab_size", vocab_size), ("context_length", context_length), ("width", width), ("heads", heads),
                        ("layers", layers), ("embed_dim", embed_dim)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"CLIPTextEncoder: {name} must be a positive integer, got {v!r}")
        if heads * 64 != width:
            raise ValueError(f"CLIPTextEncoder: the attention kernel has heads of 64 channels: width {width} != 64 * {heads} heads")
        if width > 2048:
            raise ValueError("CLIPTextEncoder: width above 2048 (the LayerNorm kernels hold a row in registers)")
        self.vocab_size, self.context_length, self.width, self.heads, self.embed_dim = vocab_size, context_length, width, heads, embed_dim
        self.token_embedding = nn.Embedding(vocab_size, width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, width))
        self.transformer = _Transformer(width, heads, layers)
        self.ln_final = nn.LayerNorm(width, eps=1e-5)
        self.text_projection = nn.Parameter(torch.empty(width, embed_dim))
        self._pw_proj32 = engine.PackedWeightF32()
        self.reset_parameters()
        self.requires_grad_(False)
        self.eval()

    def reset_parameters(self):
        """OpenAI CLIP's initialisation of the text side"""
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        n = len(self.transformer.resblocks)
        proj_std = (self.width ** -0.5) * ((2 * n) ** -0.5)
        attn_std = self.width ** -0.5
        fc_std = (2 * self.width) ** -0.5
        for b in self.transformer.resblocks:
            nn.init.normal_(b.attn.in_proj_weight, std=attn_std)
            nn.init.normal_(b.attn.out_proj.weight, std=proj_std)
            nn.init.normal_(b.mlp.c_fc.weight, std=fc_std)
            nn.init.normal_(b.mlp.c_proj.weight, std=proj_std)
        nn.init.normal_(self.text_projection, std=self.width ** -0.5)

    def _check_ids(self, ids):
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.ndim != 2:
            raise ValueError("CLIPTextEncoder: token ids must be int64 [N, L]")
        if ids.shape[1] > self.context_length:
            raise ValueError(f"CLIPTextEncoder: {ids.shape[1]} tokens per text, the context holds {self.context_length}")
        return ids.to(self.positional_embedding.device).contiguous()

    @torch.no_grad()
    def forward_fp32(self, ids):
        """int64 token ids [N, L] (L <= context_length; SOT, tokens, EOT, anything) -> fp32 [N, embed_dim], not normalised.  What
        follows the end-of-text token cannot reach it through the causal mask."""
        ids = self._check_ids(ids)
        N, L = ids.shape
        x = hip.clip_text_embed(ids, self.token_embedding.weight.detach(), self.positional_embedding.detach())
        for block in self.transformer.resblocks:
            x = block.forward_fp32(x, N, L)
        e = hip.clip_text_eot_norm(x, ids, self.ln_final.weight, self.ln_final.bias, self.ln_final.eps)
        return _linear(e, self.text_projection.detach().T, None, self._pw_proj32)

    forward = forward_fp32

    @torch.no_grad()
    def encode_classes(self, prompt_ids, group_offsets, chunk=256):
        """prompt_ids int64 [N, L]: the prompts of class k are rows group_offsets[k] .. group_offsets[k + 1] - 1 (int64 [K + 1]).
        -> fp32 [K, embed_dim] unit rows: every prompt's embedding normalised, summed per class in prompt order, normalised
        (CLIP's prompt ensemble).  The tower runs `chunk` prompts at a time."""
        prompt_ids = self._check_ids(prompt_ids)
        N = prompt_ids.shape[0]
        e = torch.empty((N, self.embed_dim), dtype=torch.float32, device=prompt_ids.device)
        for i in range(0, N, chunk):
            e[i:i + chunk] = self.forward_fp32(prompt_ids[i:i + chunk])
        return hip.prompt_mean_normalize(e, group_offsets)


# --------------------------------------------------------------------------------------------- checkpoints
def convert_hf_state_dict(sd):
    """HuggingFace CLIPTextModelWithProjection (or CLIPModel) state dict -> OpenAI names: q/k/v projections concatenated into
    in_proj, text_projection.weight transposed (HF applies it as a Linear)."""
    out = {}
    p = _HF_PREFIX
    out["token_embedding.weight"] = sd[p + "embeddings.token_embedding.weight"]
    out["positional_embedding"] = sd[p + "embeddings.position_embedding.weight"]
    i = 0
    while f"{p}encoder.layers.{i}.layer_norm1.weight" in sd:
        s, d = f"{p}encoder.layers.{i}.", f"transformer.resblocks.{i}."
        for t in ("weight", "bias"):
            out[f"{d}attn.in_proj_{t}"] = torch.cat([sd[f"{s}self_attn.{n}_proj.{t}"] for n in ("q", "k", "v")], dim=0)
            out[f"{d}attn.out_proj.{t}"] = sd[f"{s}self_attn.out_proj.{t}"]
            out[f"{d}ln_1.{t}"] = sd[f"{s}layer_norm1.{t}"]
            out[f"{d}mlp.c_fc.{t}"] = sd[f"{s}mlp.fc1.{t}"]
            out[f"{d}mlp.c_proj.{t}"] = sd[f"{s}mlp.fc2.{t}"]
            out[f"{d}ln_2.{t}"] = sd[f"{s}layer_norm2.{t}"]
        i += 1
    if i == 0:
        raise ValueError("convert_hf_state_dict: no text_model.encoder.layers.* keys")
    for t in ("weight", "bias"):
        out[f"ln_final.{t}"] = sd[f"{p}final_layer_norm.{t}"]
    out["text_projection"] = sd["text_projection.weight"].T.contiguous()
    return out


def text_state_dict(sd):
    """the text keys, in OpenAI names, of a plain text state dict, a full OpenAI CLIP state dict (visual.*, logit_scale and the
    shape scalars of the JIT archive ignored) or a HuggingFace one"""
    if any(k.startswith(_HF_PREFIX) for k in sd):
        return convert_hf_state_dict(sd)
    keep = ("token_embedding.", "positional_embedding", "transformer.", "ln_final.", "text_projection")
    out = {k: v for k, v in sd.items() if k.startswith(keep)}
    if "text_projection" not in out:
        raise ValueError("no CLIP text tower in this state dict (text_projection is missing)")
    return out


def load_clip_text_checkpoint(path, device=None):
    """CLIPTextEncoder with the geometry and the weights of the checkpoint at `path` (torch.save'd state dict, possibly under
    'state_dict' or 'model'; a TorchScript archive of OpenAI's is read through torch.jit.load)."""
    try:
        obj = torch.load(path, map_location="cpu", weights_only=True)
    except Exception:
        obj = torch.jit.load(path, map_location="cpu").state_dict()
    if hasattr(obj, "state_dict"):
        obj = obj.state_dict()
    for key in ("state_dict", "model"):
        if isinstance(obj, dict) and key in obj and isinstance(obj[key], dict):
            obj = obj[key]
    sd = {k: v.float() for k, v in text_state_dict(obj).items()}
    vocab, width = sd["token_embedding.weight"].shape
    layers = len({k.split(".")[2] for k in sd if k.startswith("transformer.resblocks.")})
    if width % 64:
        raise ValueError(f"load_clip_text_checkpoint: width {width} is no multiple of 64")
    m = CLIPTextEncoder(vocab_size=vocab, context_length=sd["positional_embedding"].shape[0], width=width, heads=width // 64,
                        layers=layers, embed_dim=sd["text_projection"].shape[1])
    m.load_state_dict(sd, strict=True)
    return m if device is None else m.to(device)


# --------------------------------------------------------------------------------------------- prompts
SINGLE_TEMPLATE = 'a photo of a {}.'


def read_templates(spec):
    """'single' -> ['a photo of a {}.'], 'none' -> ['{}'], otherwise a file with one template containing {} per line"""
    if spec is None or spec == 'single':
        return [SINGLE_TEMPLATE]
    if spec == 'none':
        return ['{}']
    with open(spec) as f:
        lines = [ln.strip() for ln in f if ln.strip()]
    if not lines or any('{}' not in ln for ln in lines):
        raise ValueError(f"{spec}: every template line must contain {{}}")
    return lines


def parse_classes(spec):
    """A comma list, or a file with one class per line; `a|b|c` names several names of one class -> the list build_prompts and
    build_vocabulary take (a name, or a list of names)"""
    if os.path.isfile(spec):
        with open(spec) as f:
            entries = [ln.strip() for ln in f if ln.strip()]
    else:
        entries = [e.strip() for e in spec.split(',') if e.strip()]
    classes = []
    for e in entries:
        names = [n.strip() for n in e.split('|') if n.strip()]
        if not names:
            raise ValueError(f"--classes: empty class in {e!r}")
        classes.append(names[0] if len(names) == 1 else names)
    if not classes:
        raise ValueError("--classes: no class")
    return classes


def build_prompts(classes, templates):
    """classes: list whose entries are a name or a list of synonyms -> (prompts, offsets): for class k every synonym under every
    template (synonym-major), offsets[k] .. offsets[k + 1] its rows"""
    prompts, offsets = [], [0]
    for c in classes:
        names = [c] if isinstance(c, str) else list(c)
        if not names or any(not isinstance(n, str) or not n.strip() for n in names):
            raise ValueError(f"class entry {c!r} must be a non-empty name or a list of them")
        prompts += [t.replace('{}', n.strip()) for n in names for t in templates]
        offsets.append(len(prompts))
    if len(offsets) < 2:
        raise ValueError("no classes")
    return prompts, torch.tensor(offsets, dtype=torch.int64)


def build_vocabulary(classes, templates):
    """An open vocabulary with several names per class.  classes: as build_prompts.  Returns
    (prompts, name_offsets int64 [P + 1], class_offsets int64 [K + 1], names): one row PER NAME -- encode_classes(ids,
    name_offsets) pools a name's templates, CLIP's ensemble -- and class k owns the names class_offsets[k] ... class_offsets[k + 1]
    - 1, the contiguous groups hip.segment_render / hip.vocab_render merge by their maximum.  names: the K lists of names."""
    names = []
    for c in classes:
        group = [c] if isinstance(c, str) else list(c)
        if not group or any(not isinstance(n, str) or not n.strip() for n in group):
            raise ValueError(f"class entry {c!r} must be a non-empty name or a list of them")
        names.append([n.strip() for n in group])
    if not names:
        raise ValueError("no classes")
    prompts, name_offsets = build_prompts([n for group in names for n in group], templates)
    class_offsets = [0]
    for group in names:
        class_offsets.append(class_offsets[-1] + len(group))
    return prompts, name_offsets, torch.tensor(class_offsets, dtype=torch.int64), names


@torch.no_grad()
def compute_text_embeddings(checkpoint, bpe_path, classes, templates='single', device='cuda'):
    """the whole pipeline: checkpoint + merges file + class list -> fp32 [K, embed_dim] unit rows on the CPU"""
    from .clip_tokenizer import CLIPTokenizer
    model = load_clip_text_checkpoint(checkpoint, device)
    prompts, offsets = build_prompts(classes, read_templates(templates))
    ids = CLIPTokenizer(bpe_path).tokenize(prompts, context_length=model.context_length)
    return model.encode_classes(ids, offsets).cpu()
