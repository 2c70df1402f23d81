"""Host-side checks of CLIP's text tower (K29): every OESS_EINVAL of the five new entries by calls that cannot launch, the
wrappers' refusals (a ValueError naming the operand, before the device check), the model's construction and checkpoint forms, the
`text_classes` settings keys, what the trainers refuse before anything is built, and the shipped YAML.  No GPU."""
import ctypes
import os

import pytest
import torch
import yaml

from tests import clip_text_reference as cr

EINVAL = -22
CFG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")
CFG = os.path.join(CFG_DIR, "pretrain_dsec_synthetic.yaml")
SIBLING = os.path.join(CFG_DIR, "pretrain_dsec_synthetic_online_maskclip_fp32.yaml")
EXAMPLE = os.path.join(CFG_DIR, "pretrain_dsec_synthetic_online_maskclip_text_classes.yaml")


def _aligned():
    buf = ctypes.create_string_buffer(1 << 16)
    addr = ctypes.addressof(buf)
    return buf, addr + (-addr) % 16


# --------------------------------------------------------------------------------------------- raw entries, no launch
def test_causal_attention_entry_validates_arguments_before_any_launch():
    from openess_amd import _lib
    att = _lib.load().oess_attention_d64_causal_f32
    buf, a = _aligned()

    def call(qkv=a, qs=3 * 128, B=2, L=9, heads=2, scale=0.125, out=a, os_=128):
        return att(qkv, qs, B, L, heads, scale, out, os_, None)

    for bad in (dict(L=0), dict(L=-1), dict(heads=0), dict(heads=-1), dict(B=0), dict(B=-2), dict(qs=3 * 128 - 4), dict(qs=3 * 128 + 2),
                dict(qs=3 * 128 + 1), dict(os_=124), dict(os_=130), dict(qkv=a + 8), dict(qkv=a + 4), dict(out=a + 8), dict(out=a + 4),
                dict(qkv=None), dict(out=None), dict(scale=0.0), dict(scale=-0.125), dict(scale=float("inf")), dict(scale=float("nan")),
                dict(B=1 << 16, L=1 << 15), dict(qs=1 << 31), dict(os_=1 << 31), dict(heads=(1 << 20) + 1, qs=1 << 30, os_=1 << 30),
                dict(B=1 << 11, L=1 << 19, heads=1 << 10, qs=3 << 16, os_=1 << 16)):
        assert call(**bad) == EINVAL, bad
    del buf


def test_embed_entry_validates_arguments_before_any_launch():
    from openess_amd import _lib
    emb = _lib.load().oess_clip_text_embed_f32
    buf, a = _aligned()

    def call(ids=a, N=2, L=7, table=a, ts=64, V=50, C=64, pos=a, ps=64, out=a, os_=64):
        return emb(ids, N, L, table, ts, V, C, pos, ps, out, os_, None)

    for bad in (dict(ids=None), dict(table=None), dict(pos=None), dict(out=None), dict(N=0), dict(N=-1), dict(L=0), dict(L=-3), dict(V=0),
                dict(V=-1), dict(C=0), dict(C=-64), dict(C=(1 << 20) + 4, ts=1 << 21, ps=1 << 21, os_=1 << 21), dict(ts=63), dict(ps=63),
                dict(os_=63), dict(ts=1 << 31), dict(ps=1 << 31), dict(os_=1 << 31), dict(ids=a + 4), dict(table=a + 2), dict(pos=a + 1),
                dict(out=a + 3), dict(N=1 << 16, L=1 << 15)):
        assert call(**bad) == EINVAL, bad
    del buf


def test_quick_gelu_entry_validates_arguments_before_any_launch():
    from openess_amd import _lib
    lin = _lib.load().oess_linear_tokens_quick_gelu_f32
    buf, a = _aligned()

    def call(x=a, xs=24, rows=5, Cin=24, w=a, bias=a, Cout=11, res=a, rs=11, out=a, os_=11):
        return lin(x, xs, rows, Cin, w, bias, Cout, res, rs, out, os_, None)

    for bad in (dict(x=None), dict(w=None), dict(out=None), dict(rows=0), dict(rows=-1), dict(rows=1 << 31), dict(Cin=0), dict(Cin=-1),
                dict(Cin=(1 << 20) + 1, xs=1 << 21), dict(Cout=0), dict(Cout=-3), dict(xs=23), dict(os_=10), dict(rs=10), dict(w=a + 4),
                dict(w=a + 8), dict(bias=a + 2), dict(res=a + 1), dict(xs=1 << 31), dict(os_=1 << 31), dict(rs=1 << 31)):
        assert call(**bad) == EINVAL, bad
    plain = _lib.load().oess_linear_tokens_f32                                  # the QuickGELU is no `act` of the plain entry
    assert plain(a, 24, 5, 24, a, a, 11, 2, a, 11, a, 11, None) == EINVAL
    del buf


def test_eot_layernorm_entry_validates_arguments_before_any_launch():
    from openess_amd import _lib
    eot = _lib.load().oess_clip_text_eot_layernorm_f32
    buf, a = _aligned()

    def call(x=a, xs=512, ids=a, N=3, L=77, C=512, gamma=a, beta=a, eps=1e-5, y=a, ys=512):
        return eot(x, xs, ids, N, L, C, gamma, beta, eps, y, ys, None)

    for bad in (dict(x=None), dict(ids=None), dict(y=None), dict(gamma=None), dict(beta=None), dict(N=0), dict(N=-1), dict(L=0), dict(L=-1),
                dict(C=0), dict(C=-4), dict(C=2049, xs=2052, ys=2052), dict(xs=511), dict(ys=511), dict(eps=0.0), dict(eps=-1e-5),
                dict(eps=float("nan")), dict(x=a + 2), dict(y=a + 1), dict(gamma=a + 3), dict(beta=a + 2), dict(ids=a + 4),
                dict(xs=1 << 31), dict(ys=1 << 31), dict(N=1 << 16, L=1 << 15)):
        assert call(**bad) == EINVAL, bad
    del buf


def test_prompt_mean_entry_validates_arguments_before_any_launch():
    from openess_amd import _lib
    pm = _lib.load().oess_prompt_mean_normalize_f32
    buf, a = _aligned()

    def offsets(*v):
        return (ctypes.c_int64 * len(v))(*v)

    good = offsets(0, 1, 3, 10)

    def call(e=a, es=512, N=10, D=512, host=good, dev=a, K=3, out=a, os_=512):
        return pm(e, es, N, D, host if host is None or isinstance(host, int) else ctypes.addressof(host), dev, K, out, os_, None)

    for bad in (dict(e=None), dict(host=None), dict(dev=None), dict(out=None), dict(N=0), dict(N=-1), dict(N=1 << 31), dict(D=0), dict(D=-1),
                dict(D=2049, es=2052, os_=2052), dict(K=0), dict(K=-1), dict(es=511), dict(os_=511), dict(es=1 << 31), dict(os_=1 << 31),
                dict(e=a + 2), dict(out=a + 1), dict(dev=a + 4), dict(host=ctypes.addressof(good) + 4),
                dict(host=offsets(1, 2, 3, 10)), dict(host=offsets(0, 1, 3, 9)), dict(host=offsets(0, 1, 3, 11)),
                dict(host=offsets(0, 3, 3, 10)), dict(host=offsets(0, 4, 3, 10)), dict(host=offsets(0, 1, 3, 10), N=11),
                dict(host=offsets(0, -1, 3, 10))):
        assert call(**bad) == EINVAL, bad
    del buf


# --------------------------------------------------------------------------------------------- wrappers
def test_attention_causal_flag_refusals():
    from openess_amd import hip
    qkv = torch.zeros(5, 192)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="causal must be a bool"):
            hip.attention_d64_f32(qkv, 1, 5, 1, causal=bad)
    for flag in (False, True):
        with pytest.raises(ValueError, match="attention_d64_f32: qkv "):
            hip.attention_d64_f32(qkv[:, :-4], 1, 5, 1, causal=flag)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            hip.attention_d64_f32(qkv, 1, 5, 1, causal=flag)


def test_linear_tokens_quick_gelu_route_checks_like_its_neighbours():
    from openess_amd import hip
    x = torch.zeros(5, 24)
    packed = hip.pack_conv_weight_f32(torch.zeros(11, 24, 1, 1))
    with pytest.raises(ValueError, match="linear_tokens_f32: x "):
        hip.linear_tokens_f32(x.double(), packed, None, 11, act='quick_gelu')
    with pytest.raises(ValueError, match="act must be one of"):
        hip.linear_tokens_f32(x, packed, None, 11, act='quickgelu')
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.linear_tokens_f32(x, packed, None, 11, act='quick_gelu')


def test_clip_text_embed_refusals():
    from openess_amd import hip
    V, C, N, L = 20, 64, 2, 5
    table, pos, ids = torch.zeros(V, C), torch.zeros(8, C), torch.zeros(N, L, dtype=torch.int64)
    for bad in (table.double(), table[0], torch.zeros(V, 2 * C)[:, ::2], None):
        with pytest.raises(ValueError, match="clip_text_embed: token_embedding "):
            hip.clip_text_embed(ids, bad, pos)
    for bad in (ids.int(), ids[0], ids.float(), torch.zeros(N, 2 * L, dtype=torch.int64)[:, ::2], ids.to("meta"), None):
        with pytest.raises(ValueError, match="clip_text_embed: ids "):
            hip.clip_text_embed(bad, table, pos)
    for bad in (pos.double(), torch.zeros(8, C + 4), pos[0], pos.to("meta"), None):
        with pytest.raises(ValueError, match="clip_text_embed: positional_embedding "):
            hip.clip_text_embed(ids, table, bad)
    with pytest.raises(ValueError, match="5 tokens per text, positional_embedding has 4 rows"):
        hip.clip_text_embed(ids, table, pos[:4])
    for v in (-1, V, 1 << 40):
        bad = ids.clone()
        bad[1, 3] = v
        with pytest.raises(ValueError, match="ids must lie in"):
            hip.clip_text_embed(bad, table, pos)
    for o in (torch.empty(N * L, C).double(), torch.empty(N * L + 1, C), torch.empty(N * L, C + 4), torch.empty(N * L, C, device="meta")):
        with pytest.raises(ValueError, match="clip_text_embed: out "):
            hip.clip_text_embed(ids, table, pos, out=o)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.clip_text_embed(ids, table, pos)


def test_clip_text_eot_norm_refusals():
    from openess_amd import hip
    N, L, C = 2, 5, 64
    x, ids, g, b = torch.zeros(N * L, C), torch.zeros(N, L, dtype=torch.int64), torch.ones(C), torch.zeros(C)
    for bad in (x.double(), x[0], x[:-1], torch.zeros(N * L, 2 * C)[:, ::2], torch.zeros(N * L, 2052), None):
        with pytest.raises(ValueError, match="clip_text_eot_norm: x "):
            hip.clip_text_eot_norm(bad, ids, g, b)
    for bad in (ids.int(), ids[0], ids.to("meta"), None):
        with pytest.raises(ValueError, match="clip_text_eot_norm: ids "):
            hip.clip_text_eot_norm(x, bad, g, b)
    for p in (g.double(), torch.ones(C + 1), torch.ones(2 * C)[::2], g.to("meta"), None):
        with pytest.raises(ValueError, match="gamma must be contiguous fp32"):
            hip.clip_text_eot_norm(x, ids, p, b)
        with pytest.raises(ValueError, match="beta must be contiguous fp32"):
            hip.clip_text_eot_norm(x, ids, g, p)
    for eps in (0.0, -1e-5, float("nan")):
        with pytest.raises(ValueError, match="eps"):
            hip.clip_text_eot_norm(x, ids, g, b, eps=eps)
    for o in (torch.empty(N, C).double(), torch.empty(N + 1, C), torch.empty(N, C - 4), torch.empty(N, C, device="meta")):
        with pytest.raises(ValueError, match="clip_text_eot_norm: out "):
            hip.clip_text_eot_norm(x, ids, g, b, out=o)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.clip_text_eot_norm(x, ids, g, b)


def test_prompt_mean_normalize_refusals():
    from openess_amd import hip
    e = torch.ones(6, 32)
    off = torch.tensor([0, 2, 6])
    for bad in (e.double(), e[0], torch.ones(6, 64)[:, ::2], torch.ones(6, 2052), torch.ones(0, 32), None):
        with pytest.raises(ValueError, match="prompt_mean_normalize: e "):
            hip.prompt_mean_normalize(bad, off)
    for bad in (off.int(), off[None], torch.tensor([0]), off.tolist(), None):
        with pytest.raises(ValueError, match="group_offsets must be int64"):
            hip.prompt_mean_normalize(e, bad)
    for bad in ([1, 2, 6], [0, 2, 5], [0, 2, 7], [0, 2, 2, 6], [0, 4, 2, 6], [0, -1, 6]):
        with pytest.raises(ValueError, match="ascend strictly from 0 to 6"):
            hip.prompt_mean_normalize(e, torch.tensor(bad))
    for o in (torch.empty(2, 32).double(), torch.empty(3, 32), torch.empty(2, 36), torch.empty(2, 32, device="meta")):
        with pytest.raises(ValueError, match="prompt_mean_normalize: out "):
            hip.prompt_mean_normalize(e, off, out=o)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.prompt_mean_normalize(e, off)


# --------------------------------------------------------------------------------------------- model, checkpoints
def test_encoder_has_openai_names_and_refuses_other_head_sizes():
    from openess_amd.models.clip_text import CLIPTextEncoder
    m = CLIPTextEncoder(**cr.TOWER_SMALL)
    keys = list(m.state_dict())
    want = ["token_embedding.weight", "positional_embedding", "text_projection", "ln_final.weight", "ln_final.bias"]
    for i in range(2):
        want += [f"transformer.resblocks.{i}.{k}" for k in
                 ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "ln_1.weight", "ln_1.bias",
                  "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias", "ln_2.weight", "ln_2.bias")]
    assert sorted(keys) == sorted(want) and sorted(cr.tower_state("small")) == sorted(want)
    assert not any(p.requires_grad for p in m.parameters()) and not m.training
    m.load_state_dict(cr.tower_state("small"), strict=True)
    full = CLIPTextEncoder()
    assert full.token_embedding.weight.shape == (49408, 512) and full.positional_embedding.shape == (77, 512)
    assert len(full.transformer.resblocks) == 12 and full.text_projection.shape == (512, 512)
    for kw in (dict(width=512, heads=4), dict(width=500, heads=8), dict(width=128, heads=8)):
        with pytest.raises(ValueError, match="heads of 64"):
            CLIPTextEncoder(**{**cr.TOWER_SMALL, **kw})
    for kw in (dict(layers=0), dict(vocab_size=-1), dict(embed_dim=1.5), dict(context_length=True)):
        with pytest.raises(ValueError, match="positive integer"):
            CLIPTextEncoder(**{**cr.TOWER_SMALL, **kw})
    for bad in (torch.zeros(2, 16), torch.zeros(16, dtype=torch.int64), torch.zeros(2, 17, dtype=torch.int64)):
        with pytest.raises(ValueError, match="CLIPTextEncoder"):
            m.forward_fp32(bad)


def _hf_from_openai(sd, layers):
    """the inverse of convert_hf_state_dict, written out key by key"""
    W = sd["positional_embedding"].shape[1]
    out = {"text_model.embeddings.token_embedding.weight": sd["token_embedding.weight"],
           "text_model.embeddings.position_embedding.weight": sd["positional_embedding"],
           "text_model.final_layer_norm.weight": sd["ln_final.weight"], "text_model.final_layer_norm.bias": sd["ln_final.bias"],
           "text_projection.weight": sd["text_projection"].T.contiguous()}
    for i in range(layers):
        s, d = f"transformer.resblocks.{i}.", f"text_model.encoder.layers.{i}."
        for t in ("weight", "bias"):
            for j, n in enumerate("qkv"):
                out[f"{d}self_attn.{n}_proj.{t}"] = sd[f"{s}attn.in_proj_{t}"][j * W:(j + 1) * W]
            out[f"{d}self_attn.out_proj.{t}"] = sd[f"{s}attn.out_proj.{t}"]
            out[f"{d}layer_norm1.{t}"], out[f"{d}layer_norm2.{t}"] = sd[f"{s}ln_1.{t}"], sd[f"{s}ln_2.{t}"]
            out[f"{d}mlp.fc1.{t}"], out[f"{d}mlp.fc2.{t}"] = sd[f"{s}mlp.c_fc.{t}"], sd[f"{s}mlp.c_proj.{t}"]
    return out


def test_checkpoint_forms_load_to_the_same_weights(tmp_path):
    from openess_amd.models.clip_text import convert_hf_state_dict, load_clip_text_checkpoint
    sd = cr.tower_state("small")
    hf = _hf_from_openai(sd, 2)
    back = convert_hf_state_dict(hf)
    assert sorted(back) == sorted(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(ValueError, match="no text_model.encoder.layers"):
        convert_hf_state_dict({k: v for k, v in hf.items() if "encoder.layers" not in k})
    full = dict(sd, **{"visual.proj": torch.zeros(3, 3), "visual.conv1.weight": torch.zeros(2, 3, 4, 4), "logit_scale": torch.tensor(1.0),
                       "input_resolution": torch.tensor(224), "context_length": torch.tensor(16), "vocab_size": torch.tensor(64)})
    forms = {"plain": sd, "full": full, "hf": hf, "wrapped": {"state_dict": full}, "half": {k: v.half() for k, v in full.items()}}
    for name, obj in forms.items():
        torch.save(obj, tmp_path / f"{name}.pt")
        m = load_clip_text_checkpoint(str(tmp_path / f"{name}.pt"))
        assert (m.vocab_size, m.context_length, m.width, m.heads, m.embed_dim, len(m.transformer.resblocks)) == (64, 16, 128, 2, 96, 2)
        got = m.state_dict()
        assert sorted(got) == sorted(sd)
        for k in sd:
            assert got[k].dtype == torch.float32
            assert torch.equal(got[k], sd[k].half().float() if name == "half" else sd[k]), (name, k)
    torch.save({"visual.proj": torch.zeros(3, 3)}, tmp_path / "image_only.pt")
    with pytest.raises(ValueError, match="no CLIP text tower"):
        load_clip_text_checkpoint(str(tmp_path / "image_only.pt"))


def test_prompts_and_templates(tmp_path):
    from openess_amd.models.clip_text import build_prompts, read_templates
    assert read_templates('single') == ['a photo of a {}.'] and read_templates(None) == ['a photo of a {}.'] and read_templates('none') == ['{}']
    (tmp_path / "t.txt").write_text("a photo of a {}.\n\n  a blurry photo of the {}.  \n")
    assert read_templates(str(tmp_path / "t.txt")) == ["a photo of a {}.", "a blurry photo of the {}."]
    (tmp_path / "bad.txt").write_text("a photo of a {}.\na photo\n")
    with pytest.raises(ValueError, match="must contain"):
        read_templates(str(tmp_path / "bad.txt"))
    prompts, off = build_prompts(["road", ["car", "bus"]], ["a {}.", "the {}"])
    assert prompts == ["a road.", "the road", "a car.", "the car", "a bus.", "the bus"] and off.tolist() == [0, 2, 6] and off.dtype == torch.int64
    for bad in ([], [[]], ["road", ""], [["car", 3]]):
        with pytest.raises(ValueError):
            build_prompts(bad, ["{}"])


# --------------------------------------------------------------------------------------------- the figures behind the bounds
def test_committed_figures_are_what_fp32_on_the_cpu_gives():
    """the *_FIGURES constants are tools/exp_clip_text_bounds.py's output: re-measured here within a factor of two either way (a
    BLAS with another blocking moves the last digits, not the magnitude); the bounds are four times the constants"""
    measured = {}
    for B, L, heads in cr.CAUSAL_BOUNDED:
        qkv = cr.causal_bounded_case(B, L, heads)
        measured["causal", B, L, heads] = (cr.rel_max(cr.causal_attention32(qkv, B, L, heads), cr.causal_attention64(qkv, B, L, heads)),
                                           cr.CAUSAL_FIGURES[B, L, heads], cr.CAUSAL_BOUNDS[B, L, heads])
    for shape in cr.QGELU_SHAPES:
        c = cr.qgelu_case(*shape)
        measured[("qgelu",) + shape] = (cr.rel_max(cr.qgelu32(c), cr.qgelu64(c)), cr.QGELU_FIGURES[shape], cr.QGELU_BOUNDS[shape])
    for D in cr.PROMPT_D:
        c = cr.prompt_case(D)
        measured["prompt", D] = (cr.rel_max(cr.prompt_mean32(c["e"], c["offsets"]), cr.prompt_mean64(c["e"], c["offsets"])),
                                 cr.PROMPT_FIGURES[D], cr.PROMPT_BOUNDS[D])
    got = cr.text_encode32(cr.tower_state("small"), cr.tower_ids("small"), 2)
    measured["tower", "small"] = (cr.rel_max(got, cr.tower_reference("small")), cr.TOWER_FIGURES["small"], cr.TOWER_BOUNDS["small"])
    for key, (now, figure, bound) in measured.items():
        assert 0.5 * figure <= now <= 2.0 * figure, (key, now, figure)
        assert bound == 4.0 * figure
    assert cr.TOWER_BOUNDS["real"] == 4.0 * cr.TOWER_FIGURES["real"]


# --------------------------------------------------------------------------------------------- settings keys, trainers, YAML
def _settings(tmp_path, base=CFG, task=None, **clip):
    from openess_amd.config.settings import Settings
    cfg = yaml.load(open(base), yaml.Loader)
    cfg['clip'].update(clip)
    if task:
        cfg['task'].update(task)
    path = tmp_path / "settings.yaml"
    path.write_text(yaml.dump(cfg))
    return Settings(str(path), generate_log=False)


CLASSES = ['background', 'building', 'fence', 'person', 'pole', 'road', 'sidewalk', 'vegetation', ['car', 'vehicle'], 'wall', 'traffic sign']


def test_text_classes_settings_keys(tmp_path):
    s = _settings(tmp_path)
    assert s.text_classes is None and s.clip_text_checkpoint is None and s.clip_bpe_path is None and s.text_templates == 'single'
    s = _settings(tmp_path, text_classes=CLASSES, clip_text_checkpoint='a.pt', clip_bpe_path='m.txt', text_templates='none')
    assert s.text_classes == CLASSES and (s.clip_text_checkpoint, s.clip_bpe_path, s.text_templates) == ('a.pt', 'm.txt', 'none')
    for bad in ('road,car', [], ['road', 3], ['road', []], ['road', ['car', None]], {'road': 1}, ['road', ''], 11):
        with pytest.raises(ValueError, match="text_classes"):
            _settings(tmp_path, text_classes=bad)
    for key in ('clip_text_checkpoint', 'clip_bpe_path'):
        for bad in (3, ['a.pt'], True):
            with pytest.raises(ValueError, match=key):
                _settings(tmp_path, **{key: bad})
    for bad in (None, 3, '', ['single']):
        with pytest.raises(ValueError, match="text_templates"):
            _settings(tmp_path, text_templates=bad)


def test_trainers_refuse_text_classes_without_what_it_needs(tmp_path):
    from openess_amd.training.base_trainer_ov import text_classes_options
    from openess_amd.training.pretrain_trainer import OpenESSPretrainModel
    ckpt, bpe = tmp_path / "c.pt", tmp_path / "m.txt"
    ckpt.write_bytes(b"x")
    bpe.write_text("a b\n")
    good = dict(text_classes=CLASSES, clip_text_checkpoint=str(ckpt), clip_bpe_path=str(bpe))
    assert text_classes_options(_settings(tmp_path)) is None
    assert text_classes_options(_settings(tmp_path, **good)) == {'classes': CLASSES, 'checkpoint': str(ckpt), 'bpe': str(bpe),
                                                                 'templates': 'single'}
    cases = ((dict(good, clip_text_checkpoint=None), "needs clip_text_checkpoint"),
             (dict(good, clip_bpe_path=None), "needs clip_text_checkpoint"),
             (dict(good, clip_bpe_path=''), "needs clip_text_checkpoint"),
             (dict(good, text_embeddings_path=str(ckpt)), "give one of them"),
             (dict(good, clip_text_checkpoint=str(tmp_path / "absent.pt")), "clip_text_checkpoint: .* not found"),
             (dict(good, clip_bpe_path=str(tmp_path / "absent.txt")), "clip_bpe_path: .* not found"),
             (dict(good, text_templates=str(tmp_path / "absent_templates.txt")), "text_templates: .* not found"),
             (dict(good, text_classes=CLASSES[:-1]), "names 10 classes, semseg_num_classes is 11"))
    for clip, msg in cases:
        s = _settings(tmp_path, **clip)
        with pytest.raises(ValueError, match=msg):
            text_classes_options(s)
        with pytest.raises(ValueError, match=msg):                              # before the device check, before any model
            OpenESSPretrainModel(settings=s)


@pytest.mark.parametrize("yaml_name,cls", (("finetune_dsec_synthetic.yaml", "finetune_trainer.OpenESSFineTuneModel"),
                                           ("finetune_dsec_synthetic.yaml", "linear_probe_trainer.OpenESSLinearProbeModel"),
                                           ("finetune_dsec_synthetic.yaml", "sup_only_trainer.SupOnlyModel"),
                                           ("openess_dsec_synthetic.yaml", "openess_trainer.OpenESSModel")))
def test_every_trainer_refuses_before_anything_is_built(tmp_path, yaml_name, cls):
    import importlib
    mod, name = cls.split(".")
    trainer = getattr(importlib.import_module(f"openess_amd.training.{mod}"), name)
    s = _settings(tmp_path, base=os.path.join(CFG_DIR, yaml_name), text_classes=CLASSES)
    with pytest.raises(ValueError, match="needs clip_text_checkpoint"):
        trainer(settings=s)


def test_the_helper_runs_before_init_fn_and_points_the_setting_at_the_file(tmp_path, monkeypatch):
    """with a GPU reported and the tower replaced: the embeddings are written and named before init_fn (buildModels) runs"""
    from openess_amd.training import base_trainer_ov as bt
    from openess_amd.models import clip_text
    ckpt, bpe = tmp_path / "c.pt", tmp_path / "m.txt"
    ckpt.write_bytes(b"x")
    bpe.write_text("a b\n")
    s = _settings(tmp_path, text_classes=CLASSES, clip_text_checkpoint=str(ckpt), clip_bpe_path=str(bpe), text_templates='none')
    emb = torch.nn.functional.normalize(torch.randn(11, 512), dim=1)
    seen = {}

    def fake(checkpoint, bpe_path, classes, templates, device):
        seen['args'] = (checkpoint, bpe_path, classes, templates)
        return emb

    class Stop(Exception):
        pass

    class Trainer(bt.BaseTrainer):
        def init_fn(self):
            seen['path'] = self.settings.text_embeddings_path
            raise Stop

    monkeypatch.setattr(clip_text, 'compute_text_embeddings', fake)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    with pytest.raises(Stop):
        Trainer(settings=s)
    assert seen['args'] == (str(ckpt), str(bpe), CLASSES, 'none')
    assert os.path.isfile(seen['path']) and torch.equal(torch.load(seen['path']), emb)
    os.remove(seen['path'])
    seen.clear()
    with pytest.raises(Stop):                                                    # without the key: nothing is computed
        Trainer(settings=_settings(tmp_path))
    assert 'args' not in seen and seen['path'] == ''


def test_example_yaml_differs_from_its_sibling_by_the_new_keys_alone():
    new = yaml.load(open(EXAMPLE), yaml.Loader)
    old = yaml.load(open(SIBLING), yaml.Loader)
    assert new['clip'].pop('text_classes') == CLASSES
    assert new['clip'].pop('clip_text_checkpoint').endswith('.pt') and new['clip'].pop('clip_bpe_path').endswith('merges.txt')
    assert new['clip'].pop('text_templates') == 'single'
    assert new == old and old['clip']['text_embeddings_path'] == ''
