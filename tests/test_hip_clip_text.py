"""GPU tests of CLIP's text tower in fp32 (K29: openess_amd/csrc/clip_text_f32.hip, the causal and end-of-text instances of
vit_f32.hip, the QuickGELU epilogue of conv_f32.hip, openess_amd/models/clip_text.py, tools/write_text_embeddings.py) on the cases
of tests/clip_text_reference.py:

  * causal attention, exact: selection (the selected key <= the query) and constant-V cases bit for bit, row 0 of every sequence
    its V row, NaN rows behind the buffer, row-strided operands with NaN gaps; future keys overwritten by large finite values
    leave the earlier queries' bits alone; non-bf16-exact operands against float64; two runs give equal bits;
  * embedding, QuickGELU GEMM, end-of-text LayerNorm, prompt ensemble: exact where the arithmetic is, float64-bounded elsewhere;
  * the tower at a small and at the real geometry against the float64 restatement; the tool end to end; a trainer from the YAML.

Every bound is four times what torch fp32 on the CPU gives against float64 on the same case (tools/exp_clip_text_bounds.py);
nothing the kernels produce went into one.  No element is left out of a comparison."""
import math
import os

import pytest
import torch

from tests import clip_text_reference as cr
from tests import vit_token_cases as vc

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "configs")
EXACT = [(f, B, L, h) for f in ("selection", "constant_v") for (B, h) in cr.CAUSAL_BH for L in cr.CAUSAL_L]


# --------------------------------------------------------------------------------------------- causal attention
def _exact(family, B, L, heads, extra_cols=0, out_cols=0):
    from openess_amd import hip
    c = cr.causal_exact_case(family, B, L, heads)
    C = heads * 64
    buf, qkv = vc.embed(c["qkv"], vc.NAN_TAIL_ROWS, extra_cols, math.nan, DEV)
    assert qkv.data_ptr() % 16 == 0 and (B * L == 1 or qkv.stride(0) == 3 * C + extra_cols)
    obuf = torch.full((B * L, C + out_cols), cr.SENTINEL, dtype=torch.float32, device=DEV)
    o = hip.attention_d64_f32(qkv, B, L, heads, out=obuf[:, :C], causal=True)
    assert o.data_ptr() == obuf.data_ptr() and o.dtype == torch.float32
    got = o.cpu()
    assert not bool(torch.isnan(got).any()), "NaN: a masked key's V row or a row past B L reached the output"
    wrong = (got != c["expect"]).any(dim=1).nonzero().flatten().tolist()
    assert torch.equal(got, c["expect"]), f"{family} B={B} L={L} heads={heads}: {len(wrong)} rows differ, first {wrong[:8]}"
    first = got.view(B, L, C)[:, 0]
    assert torch.equal(first, c["qkv"][:, 2 * C:].view(B, L, C)[:, 0]), "row 0 of a sequence is its V row"
    assert bool((obuf[:, C:] == cr.SENTINEL).all())
    assert bool(torch.isnan(buf[B * L:]).all()) and bool(torch.isnan(buf[:, 3 * C:]).all())


@pytest.mark.parametrize("family,B,L,heads", EXACT)
def test_causal_attention_exact(family, B, L, heads):
    _exact(family, B, L, heads)


@pytest.mark.parametrize("family", ("selection", "constant_v"))
@pytest.mark.parametrize("L", (77, 129, 200))
def test_causal_attention_exact_with_row_strides(family, L):
    _exact(family, 3, L, 2, extra_cols=cr.CAUSAL_STRIDE_EXTRA, out_cols=cr.CAUSAL_OUT_EXTRA)


@pytest.mark.parametrize("L,j", cr.LEAK_CASES)
def test_future_keys_do_not_leak(L, j):
    """K and V of every key > j replaced by large finite values (a diagonal tile multiplies them by an exact zero; NaN would
    not survive that): the outputs of the queries <= j keep their bits"""
    from openess_amd import hip
    B, heads = 2, 2
    C = heads * 64
    qkv = (torch.randn(B * L, 3 * C, generator=cr._gen("leak", L, j)) * 1.5).to(DEV)
    base = hip.attention_d64_f32(qkv, B, L, heads, causal=True)
    assert bool(torch.isfinite(base).all())
    mod = qkv.clone()
    mod.view(B, L, 3 * C)[:, j + 1:, C:] = 1e18
    got = hip.attention_d64_f32(mod, B, L, heads, causal=True)
    assert torch.equal(got.view(B, L, C)[:, :j + 1], base.view(B, L, C)[:, :j + 1]), "a future key reached a query"
    assert not torch.equal(got.view(B, L, C)[:, j + 1:], base.view(B, L, C)[:, j + 1:])           # the change is seen where it may be


@pytest.mark.parametrize("B,L,heads", cr.CAUSAL_BOUNDED)
def test_causal_attention_within_the_float64_bound(B, L, heads):
    from openess_amd import hip
    qkv = cr.causal_bounded_case(B, L, heads)
    dev = qkv.to(DEV)
    plain_before = hip.attention_d64_f32(dev, B, L, heads)
    o = hip.attention_d64_f32(dev, B, L, heads, causal=True)
    err = cr.rel_max(o, cr.causal_attention64(qkv, B, L, heads))
    print(f"causal attention {(B, L, heads)}: err {err:.3e} (figure {cr.CAUSAL_FIGURES[B, L, heads]:.3e}, "
          f"bound {cr.CAUSAL_BOUNDS[B, L, heads]:.3e})")
    assert err <= cr.CAUSAL_BOUNDS[B, L, heads]
    assert torch.equal(hip.attention_d64_f32(dev, B, L, heads, causal=True), o), "two runs differ"
    assert torch.equal(hip.attention_d64_f32(dev, B, L, heads), plain_before), "the plain entry moved"
    assert not torch.equal(plain_before, o)


# --------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("C", cr.EMBED_C)
def test_embedding_is_exact(C):
    from openess_amd import hip
    g = cr._gen("embed", C)
    V, N, L, P = 97, 5, 13, 16
    table, pos = torch.randn(V, C, generator=g), torch.randn(P, C, generator=g)
    ids = torch.randint(0, V, (N, L), generator=g)
    ids[0, 0], ids[-1, -1] = 0, V - 1
    got = hip.clip_text_embed(ids.to(DEV), table.to(DEV), pos.to(DEV))
    assert got.shape == (N * L, C) and torch.equal(got.cpu(), (table[ids] + pos[:L]).view(N * L, C))
    for bad in (ids.clone().index_put_((torch.tensor(1), torch.tensor(2)), torch.tensor(V)),
                ids.clone().index_put_((torch.tensor(1), torch.tensor(2)), torch.tensor(-1))):
        with pytest.raises(ValueError, match="ids must lie in"):
            hip.clip_text_embed(bad.to(DEV), table.to(DEV), pos.to(DEV))
    with pytest.raises(ValueError, match="tokens per text"):
        hip.clip_text_embed(ids.to(DEV), table.to(DEV), pos[:L - 1].to(DEV))


def test_embedding_with_row_strides():
    from openess_amd import hip
    g = cr._gen("embed_strided")
    V, N, L, C = 31, 3, 7, 64
    tbuf, pbuf = torch.randn(V, C + 4, generator=g), torch.randn(L, C + 8, generator=g)
    ids = torch.randint(0, V, (N, L), generator=g)
    obuf = torch.full((N * L, C + 4), cr.SENTINEL, device=DEV)
    got = hip.clip_text_embed(ids.to(DEV), tbuf.to(DEV)[:, :C], pbuf.to(DEV)[:, :C], out=obuf[:, :C])
    assert torch.equal(got.cpu(), (tbuf[:, :C][ids] + pbuf[:, :C]).view(N * L, C)) and bool((obuf[:, C:] == cr.SENTINEL).all())


# --------------------------------------------------------------------------------------------- QuickGELU GEMM
@pytest.mark.parametrize("rows,Cin,Cout", cr.QGELU_SHAPES)
def test_quick_gelu_linear_within_the_float64_bound(rows, Cin, Cout):
    from openess_amd import hip
    c = cr.qgelu_case(rows, Cin, Cout)
    packed = hip.pack_conv_weight_f32(c["w"][:, :, None, None].to(DEV))
    y = hip.linear_tokens_f32(c["x"].to(DEV), packed, c["b"].to(DEV), Cout, act='quick_gelu')
    err = cr.rel_max(y, cr.qgelu64(c))
    print(f"quick_gelu linear {(rows, Cin, Cout)}: err {err:.3e} (figure {cr.QGELU_FIGURES[rows, Cin, Cout]:.3e}, "
          f"bound {cr.QGELU_BOUNDS[rows, Cin, Cout]:.3e})")
    assert err <= cr.QGELU_BOUNDS[rows, Cin, Cout]
    assert torch.equal(hip.linear_tokens_f32(c["x"].to(DEV), packed, c["b"].to(DEV), Cout, act='quick_gelu'), y)


@pytest.mark.parametrize("rows,Cin,Cout", cr.QGELU_SHAPES)
def test_quick_gelu_linear_on_integers(rows, Cin, Cout):
    """integer operands: the pre-activation v is exact, so the result is fp32 v / (1 + expf(-1.702 v)) to the last bits of expf,
    and exactly 0 where v is 0; a residual enters before the activation"""
    from openess_amd import hip
    c = cr.qgelu_int_case(rows, Cin, Cout)
    packed = hip.pack_conv_weight_f32(c["w"][:, :, None, None].to(DEV))
    v = (c["x"].double() @ c["w"].double().T + c["b"].double())
    y = hip.linear_tokens_f32(c["x"].to(DEV), packed, c["b"].to(DEV), Cout, act='quick_gelu').cpu()
    assert bool((y[v == 0] == 0).all()) and bool((v[:, 0] == 0).all()) and int((v == 0).sum()) >= rows
    assert cr.rel_max(y, cr.quick_gelu64(v)) <= 4.0 * 2.0 ** -24                # one division and one expf on exact operands
    res = -v.float()                                                            # v + residual = 0 everywhere
    z = hip.linear_tokens_f32(c["x"].to(DEV), packed, c["b"].to(DEV), Cout, act='quick_gelu', residual=res.to(DEV))
    assert bool((z == 0).all())


# --------------------------------------------------------------------------------------------- end-of-text LayerNorm
@pytest.mark.parametrize("N,L,C", cr.EOT_CASES)
def test_eot_norm_picks_the_first_maximum_and_equals_the_layernorm_kernel(N, L, C):
    from openess_amd import hip
    c = cr.eot_case(N, L, C)
    x, g, b, ids = c["x"].to(DEV), c["gamma"].to(DEV), c["beta"].to(DEV), c["ids"].to(DEV)
    got = hip.clip_text_eot_norm(x, ids, g, b, 1e-5)
    rows = x.view(N, L, C)[torch.arange(N), c["pos"].to(DEV)].contiguous()
    want = hip.layer_norm_tokens_f32(rows, g, b, 1e-5)
    assert got.shape == (N, C) and torch.equal(got, want)
    ref = torch.nn.functional.layer_norm(c["x"].double().view(N, L, C)[torch.arange(N), c["pos"]], (C,), c["gamma"].double(),
                                         c["beta"].double(), 1e-5)
    assert cr.rel_max(got, ref) <= 4.0 * 2.0 ** -22                             # the kernel itself is held by tests/test_hip_vit_f32.py
    assert torch.equal(hip.clip_text_eot_norm(x, ids, g, b, 1e-5), got)


# --------------------------------------------------------------------------------------------- prompt ensemble
@pytest.mark.parametrize("D", cr.PROMPT_D)
def test_prompt_mean_normalize(D):
    from openess_amd import hip
    c = cr.prompt_case(D)
    e, off = c["e"].to(DEV), c["offsets"]
    got = hip.prompt_mean_normalize(e, off)
    ref = cr.prompt_mean64(c["e"], off)
    err = cr.rel_max(got, ref)
    print(f"prompt mean D={D}: err {err:.3e} (figure {cr.PROMPT_FIGURES[D]:.3e}, bound {cr.PROMPT_BOUNDS[D]:.3e})")
    assert err <= cr.PROMPT_BOUNDS[D]
    assert float((got.double().norm(dim=1) - 1.0).abs().max()) <= 4.0 * 2.0 ** -24
    for k, n in enumerate(cr.PROMPT_GROUPS):                                    # a single prompt: plain normalisation
        if n == 1:
            row = c["e"][int(off[k])]
            alone = hip.prompt_mean_normalize(row[None].to(DEV), torch.tensor([0, 1]))
            assert torch.equal(alone[0], got[k])
            assert cr.rel_max(got[k], row.double() / row.double().norm()) <= 4.0 * 2.0 ** -24
    assert torch.equal(hip.prompt_mean_normalize(e, off.to(DEV)), got), "two runs (offsets on the device) differ"
    for bad in (torch.tensor([0, 3, 3, int(off[-1])]), torch.tensor([1, int(off[-1])]), torch.tensor([0, int(off[-1]) - 1])):
        with pytest.raises(ValueError, match="ascend strictly"):
            hip.prompt_mean_normalize(e, bad)


# --------------------------------------------------------------------------------------------- tower
def _tower(name):
    from openess_amd.models.clip_text import CLIPTextEncoder
    m = CLIPTextEncoder(**cr.TOWER_CASES[name][0])
    m.load_state_dict(cr.tower_state(name), strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("name", tuple(cr.TOWER_CASES))
def test_tower_within_the_float64_bound(name):
    geo, N, L = cr.TOWER_CASES[name]
    m = _tower(name)
    ids = cr.tower_ids(name)
    ref = cr.tower_reference(name)
    got = m.forward_fp32(ids.to(DEV))
    assert got.shape == (N, geo["embed_dim"]) and got.dtype == torch.float32
    err = cr.rel_max(got, ref)
    print(f"text tower {name}: err {err:.3e} (figure {cr.TOWER_FIGURES[name]:.3e}, bound {cr.TOWER_BOUNDS[name]:.3e})")
    assert err <= cr.TOWER_BOUNDS[name]
    assert torch.equal(m.forward_fp32(ids.to(DEV)), got), "two calls differ"
    # what follows the end-of-text token cannot reach it
    other = ids.clone()
    g = cr._gen("tower_tail", name)
    for n in range(N):
        t = int(ids[n].argmax())
        other[n, t + 1:] = torch.randint(1, geo["vocab_size"] - 2, (L - t - 1,), generator=g)
    assert not torch.equal(other, ids)
    assert torch.equal(m.forward_fp32(other.to(DEV)), got), "ids behind the end-of-text token changed the embedding"
    # classes: the prompt ensemble over the same prompts
    off = cr.tower_offsets(name)
    cls = m.encode_classes(ids, off)
    assert cr.rel_max(cls, cr.prompt_mean64(ref, off)) <= cr.TOWER_BOUNDS[name] + 4.0 * cr.PROMPT_FIGURES[geo["embed_dim"]]
    assert float((cls.double().norm(dim=1) - 1.0).abs().max()) <= 4.0 * 2.0 ** -24


def test_tower_sees_a_weight_changed_in_place():
    m = _tower("small")
    ids = cr.tower_ids("small").to(DEV)
    before = m.forward_fp32(ids)
    sd = {k: v.clone() for k, v in cr.tower_state("small").items()}
    for key in ("transformer.resblocks.1.mlp.c_fc.weight", "text_projection"):
        with torch.no_grad():
            dict(m.named_parameters())[key].mul_(1.25)
        sd[key] = sd[key] * 1.25
        now = m.forward_fp32(ids)
        assert not torch.equal(now, before), key
        assert cr.rel_max(now, cr.text_encode64(sd, ids.cpu(), 2)) <= cr.TOWER_BOUNDS["small"], key
        before = now


# --------------------------------------------------------------------------------------------- tool, trainer
def test_tool_writes_a_file_the_consumers_load(tmp_path):
    import importlib.util
    from openess_amd.models.clip_text import build_prompts, load_clip_text_checkpoint
    from openess_amd.models.clip_tokenizer import CLIPTokenizer
    from openess_amd.models.deeplabv3 import deeplabv3_resnet50
    spec = importlib.util.spec_from_file_location("write_text_embeddings", os.path.join(ROOT, "tools", "write_text_embeddings.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ckpt = cr.write_synthetic_checkpoint(tmp_path / "clip.pt")
    bpe = cr.write_merges(tmp_path / "merges.txt")
    (tmp_path / "classes.txt").write_text("road\ncar|a cab\nbroad road\n")
    (tmp_path / "templates.txt").write_text("a photo of a {}.\n{} on the road\n")
    out = tmp_path / "text.pt"
    tool.main(["--checkpoint", ckpt, "--bpe", bpe, "--classes", str(tmp_path / "classes.txt"), "--templates",
               str(tmp_path / "templates.txt"), "--out", str(out)])
    emb = torch.load(out, map_location="cpu")
    assert emb.shape == (3, 512) and emb.dtype == torch.float32
    prompts, off = build_prompts(["road", ["car", "a cab"], "broad road"], ["a photo of a {}.", "{} on the road"])
    assert off.tolist() == [0, 2, 6, 8] and prompts[2] == "a photo of a car." and prompts[5] == "a cab on the road"
    m = load_clip_text_checkpoint(ckpt, DEV)
    assert torch.equal(m.encode_classes(CLIPTokenizer(bpe).tokenize(prompts), off).cpu(), emb)
    assert float((emb[0] - emb[2]).abs().max()) > 1e-3                           # the classes differ
    net = deeplabv3_resnet50(num_classes=3, text_embeddings_path=str(out), output_stride=32, pretrained_backbone='')
    assert torch.equal(net.classifier.text_embeddings.detach().cpu().float().view(3, 512), emb)
    tool.main(["--checkpoint", ckpt, "--bpe", bpe, "--classes", "road,car|a cab,broad road", "--templates",
               str(tmp_path / "templates.txt"), "--out", str(tmp_path / "again.pt")])
    assert torch.equal(torch.load(tmp_path / "again.pt"), emb)


def test_a_yaml_with_text_classes_trains_without_an_embeddings_file(tmp_path):
    import yaml
    import train
    from openess_amd.config.settings import Settings
    cfg = yaml.load(open(os.path.join(CFG, "pretrain_dsec_synthetic_online_maskclip_text_classes.yaml")), yaml.Loader)
    for key in ("clip_text_checkpoint", "clip_bpe_path"):
        os.makedirs(os.path.dirname(cfg["clip"][key]), exist_ok=True)
    ckpt = cr.write_synthetic_checkpoint(cfg["clip"]["clip_text_checkpoint"])
    bpe = cr.write_merges(cfg["clip"]["clip_bpe_path"])
    train.seed_everything()
    s = Settings(os.path.join(CFG, "pretrain_dsec_synthetic_online_maskclip_text_classes.yaml"), generate_log=False)
    s.ckpt_dir = str(tmp_path)
    assert s.text_embeddings_path == ''
    trainer, loop = train.build_trainer(s)
    assert loop == 'pretraining' and os.path.isfile(s.text_embeddings_path)
    emb = torch.load(s.text_embeddings_path, map_location="cpu")
    from openess_amd.models.clip_text import compute_text_embeddings
    assert emb.shape == (11, 512) and torch.equal(emb, compute_text_embeddings(ckpt, bpe, s.text_classes, 'single', DEV))
    back = trainer.models_dict['back_end']
    assert torch.equal(back.text_embeddings.detach().cpu().float().view(11, 512), emb)
    batch = trainer.prepare_batch(next(iter(trainer.train_loader_sensor_b)), 'train')
    losses = trainer.train_step(batch)[0]
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    os.remove(s.text_embeddings_path)
