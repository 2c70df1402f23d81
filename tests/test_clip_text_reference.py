"""The float64 restatement of CLIP's text encoder (tests/clip_text_reference.py, the oracle of tests/test_hip_clip_text.py) against
HuggingFace's CLIPTextModelWithProjection in float64 on a tiny configuration built offline, through convert_hf_state_dict (so
the key mapping, the q/k/v concatenation and the transposed projection are held too).  No GPU."""
import pytest
import torch

transformers = pytest.importorskip('transformers')

from tests import clip_text_reference as cr  # noqa: E402

TOL = 1e-12


@pytest.fixture(scope="module")
def hf():
    cfg = transformers.CLIPTextConfig(vocab_size=64, hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=512,
                                      projection_dim=96, max_position_embeddings=16, hidden_act='quick_gelu', eos_token_id=2,
                                      bos_token_id=1, pad_token_id=0)
    torch.manual_seed(11)
    m = transformers.CLIPTextModelWithProjection(cfg).double().eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('bias'):
                p.normal_(0, 0.1)
            elif 'layer_norm' in n:
                p.uniform_(0.7, 1.3)
            else:
                p.mul_(8.0)                               # the initialisation's 0.02 leaves the attention nearly uniform
    return m


def _ids():
    g = cr._gen("hf_ids")
    ids = torch.randint(0, 62, (7, 16), generator=g)
    eot = torch.tensor([1, 15, 4, 9, 12, 2, 7])
    ids[torch.arange(7), eot] = 63
    ids[3, 12] = 63                                        # a second maximum behind the first
    return ids, eot


def test_restatement_equals_huggingface_in_float64(hf):
    from openess_amd.models.clip_text import convert_hf_state_dict
    sd = convert_hf_state_dict(hf.state_dict())
    ids, eot = _ids()
    with torch.no_grad():
        out = hf(input_ids=ids, output_hidden_states=True)
    got = cr.text_encode64(sd, ids, heads=2)
    assert got.shape == (7, 96)
    assert float((got - out.text_embeds).abs().max()) <= TOL
    hidden = cr.text_hidden64(sd, ids, heads=2)
    last = out.hidden_states[-1]
    for n in range(7):                                     # up to each end-of-text token (HF's padding mask is not CLIP's)
        assert float((hidden[n, :eot[n] + 1] - last[n, :eot[n] + 1]).abs().max()) <= TOL


def test_huggingface_is_causal_and_pools_at_the_argmax(hf):
    ids, eot = _ids()
    other = ids.clone()
    for n in range(7):
        other[n, eot[n] + 1:] = torch.randint(0, 62, (15 - int(eot[n]),), generator=cr._gen("hf_tail", n))
    with torch.no_grad():
        a, b = hf(input_ids=ids).text_embeds, hf(input_ids=other).text_embeds
    assert float((a - b).abs().max()) <= TOL and not torch.equal(ids, other)


def test_fp32_restatement_is_the_float64_one_rounded(hf):
    """text_encode32 (the figures' fp32 side) follows the same definition"""
    from openess_amd.models.clip_text import convert_hf_state_dict
    sd = convert_hf_state_dict(hf.state_dict())
    ids, _ = _ids()
    assert cr.rel_max(cr.text_encode32(sd, ids, 2), cr.text_encode64(sd, ids, 2)) <= 1e-5
