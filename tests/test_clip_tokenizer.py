"""OpenAI's byte-level BPE in plain Python (openess_amd/models/clip_tokenizer.py) on a synthetic merges file
(tests/clip_text_reference.py: five merges that build `road</w>` and `car</w>`): hand-worked ids, the cleaning, both file forms,
overflow, and transformers.CLIPTokenizer where it is importable.  No GPU."""
import json

import pytest
import torch

from tests import clip_text_reference as cr

SOT, EOT = cr.SYNTH_SOT, cr.SYNTH_EOT


def _sym(ch, end=False):
    """id of a printable ASCII byte symbol, with </w> when it ends a word"""
    return ord(ch) - 33 + (256 if end else 0)


@pytest.fixture()
def tok(tmp_path):
    from openess_amd.models.clip_tokenizer import CLIPTokenizer
    return CLIPTokenizer(cr.write_merges(tmp_path / "merges.txt"))


def test_hand_worked_ids(tok):
    assert tok.vocab_size == cr.SYNTH_VOCAB and (tok.sot_id, tok.eot_id) == (SOT, EOT) and EOT == tok.vocab_size - 1
    assert tok.encode("road") == [514]                                          # r o a d</w> -> ro a d</w> -> ro ad</w> -> road</w>
    assert tok.encode("car") == [516]
    assert tok.encode("a car") == [_sym("a", True), 516]
    assert tok.encode("cab") == [515, _sym("b", True)]                          # ca b</w>
    assert tok.encode("roads") == [512, _sym("a"), _sym("d"), _sym("s", True)]  # ad</w> needs the word to end in d
    assert tok.encode("car.") == [516, _sym(".", True)]
    assert tok.encode("it's 42") == [_sym("i"), _sym("t", True), _sym("'"), _sym("s", True), _sym("4", True), _sym("2", True)]
    assert tok.encode("") == []
    ids = tok.tokenize(["road", "a car"], context_length=6)
    assert ids.dtype == torch.int64 and ids.tolist() == [[SOT, 514, EOT, 0, 0, 0], [SOT, _sym("a", True), 516, EOT, 0, 0]]
    assert tok.tokenize("road", context_length=4).tolist() == [[SOT, 514, EOT, 0]]
    assert bool((ids.argmax(dim=1) == torch.tensor([2, 3])).all())             # the pooling position
    assert tok.decode([514, 516]) == "road car "


def test_case_whitespace_and_html_folding(tok):
    want = tok.encode("a road")
    for text in ("A ROAD", "  a \t road\n", "a&#32;road", "a &amp;#32; road", "A Road"):
        assert tok.encode(text) == want, text
    assert tok.encode("café") == [515, _sym("f")] + [tok.encoder[tok.byte_encoder[0xc3]], tok.encoder[tok.byte_encoder[0xa9] + "</w>"]]


def test_gz_and_plain_and_headerless_files_agree(tmp_path):
    from openess_amd.models.clip_tokenizer import CLIPTokenizer
    texts = ["a photo of a road.", "car on the road", "broad"]
    toks = [CLIPTokenizer(cr.write_merges(tmp_path / "m.txt")), CLIPTokenizer(cr.write_merges(tmp_path / "m.txt.gz", gz=True)),
            CLIPTokenizer(cr.write_merges(tmp_path / "bare.txt", header=False))]
    first = toks[0].tokenize(texts)
    assert first.shape == (3, 77)
    for t in toks[1:]:
        assert torch.equal(t.tokenize(texts), first)
    (tmp_path / "bad.txt").write_text("#version: 0.2\na b c\n")
    with pytest.raises(ValueError, match="two symbols per line"):
        CLIPTokenizer(str(tmp_path / "bad.txt"))


def test_overflow_raises_and_truncation_keeps_the_end_token_last(tok):
    text = "road " * 10
    assert tok.tokenize(text, context_length=12).tolist() == [[SOT] + [514] * 10 + [EOT]]
    with pytest.raises(ValueError, match="context holds 11"):
        tok.tokenize(text, context_length=11)
    cut = tok.tokenize(["car", text], context_length=8, truncate=True)
    assert cut.tolist() == [[SOT, 516, EOT, 0, 0, 0, 0, 0], [SOT] + [514] * 6 + [EOT]]


def test_equals_transformers_clip_tokenizer_up_to_the_first_end_token(tok, tmp_path):
    transformers = pytest.importorskip("transformers")
    import inspect
    if "vocab" in inspect.signature(transformers.CLIPTokenizer.__init__).parameters:        # transformers 5: the tables themselves
        hf = transformers.CLIPTokenizer(vocab=dict(tok.encoder), merges=[tuple(m) for m in cr.SYNTH_MERGES])
    else:                                                                                    # transformers 4: the two files
        (tmp_path / "vocab.json").write_text(json.dumps(tok.encoder))
        hf = transformers.CLIPTokenizer(vocab_file=str(tmp_path / "vocab.json"), merges_file=cr.write_merges(tmp_path / "hf_merges.txt"))
    texts = ["road", "a photo of a car.", "A  Broad ROAD, it's 42 cabs!", "café road"]
    ours = tok.tokenize(texts, context_length=40)
    theirs = hf(texts, padding="max_length", max_length=40)["input_ids"]
    for a, b in zip(ours.tolist(), theirs):
        n = a.index(EOT) + 1
        assert a[:n] == b[:n] and b[0] == SOT
