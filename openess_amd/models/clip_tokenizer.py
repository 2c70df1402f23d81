"""OpenAI CLIP's byte-level BPE tokenizer in plain Python (K29), for the text tower of models/clip_text.py.

The merges come from a file the user names: OpenAI's `bpe_simple_vocab_16e6.txt.gz`, or a `merges.txt` (plain or gzipped, as
HuggingFace ships it).  The first line is a header when it starts with `#version` (both files have one; the OpenAI file's is
`"bpe_simple_vocab_16e6.txt#version: 0.2`) and at most 49152 - 256 - 2 merges are used, like OpenAI's loader.  The vocabulary is
the 256 byte symbols, the same with `</w>`, one entry per merge, then <|startoftext|> and <|endoftext|>: the end-of-text token
has the largest id, which is what the tower's pooling (argmax of the ids) relies on.

A text is cleaned as OpenAI's `clip.tokenize` does: `ftfy.fix_text` WHEN ftfy IS IMPORTABLE (it is an optional package; without
it that step is skipped, which differs only on text with broken Unicode), html.unescape twice, whitespace collapsed, lower-cased;
then split by CLIP's pattern with the `regex` package (with the standard `re` and the nearest classes when `regex` is missing:
[^\\W\\d_] for \\p{L}, \\d for \\p{N})."""
import functools
import gzip
import html

import torch

try:
    import regex as _re
    _PATTERN = r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+"""
except ImportError:                                      # pragma: no cover
    import re as _re
    _PATTERN = r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[^\W\d_]+|\d|(?:[^\s\w]|_)+"""

try:
    import ftfy as _ftfy
except ImportError:
    _ftfy = None

MAX_MERGES = 49152 - 256 - 2
SOT, EOT = '<|startoftext|>', '<|endoftext|>'


@functools.lru_cache()
def bytes_to_unicode():
    """byte -> a printable unicode character (GPT-2's table): BPE then works on strings without whitespace or control bytes"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


def read_merges(path):
    with open(path, 'rb') as f:
        raw = f.read()
    if raw[:2] == b'\x1f\x8b':
        raw = gzip.decompress(raw)
    lines = raw.decode('utf-8').split('\n')
    if lines and '#version' in lines[0]:
        lines = lines[1:]
    merges = [tuple(ln.split()) for ln in lines[:MAX_MERGES] if ln.strip()]
    if not merges or any(len(m) != 2 for m in merges):
        raise ValueError(f"{path}: a merges file has two symbols per line")
    return merges


def clean_text(text):
    if _ftfy is not None:
        text = _ftfy.fix_text(text)
    text = html.unescape(html.unescape(text))
    return ' '.join(text.split()).strip().lower()


class CLIPTokenizer:
    def __init__(self, bpe_path):
        merges = read_merges(bpe_path)
        self.byte_encoder = bytes_to_unicode()
        vocab = list(self.byte_encoder.values())
        vocab = vocab + [v + '</w>' for v in vocab] + [''.join(m) for m in merges] + [SOT, EOT]
        self.encoder = dict(zip(vocab, range(len(vocab))))
        self.decoder = {v: k for k, v in self.encoder.items()}
        self.bpe_ranks = dict(zip(merges, range(len(merges))))
        self.cache = {SOT: SOT, EOT: EOT}
        self.pat = _re.compile(_PATTERN, _re.IGNORECASE)
        self.sot_id, self.eot_id = self.encoder[SOT], self.encoder[EOT]

    @property
    def vocab_size(self):
        return len(self.encoder)

    def bpe(self, token):
        if token in self.cache:
            return self.cache[token]
        word = tuple(token[:-1]) + (token[-1] + '</w>',)
        while len(word) > 1:
            pairs = set(zip(word[:-1], word[1:]))
            best = min(pairs, key=lambda p: self.bpe_ranks.get(p, float('inf')))
            if best not in self.bpe_ranks:
                break
            first, second = best
            new, i = [], 0
            while i < len(word):
                if i + 1 < len(word) and word[i] == first and word[i + 1] == second:
                    new.append(first + second)
                    i += 2
                else:
                    new.append(word[i])
                    i += 1
            word = tuple(new)
        out = ' '.join(word)
        self.cache[token] = out
        return out

    def encode(self, text):
        ids = []
        for token in self.pat.findall(clean_text(text)):
            token = ''.join(self.byte_encoder[b] for b in token.encode('utf-8'))
            ids.extend(self.encoder[t] for t in self.bpe(token).split(' '))
        return ids

    def decode(self, ids):
        byte_decoder = {v: k for k, v in self.byte_encoder.items()}
        text = ''.join(self.decoder[int(i)] for i in ids)
        return bytearray(byte_decoder[c] for c in text).decode('utf-8', errors='replace').replace('</w>', ' ')

    def tokenize(self, texts, context_length=77, truncate=False):
        """str or list of str -> int64 [N, context_length]: SOT, tokens, EOT, zeros.  A text that does not fit raises ValueError
        unless truncate=True, which cuts the tokens and keeps EOT last."""
        if isinstance(texts, str):
            texts = [texts]
        out = torch.zeros(len(texts), context_length, dtype=torch.int64)
        for i, text in enumerate(texts):
            ids = [self.sot_id] + self.encode(text) + [self.eot_id]
            if len(ids) > context_length:
                if not truncate:
                    raise ValueError(f"text {text!r} has {len(ids)} tokens, the context holds {context_length}")
                ids = ids[:context_length]
                ids[-1] = self.eot_id
            out[i, :len(ids)] = torch.tensor(ids, dtype=torch.int64)
        return out
