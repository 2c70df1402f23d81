"""Class names -> the fp32 [K, 512] text embeddings file that `text_embeddings_path` reads (K29): CLIP's text tower in fp32 on the
GPU (openess_amd/models/clip_text.py), OpenAI's BPE (openess_amd/models/clip_tokenizer.py), CLIP's prompt ensemble.

    python tools/write_text_embeddings.py --checkpoint ViT-B-16.pt --bpe bpe_simple_vocab_16e6.txt.gz \\
        --classes background,building,fence,person,pole,road,sidewalk,vegetation,car,wall,traffic\\ sign --out text_embeddings.pt
    python tools/write_text_embeddings.py ... --classes classes.txt --templates templates.txt --out text_embeddings.pt

--classes: a comma list, or a file with one class per line; `a|b|c` names synonyms pooled into one class.
--templates: `single` ('a photo of a {}.', the default), `none` (the bare name) or a file with one template containing {} per
line (CLIP's 80 and MaskCLIP's 85 are not shipped).  The checkpoint is a state dict of OpenAI CLIP (whole or its text keys, or
the TorchScript archive) or of HuggingFace's CLIPTextModelWithProjection."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_classes(spec):
    from openess_amd.models.clip_text import parse_classes as parse
    return parse(spec)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--checkpoint', required=True)
    ap.add_argument('--bpe', required=True)
    ap.add_argument('--classes', required=True)
    ap.add_argument('--templates', default='single')
    ap.add_argument('--out', required=True)
    a = ap.parse_args(argv)
    from openess_amd.models.clip_text import compute_text_embeddings
    if not torch.cuda.is_available():
        raise SystemExit("write_text_embeddings.py needs the GPU (the text tower has no CPU path)")
    classes = parse_classes(a.classes)
    emb = compute_text_embeddings(a.checkpoint, a.bpe, classes, a.templates, 'cuda')
    torch.save(emb, a.out)
    print(f"{a.out}: {tuple(emb.shape)} fp32, {len(classes)} classes")
    return emb


if __name__ == "__main__":
    main()
