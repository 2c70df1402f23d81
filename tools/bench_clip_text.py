"""Time CLIP's text tower (K29) at the real geometry: 11 classes x 85 prompts = 935 texts of 77 tokens, width 512, 8 heads, 12
blocks, vocabulary 49408, seeded random weights.  Per part and for the whole encode_classes, in interleaved rounds (every round
times every part once, so drift of the clock hits all of them alike); medians in ms.

    python tools/bench_clip_text.py [--rounds 7] [--chunk 256]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--chunk', type=int, default=256)
    a = ap.parse_args()
    from openess_amd import hip
    from openess_amd.models.clip_text import CLIPTextEncoder
    dev = 'cuda'
    torch.manual_seed(0)
    m = CLIPTextEncoder().to(dev)
    K, P, L, C, H = 11, 85, 77, 512, 8
    N = K * P
    ids = torch.zeros(N, L, dtype=torch.int64)
    for n in range(N):
        k = 4 + n % 12
        ids[n, 0], ids[n, 1:1 + k], ids[n, 1 + k] = 49406, torch.randint(1, 49406, (k,)), 49407
    ids = ids.to(dev)
    off = torch.arange(0, N + 1, P, dtype=torch.int64)
    n = min(a.chunk, N)
    x = hip.clip_text_embed(ids[:n], m.token_embedding.weight, m.positional_embedding)
    blk = m.transformer.resblocks[0]
    qkv = torch.randn(n * L, 3 * C, device=dev)
    e = torch.randn(N, 512, device=dev)
    parts = {
        'embed': lambda: hip.clip_text_embed(ids[:n], m.token_embedding.weight, m.positional_embedding),
        'attention_causal': lambda: hip.attention_d64_f32(qkv, n, L, H, causal=True),
        'attention_full': lambda: hip.attention_d64_f32(qkv, n, L, H),
        'block': lambda: blk.forward_fp32(x, n, L),
        'eot_norm': lambda: hip.clip_text_eot_norm(x, ids[:n], m.ln_final.weight, m.ln_final.bias, 1e-5),
        'prompt_mean': lambda: hip.prompt_mean_normalize(e, off),
        'encode_classes': lambda: m.encode_classes(ids, off, chunk=a.chunk),
    }
    for f in parts.values():                               # warm-up: packs the weights, loads the code objects
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in parts}
    for _ in range(a.rounds):
        for k, f in parts.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1))
    out = {k: round(statistics.median(v), 4) for k, v in times.items()}
    out.update(texts=N, chunk=n, rounds=a.rounds, spread={k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
