#!/usr/bin/env python3
"""Fixture generator: generate_gemma3.npz = greedy continuations of a tiny Gemma-3 text decoder by HuggingFace `transformers` alone, on the
CPU in fp64 with eager attention and no cache -- the protocol of make_golden_generate.py (each prompt alone and un-padded, every step a
full forward of the sequence so far; lengths (24, 15, 7) of S = 24, 24 new tokens; greedy / B / S / NEW / LENGTHS are that module's).

Model: hf_models.build_gemma3() (4 layers, three sliding with a window of 32 and one global, head dim 32) with seeded non-trivial (1 + w)
norm weights, as build_gemma3_4bdims gives its model (HF initialises them to zero, which would leave the four layer norms and the head
norms of the decode step untested); a checksum of the weights is stored.  The two longer prompts grow past the window (24 + 24 and
15 + 24 tokens against 32), so the sliding layers' first live key moves during generation.
Prompt seed 7: seed 1234 of the other generators leaves a smallest top-1 - top-2 margin of 1.6e-4, under the 2e-4 this protocol asks
for; seed 7 leaves 1.1e-3 and 49 distinct tokens over the three continuations (none collapses).
Stored and asserted: as make_golden_generate.py (margin >= 2e-4; HF in fp32 reproduces the fp64 tokens)."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")

PROMPT_SEED = 7
NORM_SEED = 41


def build():
    from tests.golden import hf_models
    m = hf_models.build_gemma3()
    with torch.no_grad():
        g = torch.Generator().manual_seed(NORM_SEED)
        for n_, p_ in m.named_parameters():
            if "norm" in n_:
                p_.copy_(torch.randn(p_.shape, generator=g) * 0.1)
    for p_ in m.parameters():
        p_.requires_grad_(False)
    return m


def prompts(vocab):
    from tests.golden import make_golden_generate as gg
    return torch.randint(0, vocab, (gg.B, gg.S), generator=torch.Generator().manual_seed(PROMPT_SEED))


def main():
    from tests.golden import make_golden_generate as gg
    from tests.golden.hf_models import wsum
    model = build()
    ids, ws = prompts(model.config.vocab_size), wsum(model)
    t32, l32 = zip(*(gg.greedy(model, ids[b, gg.S - n:], gg.NEW) for b, n in enumerate(gg.LENGTHS)))
    model = model.double()
    t64, l64 = zip(*(gg.greedy(model, ids[b, gg.S - n:], gg.NEW) for b, n in enumerate(gg.LENGTHS)))
    tokens, logits = np.stack(t64), np.stack(l64)
    top2 = np.sort(logits, -1)[..., -2:]
    margin = float((top2[..., 1] - top2[..., 0]).min())
    diff = float(np.abs(np.stack(l32) - logits).max() / np.abs(logits).max())
    print(f"[gemma3] margin {margin:.3e}  distinct tokens {len(set(tokens.ravel().tolist()))}  fp32 vs fp64 logits {diff:.1e} (max-normalised)")
    assert margin >= gg.MIN_MARGIN, margin
    assert (np.stack(t32) == tokens).all(), "HF fp32 does not reproduce the fp64 tokens"
    np.savez_compressed(os.path.join(HERE, "generate_gemma3.npz"), ids=ids.numpy(), lengths=np.asarray(gg.LENGTHS), tokens=tokens, logits=logits,
                        wsum=ws, margin=margin, window=model.config.sliding_window, protocol=np.array(gg.PROTOCOL))


if __name__ == "__main__":
    main()
