#!/usr/bin/env python3
"""Fixture generator: generate_{llama,qwen2,qwen3}.npz = greedy continuations by HuggingFace `transformers` alone, on the CPU in fp64 with
eager attention and no cache (every step is a full forward of the sequence so far; the reference changes only the backward, so its forward
is HF's).

Models: hf_models.build_llama(), qwen_models.build("qwen2_d64") (randomised q / k / v biases) and qwen_models.build("qwen3_d128")
(randomised head-norm weights); a checksum of the weights is stored with each.
Prompts: torch.randint(0, V, (3, 24)) from generator seed 1234 (seed 6 for the Qwen2 case: the other seeds tried collapse to 2-3 repeated
tokens), lengths (24, 15, 7) = the LAST n columns of a row (the engine's left-padded layout), 24 new tokens.  Each prompt is generated
alone and un-padded: that is what the engine's padded batch must equal, and a left-padded fp64 batch through this transformers version
returns NaN logits for the padded prompts.
Stored: ids [3, 24], lengths [3], tokens [3, 24], logits [3, 24, V] (the last row's logits of every step, fp64), wsum, margin = the smallest
top-1 - top-2 logit difference over all steps and prompts.
Asserted here: margin >= 2e-4 (an fp32 engine within the project's 1e-4 bar of these logits cannot flip an arg-max that is decided by
more), and HF in fp32 reproduces the fp64 tokens."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")

B, S, NEW = 3, 24, 24
LENGTHS = (24, 15, 7)
MIN_MARGIN = 2e-4
CASES = dict(llama=1234, qwen2=6, qwen3=1234)          # prompt seeds
PROTOCOL = "transformers, CPU, eager attention, use_cache=False; greedy arg-max of logits[0, -1] per step; each prompt alone, un-padded"


def build(name):
    from tests.golden import hf_models, qwen_models
    if name == "llama":
        return hf_models.build_llama()
    return qwen_models.build(dict(qwen2="qwen2_d64", qwen3="qwen3_d128")[name])


def prompts(name, vocab):
    return torch.randint(0, vocab, (B, S), generator=torch.Generator().manual_seed(CASES[name]))


@torch.no_grad()
def greedy(model, ids, n_new):
    """ids [n] -> (tokens [n_new], logits [n_new, V]) in the model's dtype"""
    seq, toks, rows = ids[None].clone(), [], []
    for _ in range(n_new):
        row = model(input_ids=seq, use_cache=False).logits[0, -1]
        toks.append(int(row.argmax()))
        rows.append(row)
        seq = torch.cat([seq, torch.tensor([[toks[-1]]])], 1)
    return np.asarray(toks), torch.stack(rows).double().numpy()


def run(name):
    from tests.golden.hf_models import wsum
    model = build(name)
    for p in model.parameters():
        p.requires_grad_(False)
    vocab = model.config.vocab_size
    ids = prompts(name, vocab)
    ws = wsum(model)
    t32, l32 = zip(*(greedy(model, ids[b, S - n:], NEW) for b, n in enumerate(LENGTHS)))
    model = model.double()
    t64, l64 = zip(*(greedy(model, ids[b, S - n:], NEW) for b, n in enumerate(LENGTHS)))
    tokens, logits = np.stack(t64), np.stack(l64)
    top2 = np.sort(logits, -1)[..., -2:]
    margin = float((top2[..., 1] - top2[..., 0]).min())
    diff = float(np.abs(np.stack(l32) - logits).max() / np.abs(logits).max())
    print(f"[{name}] margin {margin:.3e}  distinct tokens {len(set(tokens.ravel().tolist()))}  fp32 vs fp64 logits {diff:.1e} (max-normalised)")
    assert margin >= MIN_MARGIN, margin
    assert (np.stack(t32) == tokens).all(), "HF fp32 does not reproduce the fp64 tokens"
    np.savez_compressed(os.path.join(HERE, f"generate_{name}.npz"), ids=ids.numpy(), lengths=np.asarray(LENGTHS), tokens=tokens, logits=logits,
                        wsum=ws, margin=margin, protocol=np.array(PROTOCOL))


if __name__ == "__main__":
    for case in sys.argv[1:] or CASES:
        run(case)
