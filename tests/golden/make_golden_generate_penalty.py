#!/usr/bin/env python3
"""Fixture generator: generate_penalty_{llama,qwen3,gemma3}.npz = greedy continuations under repetition_penalty = 1.3 by HuggingFace
`transformers` alone, on the CPU in fp64 with eager attention and no cache -- the protocol of make_golden_generate.py (each prompt alone and
un-padded, every step a full forward of the sequence so far; lengths (24, 15, 7) of S = 24), with HF's own
RepetitionPenaltyLogitsProcessor(1.3) applied to the last row's logits over the whole sequence so far (prompt + generated) before the
arg-max.  12 new tokens.

Models: those of generate_{llama,qwen3}.npz (make_golden_generate.build) and of generate_gemma3.npz (make_golden_generate_gemma3.build); a
checksum of the weights is stored.  Prompts: torch.randint(0, V, (3, 24)) from generator seeds 5 / 1 / 3 -- the first seed from 1 upwards at
which every prompt's continuation differs from the un-penalised one and every step's processed top-2 margin is at least 2e-3 (the seeds of
the un-penalised fixtures leave 4e-4 on the Llama case).  The ids are random over all S columns, so the columns in front of a shorter
prompt hold real token ids: an engine that counted its left pads as history would penalise them.
Stored: ids [3, 24], lengths [3], tokens [3, 12], logits [3, 12, V] (the RAW last-row logits of every step, fp64), wsum, margin = the smallest
top-1 - top-2 difference of the PROCESSED logits over all steps and prompts, plain = the un-penalised greedy tokens of the same prompts.
Asserted here: every prompt's continuation differs from its un-penalised greedy one, and margin >= 1e-3 (an fp32 engine within the
project's 1e-4 bar of these logits cannot flip an arg-max that is decided by more)."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")

NEW = 12
RP = 1.3
MIN_MARGIN = 1e-3
CASES = dict(llama=5, qwen3=1, gemma3=3)          # prompt seeds
PROTOCOL = ("transformers, CPU, fp64, eager attention, use_cache=False; RepetitionPenaltyLogitsProcessor(1.3) over the sequence so far, then the "
            "arg-max of logits[0, -1] per step; each prompt alone, un-padded")


def build(name):
    from tests.golden import make_golden_generate as gg
    from tests.golden import make_golden_generate_gemma3 as g3
    model = g3.build() if name == "gemma3" else gg.build(name)
    for p in model.parameters():
        p.requires_grad_(False)
    return model, torch.randint(0, model.config.vocab_size, (gg.B, gg.S), generator=torch.Generator().manual_seed(CASES[name]))


@torch.no_grad()
def penalised(model, ids, n_new, rp):
    """ids [n] -> (tokens [n_new], raw logits [n_new, V], the smallest top-2 margin of the processed logits)"""
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    proc = RepetitionPenaltyLogitsProcessor(rp) if rp != 1.0 else (lambda seq, row: row)
    seq, toks, rows, margin = ids[None].clone(), [], [], float("inf")
    for _ in range(n_new):
        row = model(input_ids=seq, use_cache=False).logits[0, -1]
        scores = proc(seq, row[None].clone())[0]
        top2 = torch.topk(scores, 2).values
        margin = min(margin, float(top2[0] - top2[1]))
        toks.append(int(scores.argmax()))
        rows.append(row)
        seq = torch.cat([seq, torch.tensor([[toks[-1]]])], 1)
    return np.asarray(toks), torch.stack(rows).double().numpy(), margin


def run(name):
    from tests.golden import make_golden_generate as gg
    from tests.golden.hf_models import wsum
    model, ids = build(name)
    ws = wsum(model)
    model = model.double()
    S = gg.S
    tok, logits, margins = zip(*(penalised(model, ids[b, S - n:], NEW, RP) for b, n in enumerate(gg.LENGTHS)))
    plain = np.stack([penalised(model, ids[b, S - n:], NEW, 1.0)[0] for b, n in enumerate(gg.LENGTHS)])
    tokens, margin = np.stack(tok), min(margins)
    changed = [int((tokens[b] != plain[b]).sum()) for b in range(len(gg.LENGTHS))]
    print(f"[{name}] processed margin {margin:.3e}  tokens that differ from the un-penalised greedy run, per prompt: {changed}")
    assert all(changed), "a continuation equals the un-penalised one"
    assert margin >= MIN_MARGIN, margin
    np.savez_compressed(os.path.join(HERE, f"generate_penalty_{name}.npz"), ids=ids.numpy(), lengths=np.asarray(gg.LENGTHS), tokens=tokens,
                        logits=np.stack(logits), plain=plain, wsum=ws, margin=margin, repetition_penalty=RP, protocol=np.array(PROTOCOL))


if __name__ == "__main__":
    for case in sys.argv[1:] or CASES:
        run(case)
