#!/usr/bin/env python3
"""Fixture generator (build container only; imports the REAL reference): cp_{llama,qwen2,qwen3}.npz = CP-LRP explanations of
`lxt.efficient.monkey_patch(modeling module, patch_map=cp_LRP)` (lxt/efficient/models/llama.py, qwen2.py, qwen3.py) run on the CPU in fp64
with eager attention, by the user protocol `logits[0, p, tgt].backward(); (e * e.grad).sum(-1)`.

Models: hf_models.build_llama(), qwen_models.build("qwen2_d64") (randomised q / k / v biases) and qwen_models.build("qwen3_d128")
(randomised head-norm weights) -- the models of generate_*.npz; a checksum of the weights is stored with each.
Batch: ids = torch.randint(0, V, (3, 24)) from the generator seed of make_golden_generate.CASES, lengths (24, 15, 7) = the LAST n columns of
a row (the engine's left-padded layout).  Each prompt is explained alone and un-padded (RoPE is relative); its rows are placed at the
prompt's own columns, pads are 0.  The explained logit is the arg-max of the last position.
Stored: ids [3, 24], lengths [3], idx [3], logit [3], R_tok [3, 24], layer_R [L + 1, 3] = sum (h * h.grad) at the embedding (index 0) and at
every decoder layer's output.
Span case (key prefix `span_logit/`, `span_logprob/`): prompt 0, the T = 4 positions POS with weights W, targets = the next token (the row's
arg-max at column S - 1), f = sum_t w_t logits[0, p_t, tgt_t] or the same over log_softmax: positions, weights, target, logit, logprob [1, 4],
R_tok [1, 24], layer_R [L + 1, 1].
err32: the reference's own fp32 run of the batch against its fp64 run, normalised max error of R_tok -- the floor an fp32 engine is
measured above.  The fp32 run is made BEFORE the fp64 switch of make_golden_span.all_fp64 (which would lift the fp32 model's RMSNorm and
softmax to fp64)."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")

S = 24
LENGTHS = (24, 15, 7)
POS = (3, 11, 18, S - 1)
W = (1.0, 0.5, -1.0, 2.0)
PROTOCOL = ("lxt.efficient.monkey_patch(modeling module, patch_map=cp_LRP), CPU, eager attention; f = logits[0, -1, argmax] (batch) or "
            "sum_t w_t logits[0, p_t, tgt_t] / sum_t w_t log_softmax(logits[0, p_t])[tgt_t] (span); f.backward(); hooks on decoder-layer "
            "outputs and the input embedding; padded prompts run un-padded")


def batch(model, ids):
    """ids [3, S] -> the stored arrays of the padded batch, each prompt explained alone"""
    from tests.golden.make_golden_span import explain
    per = [explain(model, ids[b, S - n:], [n - 1], [None], [1.0], "logit") for b, n in enumerate(LENGTHS)]
    R_tok = torch.zeros(len(LENGTHS), S, dtype=torch.float64)
    for b, (n, r) in enumerate(zip(LENGTHS, per)):
        R_tok[b, S - n:] = r["R_tok"].double()
    return dict(idx=np.asarray([r["target"][0] for r in per]), logit=np.asarray([r["logit"][0] for r in per]), R_tok=R_tok.numpy(),
                layer_R=torch.stack([r["layer_R"].double() for r in per], 1).numpy())


def span(model, ids, objective):
    from tests.golden.make_golden_span import explain
    r = explain(model, ids[0], list(POS), [None] * len(POS), list(W), objective)
    return dict(positions=np.asarray([POS]), weights=np.asarray([W]), target=np.asarray([r["target"]]), logit=np.asarray([r["logit"]]),
                logprob=np.asarray([r["logprob"]]), R_tok=r["R_tok"].double().numpy()[None], layer_R=r["layer_R"].double().numpy()[:, None])


def nmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def main(reference=os.environ.get("LXT_REFERENCE", "")):
    if reference:
        sys.path.insert(0, reference)
    from lxt.efficient import monkey_patch
    from lxt.efficient.models import llama, qwen2, qwen3
    from transformers.models.llama import modeling_llama
    from transformers.models.qwen2 import modeling_qwen2
    from transformers.models.qwen3 import modeling_qwen3
    from tests.golden.hf_models import wsum
    from tests.golden.make_golden_generate import build, prompts
    from tests.golden.make_golden_span import all_fp64
    for mod, maps in ((modeling_llama, llama), (modeling_qwen2, qwen2), (modeling_qwen3, qwen3)):
        monkey_patch(mod, patch_map=maps.cp_LRP)
    models = {name: build(name) for name in ("llama", "qwen2", "qwen3")}
    ids = {name: prompts(name, m.config.vocab_size) for name, m in models.items()}
    fp32 = {name: batch(m, ids[name]) for name, m in models.items()}
    all_fp64()
    for name, model in models.items():
        ws = wsum(model)
        model = model.double()
        out = batch(model, ids[name])
        err32 = nmax(fp32[name]["R_tok"], out["R_tok"])
        assert (fp32[name]["idx"] == out["idx"]).all()
        for objective in ("logit", "logprob"):
            out.update({f"span_{objective}/{k}": v for k, v in span(model, ids[name], objective).items()})
        print(f"[{name}] idx {out['idx'].tolist()} logit {out['logit'].round(4).tolist()} sum R_tok {out['R_tok'].sum(1).round(5).tolist()} "
              f"layer_R[L] {out['layer_R'][-1].round(5).tolist()}; reference fp32 vs fp64 R_tok {err32:.2e}")
        np.savez_compressed(os.path.join(HERE, f"cp_{name}.npz"), ids=ids[name].numpy(), lengths=np.asarray(LENGTHS), wsum=ws, err32=err32,
                            protocol=np.array(PROTOCOL), **out)


if __name__ == "__main__":
    main(*sys.argv[1:2])
