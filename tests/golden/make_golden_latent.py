#!/usr/bin/env python3
"""Fixture generator (build container only; imports the REAL reference): latent_llama.npz = the latent feature attribution of the
reference's docs (docs/source/latent-feature-attribution-efficient.rst, README "Latent Feature Attribution") on a seeded Llama at the
llama_mid dimensions, `lxt.efficient.monkey_patch(modeling_llama)` (ref lxt/efficient/models/llama.py:9-14) run on the CPU in fp64.

Protocol (the doc's): forward hooks + retain_grad on every decoder layer's output and on the input embedding, a forward pre-hook + retain_grad
on every mlp.down_proj input, the arg-max logit of the last position seeded with 1.  Frozen:
  ids [S], idx, logit;
  trace [L+1, S]  = (h * h.grad).sum(-1) at the embedding (index 0) and at every decoder layer's output (index l = layer l - 1);
  resid [L+1, H]  = (h * h.grad).sum(0) at the same boundaries (token-summed residual-stream relevance);
  mlp   [L, I]    = (m * m.grad).sum(0) at every down_proj input (token-summed MLP-neuron relevance, HF column order).
Weights: oracle.llama.random_weights(cfg, seed=wseed) (tests.util checks them against wsum)."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")

CFG = dict(hidden=256, inter=512, n_layers=4, n_heads=8, n_kv=2, head_dim=32, vocab=512, rope_theta=500000.0, rms_eps=1e-5)
S, WSEED, ISEED = 128, 2, 12


def wsum(W):
    tot = float(W["embed"].double().abs().sum() + W["lm_head"].double().abs().sum())
    for L in W["layers"]:
        tot += sum(float(v.double().abs().sum()) for v in L.values())
    return tot


def main(reference=os.environ.get("LXT_REFERENCE", "")):
    if reference:
        sys.path.insert(0, reference)
    from lxt.efficient import monkey_patch
    from transformers.models.llama import modeling_llama
    from oracle import llama as ol
    from tests.golden.hf_models import build_llama_from_weights
    monkey_patch(modeling_llama)
    W = ol.random_weights(CFG, seed=WSEED)
    ids = torch.randint(0, CFG["vocab"], (S,), generator=torch.Generator().manual_seed(ISEED))
    model = build_llama_from_weights(CFG, W, attn="eager", dtype=torch.float64)

    outs, mids = [], []

    def keep_out(mod, args, out):
        h = out[0] if isinstance(out, tuple) else out
        h.retain_grad()
        outs.append(h)

    def keep_in(mod, args):
        args[0].retain_grad()
        mids.append(args[0])

    hooks = [L.register_forward_hook(keep_out) for L in model.model.layers]
    hooks += [L.mlp.down_proj.register_forward_pre_hook(keep_in) for L in model.model.layers]
    e = model.get_input_embeddings()(ids[None]).detach().requires_grad_()
    last = model(inputs_embeds=e, use_cache=False).logits[0, -1]
    idx = int(last.argmax())
    last[idx].backward()
    for h in hooks:
        h.remove()
    hs = [e] + outs
    trace = torch.stack([(h * h.grad)[0].sum(-1) for h in hs]).detach()
    resid = torch.stack([(h * h.grad)[0].sum(0) for h in hs]).detach()
    mlp = torch.stack([(m * m.grad)[0].sum(0) for m in mids]).detach()
    assert trace.shape == (CFG["n_layers"] + 1, S) and mlp.shape == (CFG["n_layers"], CFG["inter"])
    print(f"idx {idx} logit {float(last[idx]):+.6f}  sum trace[0] {float(trace[0].sum()):+.6f}  "
          f"|resid sums - trace sums| {float((resid.sum(-1) - trace.sum(-1)).abs().max()):.1e}  max|mlp| {float(mlp.abs().max()):.3e}")
    np.savez_compressed(os.path.join(HERE, "latent_llama.npz"), cfg_keys=np.array(list(CFG.keys())),
                        cfg_vals=np.array([float(v) for v in CFG.values()]), S=S, wseed=WSEED, iseed=ISEED, wsum=wsum(W), ids=ids.numpy(),
                        idx=idx, logit=float(last[idx]), trace=trace.numpy(), resid=resid.numpy(), mlp=mlp.numpy(),
                        protocol=np.array("lxt.efficient.monkey_patch(modeling_llama), fp64, CPU, eager attention; hooks on decoder-layer "
                                          "outputs, the input embedding and mlp.down_proj inputs; arg-max logit of the last position seeded 1"))


if __name__ == "__main__":
    main(*sys.argv[1:2])
