#!/usr/bin/env python3
"""Fixture generator (build container only; imports the REAL reference): the per-weight relevance `weight * weight.grad` of every decoder
Linear under `lxt.efficient.monkey_patch` (ref lxt/efficient/models/llama.py:9-14, qwen3.py), run on the CPU in fp64, eager attention, the
arg-max logit of the last position seeded with 1; two prompts of S = 48, explained one after the other.

Rows in HF order: qkv = q_proj | k_proj | v_proj rows, gate_up = gate_proj rows then up_proj rows.  Stored as fp32.  One layer's four
matrices are 0.56 MiB, so the fixture is split into files of under 1 MiB each:
  weight_relevance_llama_l{0,1,2}.npz: the seeded Llama (3 layers, H 128, I 256, 2 + 1 heads of 64, V 512; weight seed 4, id seeds 21 / 22),
      qkv [256, 128], o [128, 128], gate_up [512, 128], down [128, 256] of one layer, SUMMED over the two prompts;
  weight_relevance_llama_prompts.npz: ids [2, S], idx [2], logit [2] and the PER-PROMPT values that fit: o [2, L, 128, 128] of every
      layer, qkv_top [2, 256, 128] and down_top [2, 128, 256] of the top layer (the layer the engine evaluates on one row per prompt);
  weight_relevance_qwen3_l{0,2}.npz: tests.golden.hf_models.build_qwen3() (3 layers, 4 + 2 heads of 32, per-head q / k norms), id seeds
      31 / 32, the summed matrices of the first and the top layer only (a subset of its layers: the third would be a fifth file of this
      size), plus ids / idx / logit."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")

CFG = dict(hidden=128, inter=256, n_layers=3, n_heads=2, n_kv=1, head_dim=64, vocab=512, rope_theta=10000.0, rms_eps=1e-5)
S, WSEED, ISEEDS = 48, 4, (21, 22)
QWEN_ISEEDS, QWEN_LAYERS = (31, 32), (0, 2)
NAMES = ("qkv", "o", "gate_up", "down")
PROTOCOL = ("lxt.efficient.monkey_patch(modeling module), fp64, CPU, eager attention; arg-max logit of the last position seeded 1; "
            "p * p.grad of every decoder Linear, per prompt and summed over the prompts")


def wsum(W):
    tot = float(W["embed"].double().abs().sum() + W["lm_head"].double().abs().sum())
    for L in W["layers"]:
        tot += sum(float(v.double().abs().sum()) for v in L.values())
    return tot


def weight_relevance(model, ids):
    """-> (idx, logit, {name: [L, N, K] fp64}) of one explanation of one prompt"""
    for p_ in model.parameters():          # (the fixture builders freeze their models)
        p_.requires_grad_(True)
    model.zero_grad(set_to_none=True)
    e = model.get_input_embeddings()(ids[None]).detach().requires_grad_()
    last = model(inputs_embeds=e, use_cache=False).logits[0, -1]
    idx = int(last.argmax())
    last[idx].backward()
    rel = lambda lin: (lin.weight * lin.weight.grad).detach()          # noqa: E731
    out = {n: [] for n in NAMES}
    for L in model.model.layers:
        a, m = L.self_attn, L.mlp
        out["qkv"].append(torch.cat([rel(a.q_proj), rel(a.k_proj), rel(a.v_proj)]))
        out["o"].append(rel(a.o_proj))
        out["gate_up"].append(torch.cat([rel(m.gate_proj), rel(m.up_proj)]))
        out["down"].append(rel(m.down_proj))
    return idx, float(last[idx]), {n: torch.stack(v) for n, v in out.items()}


def run(model, vocab, seeds):
    ids = torch.stack([torch.randint(0, vocab, (S,), generator=torch.Generator().manual_seed(s)) for s in seeds])
    res = [weight_relevance(model, row) for row in ids]
    per = {n: torch.stack([r[2][n] for r in res]) for n in NAMES}              # [prompts, L, N, K]
    meta = dict(S=S, ids=ids.numpy(), idx=np.array([r[0] for r in res]), logit=np.array([r[1] for r in res]), protocol=np.array(PROTOCOL))
    for n in NAMES:
        print(f"  {n}: {tuple(per[n].shape)} max|R_W| {float(per[n].abs().max()):.3e}  sum {[float(x) for x in per[n].sum((1, 2, 3))]}")
    return meta, per


def f32(t):
    return t.to(torch.float32).numpy()


def main(reference=os.environ.get("LXT_REFERENCE", "")):
    if reference:
        sys.path.insert(0, reference)
    from lxt.efficient import monkey_patch
    from transformers.models.llama import modeling_llama
    from transformers.models.qwen3 import modeling_qwen3
    from oracle import llama as ol
    from tests.golden import hf_models
    monkey_patch(modeling_llama)
    W = ol.random_weights(CFG, seed=WSEED)
    meta, per = run(hf_models.build_llama_from_weights(CFG, W, attn="eager", dtype=torch.float64), CFG["vocab"], ISEEDS)
    cfgkw = dict(cfg_keys=np.array(list(CFG.keys())), cfg_vals=np.array([float(v) for v in CFG.values()]), wseed=WSEED, wsum=wsum(W))
    for l in range(CFG["n_layers"]):
        np.savez_compressed(os.path.join(HERE, f"weight_relevance_llama_l{l}.npz"), layer=l, **{n: f32(per[n].sum(0)[l]) for n in NAMES})
    top = CFG["n_layers"] - 1
    np.savez_compressed(os.path.join(HERE, "weight_relevance_llama_prompts.npz"), **meta, **cfgkw, iseeds=np.array(ISEEDS), o=f32(per["o"]),
                        qkv_top=f32(per["qkv"][:, top]), down_top=f32(per["down"][:, top]))
    monkey_patch(modeling_qwen3)
    meta, per = run(hf_models.build_qwen3(attn="eager").double(), 256, QWEN_ISEEDS)
    for l in QWEN_LAYERS:
        np.savez_compressed(os.path.join(HERE, f"weight_relevance_qwen3_l{l}.npz"), layer=l, **meta, iseeds=np.array(QWEN_ISEEDS),
                            wsum=hf_models.wsum(hf_models.build_qwen3()), **{n: f32(per[n].sum(0)[l]) for n in NAMES})


if __name__ == "__main__":
    main(*sys.argv[1:2])
