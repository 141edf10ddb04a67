#!/usr/bin/env python3
"""Golden fixtures for the per-expert relevance of Qwen3MoeLRP.explain(experts=True), generated FROM THE REAL REFERENCE on the CPU in float64
(build container only; the reference's `lxt` package must be importable, e.g. through PYTHONPATH):
    python tests/golden/make_golden_qwen3_moe_experts.py
writes qwen3_moe_experts_{tiny,fanout,padded}.npz: R_expert [L, B, E] -- `routing_weights * routing_weights.grad` of every router
(retain_grad), scattered by `selected_experts` and summed over a prompt's tokens, rows of dense layers 0 --, expert_index [L, B, S, k]
(-1 on dense layers and at pad positions), R_block [L, B] = sum_{t, j} out (*) out.grad at every sparse block's output (retain_grad), and
R_tok, idx, logit of the same run.  Asserts sum_e R_expert = 1/2 R_block to 1e-12 of the largest value (the weighted expert output passes
divide_gradient(., 2)) and a top-k routing margin >= 1e-4, the bar of make_golden_qwen3_moe.py.  The padded case runs each prompt un-padded,
as that script does (float64 has no finite mask value for the fully masked padding queries).  Cases: tests/golden/moe_models.py."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
warnings.simplefilter("ignore")

from tests.golden.moe_models import build_qwen3_moe, inputs, model_case  # noqa: E402


def explain(model, ids):
    """one un-padded prompt [1, S] through the quickstart protocol, with retain_grad on every router's routing weights and every sparse
    block's output -> (idx, logit, R_tok [S], per layer None or (selected_experts [S, k], w * w.grad [S, k], sum out * out.grad), margin)"""
    kept, margins, hooks = {}, [], []
    layers = model.model.layers

    def router_hook(li):
        def hook(mod, inp, out):
            probs = torch.softmax(out[0].detach().double(), -1).sort(-1, descending=True).values
            margins.append(float((probs[:, mod.top_k - 1] - probs[:, mod.top_k]).min()) if probs.shape[1] > mod.top_k else 1.0)
            out[1].retain_grad()
            kept[li] = [out[2].detach(), out[1]]
        return hook

    def block_hook(li):
        def hook(mod, inp, out):
            out.retain_grad()
            kept[li].append(out)
        return hook

    for li, L in enumerate(layers):
        if hasattr(L.mlp, "gate") and hasattr(L.mlp, "experts"):
            hooks += [L.mlp.gate.register_forward_hook(router_hook(li)), L.mlp.register_forward_hook(block_hook(li))]
    e = model.get_input_embeddings()(ids).detach().requires_grad_()
    logits = model(inputs_embeds=e, use_cache=False).logits
    last = logits[0, -1]
    idx = last.argmax(-1)
    last[idx].backward()
    for h in hooks:
        h.remove()
    per_layer = [None] * len(layers)
    for li, (sel, w, out) in kept.items():
        per_layer[li] = (sel, (w * w.grad).detach(), float((out * out.grad).sum()))
    return int(idx), float(last[idx]), (e * e.grad).sum(-1).detach()[0], per_layer, min(margins)


def main():
    from lxt.efficient import monkey_patch
    from transformers.models.qwen3_moe import modeling_qwen3_moe
    monkey_patch(modeling_qwen3_moe)
    for case in ("tiny", "fanout", "padded"):
        ids, am, _ = inputs(case)
        model = build_qwen3_moe(model_case(case)).double()
        cfg = model.config
        B, S = ids.shape
        L, E, k = cfg.num_hidden_layers, cfg.num_experts, cfg.num_experts_per_tok
        valid = am.bool() if am is not None else torch.ones_like(ids, dtype=torch.bool)
        R_expert, R_block = torch.zeros(L, B, E, dtype=torch.float64), torch.zeros(L, B, dtype=torch.float64)
        index = torch.full((L, B, S, k), -1, dtype=torch.int64)
        R_tok, idx, logit, margin = torch.zeros(B, S, dtype=torch.float64), [], [], 1.0
        for b in range(B):
            i_b, l_b, R_b, per_layer, m_b = explain(model, ids[b, valid[b]][None])
            idx.append(i_b)
            logit.append(l_b)
            R_tok[b, valid[b]] = R_b
            margin = min(margin, m_b)
            for li, entry in enumerate(per_layer):
                if entry is not None:
                    sel, wg, blk = entry
                    index[li, b, valid[b]] = sel
                    R_expert[li, b].index_add_(0, sel.flatten(), wg.flatten())
                    R_block[li, b] = blk
        moe = [li for li in range(L) if bool((index[li] >= 0).any())]
        ident = float((R_expert.sum(-1) - 0.5 * R_block).abs().max() / R_expert.abs().max())
        print(f"[{case}] idx={idx} sparse layers {moe} sum_e R_expert={R_expert.sum(-1)[moe].flatten().tolist()} 1/2-identity {ident:.1e} "
              f"routing margin {margin:.2e}")
        assert ident <= 1e-12 and margin >= 1e-4, (ident, margin)
        np.savez_compressed(os.path.join(HERE, f"qwen3_moe_experts_{case}.npz"), R_expert=R_expert.numpy(), expert_index=index.numpy(),
                            R_block=R_block.numpy(), R_tok=R_tok.numpy(), idx=np.asarray(idx), logit=np.asarray(logit), margin=margin)


if __name__ == "__main__":
    main()
