#!/usr/bin/env python3
"""Golden fixtures for the Qwen3-MoE drop-in, generated FROM THE REAL REFERENCE on the CPU (build container only):
    python tests/golden/make_golden_qwen3_moe.py
writes hf_qwen3_moe_{tiny,fanout,padded}.npz: ids, attention mask, idx, logit, R_tok (reference fp32), R_tok_fp64 (the reference run in
float64), wsum, and the smallest top-k routing margin (probability gap between the k-th and (k+1)-th expert over every real token and
layer of the fp32 run).  Asserts that the reference's fp32-vs-fp64 gap is small and that the margin is large enough that device rounding cannot flip
an expert choice.  Cases (tests/golden/moe_models.py): tiny (8 experts, top-2, norm_topk_prob, one dense layer), fanout (128 experts, top-8,
no renorm), padded (a left-padded batch of 2 on the tiny model)."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, "/root/reference")
warnings.simplefilter("ignore")

from tests.golden.moe_models import build_qwen3_moe, inputs, model_case, wsum  # noqa: E402


def explain(model, ids, am, pos, margins=None):
    """the quickstart protocol, per row: seed the arg-max logit at the row's last position"""
    hooks = []
    if margins is not None:
        def hook(mod, inp, out):
            probs = torch.softmax(out[0].detach().double(), -1).sort(-1, descending=True).values
            if am is not None:          # padding positions are masked keys: their routing reaches no real token
                probs = probs[am.flatten().bool()]
            margins.append(float((probs[:, mod.top_k - 1] - probs[:, mod.top_k]).min()))
        hooks = [m.register_forward_hook(hook) for m in model.modules() if type(m).__name__ == "Qwen3MoeTopKRouter"]
    e = model.get_input_embeddings()(ids).detach().requires_grad_()
    logits = model(inputs_embeds=e, attention_mask=am, use_cache=False).logits
    rows = torch.arange(ids.shape[0])
    last = logits[rows, pos]
    idx = last.argmax(-1)
    last[rows, idx].sum().backward()
    for h in hooks:
        h.remove()
    return idx, last[rows, idx].detach(), (e * e.grad).sum(-1).detach()


def main():
    from lxt.efficient import monkey_patch
    from transformers.models.qwen3_moe import modeling_qwen3_moe
    monkey_patch(modeling_qwen3_moe)
    for case in ("tiny", "fanout", "padded"):
        ids, am, pos = inputs(case)
        model = build_qwen3_moe(model_case(case))
        margins = []
        idx, logit, R = explain(model, ids, am, pos, margins)
        m64 = build_qwen3_moe(model_case(case)).double()
        if am is None:
            idx64, _, R64 = explain(m64, ids, am, pos)
        else:
            # float64 has no finite "minimum" mask value for the padding queries (their rows are fully masked: NaN softmax); left padding
            # changes no real token's scores (RoPE sees relative positions), so each row runs un-padded instead
            idx64, R64 = torch.zeros_like(idx), torch.zeros(ids.shape, dtype=torch.float64)
            for b in range(ids.shape[0]):
                v = am[b].bool()
                i_b, _, R_b = explain(m64, ids[b, v][None], None, torch.tensor([int(v.sum()) - 1]))
                idx64[b], R64[b, v] = i_b[0], R_b[0]
        valid = am.bool() if am is not None else torch.ones_like(ids, dtype=torch.bool)
        gap = max(float((R[b][valid[b]].double() - R64[b][valid[b]]).abs().max() / R64[b][valid[b]].abs().max()) for b in range(ids.shape[0]))
        margin = min(margins)
        print(f"[{case}] idx={idx.tolist()} logit={[round(float(v), 5) for v in logit]} sumR={[round(float(R[b][valid[b]].sum()), 5) for b in range(ids.shape[0])]} "
              f"reference fp32-vs-fp64 {gap:.1e} routing margin {margin:.2e}")
        assert torch.equal(idx, idx64) and gap < 1e-5 and margin >= 1e-4, (idx, idx64, gap, margin)
        np.savez_compressed(os.path.join(HERE, f"hf_qwen3_moe_{case}.npz"), ids=ids.numpy(),
                            mask=(am if am is not None else torch.ones_like(ids)).numpy(), pos=pos.numpy(), idx=idx.numpy(),
                            logit=logit.numpy(), R_tok=R.numpy(), R_tok_fp64=R64.float().numpy(), wsum=wsum(build_qwen3_moe(model_case(case))),
                            margin=margin, cond_gap=gap)


if __name__ == "__main__":
    main()
