#!/usr/bin/env python3
"""Golden fixtures for dense Qwen2 / Qwen3 at shapes the fused decoder layer takes, generated FROM THE REAL REFERENCE (build container only,
the reference checkout on PYTHONPATH):   python tests/golden/make_golden_qwen_fused.py [case]

  qwen_fused_<case>.npz   tests/golden/qwen_models.py::build(case) under lxt.efficient.monkey_patch(modeling_qwen2 / modeling_qwen3), quickstart
                          protocol (embed ids -> forward -> arg-max of the last position -> backward -> sum_h emb (*) grad), fp32 and fp64 (the
                          fp64 run explains the fp32 run's idx).  ids [B, S], idx [B], logit [B], R_tok [B, S] fp32, R_tok_fp64 [B, S] fp64,
                          layer_R [L + 1, B] fp64 (sum of hidden (*) grad at every residual boundary), wsum (weight checksum), gap [B],
                          margin [B] (fp32: the explained logit minus the runner-up).
The reference's own fp32-vs-fp64 gap must be below 1e-4 on every prompt: the GPU tests hold the engine to 1e-4 against the fp64 run."""
import importlib
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
warnings.simplefilter("ignore")

from tests.golden import qwen_models as qm          # noqa: E402

CHUNK = 4          # prompts per reference run (eager attention keeps [B, heads, S, S] per layer)


def nmax(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max())


def explain(model, ids, target=None):
    """quickstart protocol on a batch: rows are independent, so one backward of the summed seeds explains every prompt"""
    hs = []
    hooks = [L.register_forward_pre_hook(lambda m, a, k: hs.append(a[0] if a else k["hidden_states"]), with_kwargs=True) for L in model.model.layers]
    hooks.append(model.model.norm.register_forward_pre_hook(lambda m, a: hs.append(a[0])))
    e = model.get_input_embeddings()(ids).detach().requires_grad_()
    last = model(inputs_embeds=e, use_cache=False).logits[:, -1]
    for h in hs:
        h.retain_grad()
    idx = last.argmax(-1) if target is None else target
    rows = torch.arange(ids.shape[0])
    last[rows, idx].sum().backward()
    for h in hooks:
        h.remove()
    layer_R = torch.stack([(h * h.grad).sum((1, 2)).detach() for h in hs])
    top2 = last.detach().topk(2, -1).values
    return idx, last[rows, idx].detach(), (e * e.grad).sum(-1).detach(), layer_R, top2[:, 0] - top2[:, 1]


def make(case):
    from lxt.efficient import monkey_patch
    fam = qm.CASES[case]["family"]
    monkey_patch(importlib.import_module(f"transformers.models.{fam}.modeling_{fam}"))
    ids = qm.prompts(case)
    res = {}
    for dtype in (torch.float32, torch.float64):
        model = qm.build(case).to(dtype)
        for p in model.parameters():
            p.requires_grad_(False)
        parts = []
        for b0 in range(0, ids.shape[0], CHUNK):
            tgt = None if dtype == torch.float32 else res[torch.float32][0][b0: b0 + CHUNK]
            parts.append(explain(model, ids[b0: b0 + CHUNK], tgt))
        res[dtype] = [torch.cat([p[i] for p in parts], 1 if i == 3 else 0) for i in range(5)]
    (idx, logit, R, _, margin), (_, _, R64, lR64, _) = res[torch.float32], res[torch.float64]
    gap = [nmax(R[b], R64[b]) for b in range(ids.shape[0])]
    print(f"  [{case}] idx={idx.tolist()} sumR[0]={float(R64[0].sum()):.6f} reference fp32-vs-fp64 gap max {max(gap):.2e}")
    assert max(gap) < 1e-4, "pick another seed, not a wider bar"
    np.savez_compressed(os.path.join(HERE, f"qwen_fused_{case}.npz"), ids=ids.numpy().astype(np.int16), idx=idx.numpy(), logit=logit.numpy(),
                        R_tok=R.numpy(), R_tok_fp64=R64.numpy(), layer_R=lR64.numpy(), wsum=qm.wsum(qm.build(case)), gap=np.array(gap), margin=margin.numpy())


if __name__ == "__main__":
    torch.set_num_threads(8)
    which = sys.argv[1:] or list(qm.CASES)
    if len(which) > 1:          # lxt's patches are process-global: one family per process
        import subprocess
        for w in which:
            subprocess.run([sys.executable, os.path.abspath(__file__), w], check=True)
    else:
        make(which[0])
