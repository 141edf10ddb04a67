"""Worker for tests/test_qwen_moe_engine_gpu.py (its own process: monkey_patch is class-level and process-global): the bf16 Qwen3-MoE DROP-IN
(lxt_amd.efficient.monkey_patch + the quickstart protocol, the path the engine is measured against) on the planted-routing model of
tests/golden/moe_engine_models.py, compared with the fp32 ENGINE's outputs the test left in an .npz.  The per-expert relevance is read the
way the reference reads it: retain_grad on every router's routing weights, `w * w.grad` scattered by the selected experts.  Prints one
line `RESULT {json}`: normalised max error and cosine of R_tok and R_expert, and whether every routing choice matches."""
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")
from tests.golden import moe_engine_models as mm  # noqa: E402
from tests.util import nmax  # noqa: E402


def cos(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float(a @ b / (a.norm() * b.norm()))


def main(ref_path):
    from transformers.models.qwen3_moe import modeling_qwen3_moe
    from lxt_amd.efficient import monkey_patch
    ref = np.load(ref_path)
    monkey_patch(modeling_qwen3_moe)
    model = mm.build(attn="sdpa")
    for p in model.parameters():
        p.requires_grad_(False)
    model = model.cuda().to(torch.bfloat16)
    ids = mm.inputs().cuda()
    B, S = ids.shape
    kept = {}
    for li, L in enumerate(model.model.layers):
        if hasattr(L.mlp, "gate") and hasattr(L.mlp, "experts"):
            def hook(mod, inp, out, li=li):
                out[1].retain_grad()
                kept[li] = (out[2].detach(), out[1])
            L.mlp.gate.register_forward_hook(hook)
    e = model.get_input_embeddings()(ids).detach().requires_grad_()
    logits = model(inputs_embeds=e, use_cache=False).logits
    last = logits[:, -1]
    idx = last.argmax(-1)
    last[torch.arange(B), idx].sum().backward()
    R_tok = (e * e.grad).sum(-1).float()
    nL, E = len(model.model.layers), model.config.num_experts
    R_expert = torch.zeros(nL, B, E, dtype=torch.float64)
    same_routing = True
    for li, (sel, w) in kept.items():
        wg = (w.float() * w.grad.float()).double().cpu().view(B, -1)
        sel = sel.cpu().view(B, -1)
        for b in range(B):
            R_expert[li, b].index_add_(0, sel[b], wg[b])
        same_routing &= bool(torch.equal(sel.view(B, S, -1), torch.from_numpy(ref["expert_index"][li])))
    res = dict(idx=idx.tolist(), same_routing=same_routing,
               R_tok=[nmax(R_tok, ref["R_tok"]), cos(R_tok, torch.from_numpy(ref["R_tok"]))],
               R_expert=[nmax(R_expert, ref["R_expert"]), cos(R_expert, torch.from_numpy(ref["R_expert"]))])
    print("RESULT " + json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
