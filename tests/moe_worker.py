"""Worker for tests/test_moe_gpu.py (one process per case -- the patches are class-level and process-global, like the reference's): patch
HF's modeling_qwen3_moe with lxt_amd, run the quickstart protocol on the GPU (eager and sdpa attention) and compare the token relevance
with the fixture captured from the real reference (tests/golden/make_golden_qwen3_moe.py): fp32 against the reference's fp32 and fp64 runs
(bar 1e-4), bf16 against its fp32 run (same arg-max, cosine >= 0.99)."""
import os
import sys
import warnings

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")
from tests.golden.moe_models import build_qwen3_moe, model_case, wsum  # noqa: E402
from tests.util import load, t, nmax  # noqa: E402


def explain(model, ids, am, pos):
    e = model.get_input_embeddings()(ids).detach().requires_grad_()
    logits = model(inputs_embeds=e, attention_mask=am, use_cache=False).logits
    rows = torch.arange(ids.shape[0], device=ids.device)
    last = logits[rows, pos]
    idx = last.argmax(-1)
    last[rows, idx].sum().backward()
    return idx, last[rows, idx].detach(), (e * e.grad).sum(-1).detach()


def cos(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float(a @ b / (a.norm() * b.norm()))


def main(case):
    from transformers.models.qwen3_moe import modeling_qwen3_moe
    from lxt_amd.efficient import monkey_patch
    from lxt_amd.efficient.moe import experts_forward
    fx = load(f"hf_qwen3_moe_{case}.npz")
    monkey_patch(modeling_qwen3_moe)
    assert modeling_qwen3_moe.Qwen3MoeExperts.forward is experts_forward
    ids, am, pos = t(fx["ids"]).cuda(), t(fx["mask"]).cuda(), t(fx["pos"]).cuda()
    valid = am.bool().cpu()
    worst, worst_cos = 0.0, 1.0
    for impl in ("eager", "sdpa"):
        model = build_qwen3_moe(model_case(case), attn=impl)
        assert abs(wsum(model) - float(fx["wsum"])) < 1e-6 * float(fx["wsum"]), "weights did not reproduce"
        for p in model.parameters():
            p.requires_grad_(False)
        model = model.cuda()
        idx, logit, R = explain(model, ids, am, pos)
        assert idx.tolist() == fx["idx"].tolist(), (idx.tolist(), fx["idx"])
        assert torch.allclose(logit.cpu(), t(fx["logit"]), rtol=1e-4, atol=1e-5), (logit, fx["logit"])
        assert torch.isfinite(R).all()
        for b in range(ids.shape[0]):
            e32 = nmax(R[b].cpu()[valid[b]], t(fx["R_tok"])[b][valid[b]])
            e64 = nmax(R[b].cpu()[valid[b]], t(fx["R_tok_fp64"])[b][valid[b]])
            worst = max(worst, e32, e64)
            print(f"[qwen3_moe {case}/{impl}/fp32 row {b}] vs reference fp32 {e32:.2e} | fp64 {e64:.2e}")
        model = model.to(torch.bfloat16)
        idx, _, R = explain(model, ids, am, pos)
        assert idx.tolist() == fx["idx"].tolist(), ("bf16", idx.tolist(), fx["idx"])
        for b in range(ids.shape[0]):
            c = cos(R[b].float().cpu()[valid[b]], t(fx["R_tok"])[b][valid[b]])
            worst_cos = min(worst_cos, c)
            print(f"[qwen3_moe {case}/{impl}/bf16 row {b}] cosine vs reference fp32 {c:.5f}")
        del model
    print(f"WORST fp32 {worst:.3e} bf16 cosine {worst_cos:.5f}")
    return 0 if worst < 1e-4 and worst_cos >= 0.99 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
