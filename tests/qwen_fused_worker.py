"""Worker (one process per case: the patches are class-level and process-global): a seeded dense Qwen2 / Qwen3 model in bf16 under
lxt_amd.efficient.monkey_patch, once on the per-module patches (the yardstick) and once with every decoder layer on the fused layer, both
against the real reference's fp64 relevance (tests/golden/qwen_fused_<case>.npz); with "engine": QwenLRP in bf16 held to the same bar.
    python tests/qwen_fused_worker.py <case> [engine]"""
import importlib
import os
import sys
import warnings

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")
from tests.golden import qwen_models as qm  # noqa: E402
from tests.util import load, t, nmax  # noqa: E402


def cos(a, b):
    return float(torch.nn.functional.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0))


def main(case, engine):
    fx = load(f"qwen_fused_{case}.npz")
    fam = qm.CASES[case]["family"]
    from lxt_amd.efficient import monkey_patch
    import lxt_amd.efficient.patches as P
    mod = importlib.import_module(f"transformers.models.{fam}.modeling_{fam}")
    monkey_patch(mod)
    assert getattr(mod, f"{fam.capitalize()}DecoderLayer").forward is P.decoder_layer_forward
    ids, tgt = t(fx["ids"]).long().cuda(), t(fx["idx"]).long().cuda()
    B, S = ids.shape
    R64 = t(fx["R_tok_fp64"])

    def run(fuse_layer):
        model = qm.build(case, attn="sdpa")
        assert abs(qm.wsum(model) - float(fx["wsum"])) < 1e-6 * float(fx["wsum"]), "weights did not reproduce"
        model = qm.to_bf16_rotary_fp32(model).cuda()
        P.FUSE_LAYER = fuse_layer
        try:
            e = model.get_input_embeddings()(ids).detach().requires_grad_()
            last = model(inputs_embeds=e, use_cache=False).logits[:, -1]
            last[torch.arange(B), tgt].sum().backward()
            used = [bool(L.__dict__.get("_lrp_fused_layer", {}).get("ok_rows", {}).get((B, S), False)) for L in model.model.layers]
            return (e * e.grad).float().sum(-1).double().cpu(), used
        finally:
            P.FUSE_LAYER = True
    Rb, ub = run(False)
    Ra, ua = run(True)
    assert all(ua) and not any(ub), (ua, ub)          # every layer on the fused node with it on, none with it off
    e_a, e_b = [nmax(Ra[b], R64[b]) for b in range(B)], [nmax(Rb[b], R64[b]) for b in range(B)]
    print(f"[{case} drop-in bf16 vs reference fp64, per prompt] fused layer {[f'{x:.2e}' for x in e_a]} (cos {cos(Ra, R64):.6f})")
    print(f"[{case} drop-in bf16 vs reference fp64, per prompt] per-module {[f'{x:.2e}' for x in e_b]} (cos {cos(Rb, R64):.6f})")
    print(f"[{case}] max fused {max(e_a):.3e}  max per-module {max(e_b):.3e}  fused vs per-module {nmax(Ra, Rb):.2e}")
    if not engine:
        assert torch.isfinite(Ra).all() and cos(Ra, R64) > 0.999 and max(e_a) < max(2e-2, 1.5 * max(e_b)), (max(e_a), max(e_b), cos(Ra, R64))
        return
    import lxt_amd.engine_qwen as Q
    eng = Q.QwenLRP.from_hf(qm.to_bf16_rotary_fp32(qm.build(case)), max_seq=S)
    assert eng.dtype == torch.bfloat16 and eng._fused(B * S).full
    out = eng.explain(ids, target=tgt)
    Re = out["R_tok"].double().cpu()
    e_e = [nmax(Re[b], R64[b]) for b in range(B)]
    free = eng.explain(ids)
    print(f"[{case} QwenLRP bf16 vs reference fp64, per prompt] {[f'{x:.2e}' for x in e_e]} (cos {cos(Re, R64):.6f}); max {max(e_e):.3e}")
    # the engine's own arg-max: a bf16 forward cannot order two logits closer than its rounding.  The project's bf16 bar is 2e-2 normalised
    # (the floor of the bar below; 8 significand bits through 3 layers' residual sums), so the arg-max is held to the reference's on every
    # prompt whose fp32 margin over the runner-up exceeds 2e-2 of the explained logit's magnitude, and elsewhere the engine's logit of the
    # reference's idx must lie within that distance of its maximum
    same = free["idx"].cpu().long() == tgt.cpu()
    tol = 2e-2 * t(fx["logit"]).abs().double()
    decisive = t(fx["margin"]).double() > tol
    lg = free["logits"].double().cpu()
    short = lg.max(-1).values - lg[torch.arange(B), tgt.cpu()]
    print(f"[{case}] QwenLRP bf16 vs the fused drop-in (reported, not gated): nmax {nmax(Re, Ra):.2e}; arg-max idx equal to the fixture's on "
          f"{int(same.sum())} of {B} prompts ({int(decisive.sum())} decisive; margins of the others {t(fx['margin'])[~decisive].tolist()})")
    assert out["idx"].cpu().long().tolist() == tgt.cpu().tolist()
    assert bool(same[decisive].all()) and bool((short <= tol).all()), (same.tolist(), short.tolist(), tol.tolist())
    assert torch.isfinite(Re).all() and cos(Re, R64) > 0.999 and max(e_e) < max(2e-2, 1.5 * max(e_b)), (max(e_e), max(e_b), cos(Re, R64))


if __name__ == "__main__":
    main(sys.argv[1], len(sys.argv) > 2 and sys.argv[2] == "engine")
    print("ok")
