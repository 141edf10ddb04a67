#!/usr/bin/env python3
"""Fixture generator (build container only; imports the REAL reference, e.g. through LXT_REFERENCE or PYTHONPATH): mxfp4_qwen3_moe_tiny.npz =
the reference's explanation of the seeded "tiny" Qwen3-MoE of tests/golden/moe_models.py whose routed experts' tensors (gate_up_proj
[E, 2 I, H], down_proj [E, H, I] of every sparse layer) were replaced by their MXFP4 quantise-dequantise images -- what
Qwen3MoeLRP(weight_format="mxfp4") computes with; everything else (attention, routers, the dense layer, norms, embedding, head) as built.
`lxt.efficient.monkey_patch(modeling_qwen3_moe)`, CPU, eager attention, fp64, the quickstart protocol; the routing-weight and block hooks are
those of make_golden_qwen3_moe_experts.py (imported), the format is the numpy restatement of make_golden_mxfp4.py (imported) applied to the
tensor viewed as [E N, K].

Frozen: ids, idx, logit, R_tok [1, S], R_expert [L, 1, E], expert_index [L, 1, S, k], R_block [L, 1] (fp64), layer 0's down_proj as
`wd_codes` [E, H, I / 2] and `wd_scales` [E, H, I / 32], the routing margin, the reference's fp32-vs-fp64 gap and wsum of the ORIGINAL model.

Asserted before anything is written: top-k routing margin >= 1e-4 (4-bit experts move the router inputs of the later layers: the "fanout" and
"padded" cases at their committed seeds fall to 2.9e-5 / 3.6e-5 and are not used here), the reference's own fp32 run picks the same logit
and the same experts and is within 1e-5 (normalised max) of its fp64 run on R_tok, R_expert and R_block, and sum_e R_expert = 1/2 R_block."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")

from tests.golden.make_golden_mxfp4 import mx_dequant, mx_quantize  # noqa: E402
from tests.golden.make_golden_qwen3_moe_experts import explain  # noqa: E402
from tests.golden.moe_models import build_qwen3_moe, inputs, wsum  # noqa: E402

CASE, MARGIN_BAR, FP32_BAR, MAX_BYTES = "tiny", 1e-4, 1e-5, 1 << 20


def quantise_experts(model):
    """every routed expert tensor <- its quantise-dequantise image, in place -> (codes, scales) of layer 0's down_proj"""
    kept = None
    for li, L in enumerate(model.model.layers):
        if not (hasattr(L.mlp, "gate") and hasattr(L.mlp, "experts")):
            continue
        for name in ("gate_up_proj", "down_proj"):
            p = getattr(L.mlp.experts, name)
            E, N, K = p.shape
            codes, scales = mx_quantize(p.detach().float().numpy().reshape(E * N, K))
            img = mx_dequant(codes, scales)
            c2, s2 = mx_quantize(img.astype(np.float32))
            assert np.array_equal(c2, codes) and np.array_equal(s2, scales), "quantise(dequant(q)) != q"
            with torch.no_grad():
                p.copy_(torch.from_numpy(img).reshape(E, N, K).to(p.dtype))
            if kept is None and name == "down_proj":
                kept = codes.reshape(E, N, K // 2), scales.reshape(E, N, K // 32)
    return kept


def run(model, ids):
    """one prompt -> (idx, logit, R_tok [S], R_expert [L, E], expert_index [L, S, k], R_block [L], margin)"""
    cfg = model.config
    L, E, k, S = cfg.num_hidden_layers, cfg.num_experts, cfg.num_experts_per_tok, ids.shape[1]
    idx, logit, R, per_layer, margin = explain(model, ids)
    R_expert, R_block = torch.zeros(L, E, dtype=torch.float64), torch.zeros(L, dtype=torch.float64)
    index = torch.full((L, S, k), -1, dtype=torch.int64)
    for li, entry in enumerate(per_layer):
        if entry is not None:
            sel, wg, blk = entry
            index[li] = sel
            R_expert[li].index_add_(0, sel.flatten(), wg.flatten().double())
            R_block[li] = blk
    return idx, logit, R.double(), R_expert, index, R_block, margin


def main(reference=os.environ.get("LXT_REFERENCE", "")):
    if reference:
        sys.path.insert(0, reference)
    from lxt.efficient import monkey_patch
    from transformers.models.qwen3_moe import modeling_qwen3_moe
    monkey_patch(modeling_qwen3_moe)
    ids, _, _ = inputs(CASE)
    model = build_qwen3_moe(CASE)
    total = wsum(model)                                          # (of the ORIGINAL weights: what the engine under test is given)
    codes, scales = quantise_experts(model)
    idx32, _, R32, Re32, index32, Rb32, _ = run(model, ids)
    idx, logit, R, Re, index, Rb, margin = run(model.double(), ids)
    nm = lambda a, b: float((a - b).abs().max() / b.abs().max())      # noqa: E731
    gap = max(nm(R32, R), nm(Re32, Re), nm(Rb32, Rb))
    ident = float((Re.sum(-1) - 0.5 * Rb).abs().max() / Re.abs().max())
    print(f"[{CASE}] idx {idx} logit {logit:+.6f} routing margin {margin:.2e} reference fp32 vs fp64: idx {idx32}, normalised max {gap:.2e}; "
          f"1/2-identity {ident:.1e}")
    assert margin >= MARGIN_BAR, "the quantised experts leave a routing tie: choose another case"
    assert idx32 == idx and torch.equal(index32, index) and gap <= FP32_BAR, "badly conditioned instance"
    assert ident <= 1e-12
    path = os.path.join(HERE, f"mxfp4_qwen3_moe_{CASE}.npz")
    np.savez_compressed(path, ids=ids.numpy(), idx=np.asarray([idx]), logit=np.asarray([logit]), R_tok=R.numpy()[None], R_expert=Re.numpy()[:, None],
                        expert_index=index.numpy()[:, None], R_block=Rb.numpy()[:, None], wd_codes=codes, wd_scales=scales, margin=margin,
                        ref_fp32_gap=gap, wsum=total,
                        protocol=np.array("lxt.efficient.monkey_patch(modeling_qwen3_moe), fp64, CPU, eager attention, on the MXFP4 "
                                          "quantise-dequantise images of every routed expert tensor; arg-max logit of the last position seeded 1"))
    print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) <= MAX_BYTES


if __name__ == "__main__":
    main(*sys.argv[1:2])
