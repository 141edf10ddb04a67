#!/usr/bin/env python3
"""Fixture generator (build container only; imports the REAL reference): the token-to-token attention relevance of `lxt.efficient.monkey_patch`
(ref lxt/efficient/models/llama.py:9-14, qwen3.py; lxt/efficient/patches.py:193-203) run on the CPU in fp64, eager attention, the arg-max
logit of the last position seeded with 1.
  attn_map_llama.npz: the seeded Llama of heads_llama.npz (4 layers, 8 + 2 heads of 32, S 128, weight seed 2, id seed 12);
  attn_map_qwen3.npz: tests.golden.hf_models.build_qwen3() (3 layers, 4 + 2 heads of 32, per-head q / k norms), S 80, id seed 99.

Protocol (what a user of the reference does with `attn_weights.retain_grad()`):
  1. HF's eager attention passes the probabilities -- the tensor that multiplies `value` -- through torch.nn.functional.dropout on their way
     to that product.  For the duration of the run that function is wrapped: it retains the gradient of its input and keeps it.  The
     reference sets the rate to 0, so the call is the identity and the run is the reference's own;
  2. the module's eager_attention_forward is wrapped once more (outside the reference's divide_gradient) to keep query, key and value, and a
     forward pre-hook retains the gradient of every o_proj input.
Frozen: ids [S], idx, logit;  total [L, S, S] fp64 = sum over the query heads of P (*) P.grad;  per_head [len(head_layers), nq, S, S]
float32 (the bars of the tests are 1e-4) for the layers listed in head_layers: all of them (each file stays under the size limit of a
committed file, which is asserted).
Asserted before anything is written, each to 1e-12 of the largest value of the maps:
  the rows of every head's map sum to sum_d o (*) o.grad at the o projection's input, which is heads_*.npz's `out`;
  the map equals P (*) (G_o V^T) with G_o V^T recomputed in fp64 from o.grad and the repeated value;
  it is 0 above the diagonal;  in the top layer only the last row is non-zero.
HF's eager attention evaluates its softmax in float32 whatever the model's dtype, so the retained P is an fp32-rounded softmax of the fp64
scores: against the fp64 softmax recomputed from the retained query and repeated key it is asserted to 1e-6 (printed), not to 1e-12."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")

from tests.golden.make_golden_heads import CFG, S, WSEED, ISEED, QWEN_S, QWEN_ISEED, wsum      # noqa: E402  (the same two cases)

PROTOCOL = ("lxt.efficient.monkey_patch(modeling module), fp64, CPU, eager attention; retain_grad on the probabilities (the input of the "
            "functional dropout call inside eager_attention_forward: the tensor that multiplies value) and on every o_proj input; "
            "map = P * P.grad; arg-max logit of the last position seeded 1")
MAX_BYTES = 1 << 20              # of one .npz: the size limit of a committed file


def attn_maps(mod, model, ids):
    """-> (idx, logit, maps [L, nq, S, S] fp64) of one explanation of `model` (an instance of the already monkey-patched module `mod`)"""
    probs, qkv, oin = [], [], []
    F = torch.nn.functional
    inner, dropout = mod.eager_attention_forward, F.dropout

    def attention(module, query, key, value, *args, **kw):
        qkv.append((query, key, value, module.num_key_value_groups))
        return inner(module, query, key, value, *args, **kw)

    def dropout_kept(x, *args, **kw):
        if x.dim() == 4 and x.shape[-1] == x.shape[-2] == ids.numel():          # (the probabilities [1, nq, S, S]; nothing else has that shape)
            x.retain_grad()
            probs.append(x)
        return dropout(x, *args, **kw)

    def keep_in(m, args):
        args[0].retain_grad()
        oin.append(args[0])

    mod.eager_attention_forward, F.dropout = attention, dropout_kept
    hooks = [L.self_attn.o_proj.register_forward_pre_hook(keep_in) for L in model.model.layers]
    try:
        e = model.get_input_embeddings()(ids[None]).detach().requires_grad_()
        last = model(inputs_embeds=e, use_cache=False).logits[0, -1]
        idx = int(last.argmax())
        last[idx].backward()
    finally:
        mod.eager_attention_forward, F.dropout = inner, dropout
        for h in hooks:
            h.remove()
    nL, n = len(model.model.layers), ids.numel()
    assert len(probs) == nL and len(qkv) == nL and len(oin) == nL
    maps = torch.stack([(P * P.grad)[0] for P in probs]).detach()
    nq = maps.shape[1]
    scale = float(maps.abs().max())
    out = torch.stack([(o * o.grad)[0].view(n, nq, -1).sum(-1).T for o in oin]).detach()
    e_row = float((maps.sum(-1) - out).abs().max())
    e_gp = e_p = 0.0
    for l, (P, (q, k, v, rep), o) in enumerate(zip(probs, qkv, oin)):
        kr, vr = k.detach().repeat_interleave(rep, 1)[0], v.detach().repeat_interleave(rep, 1)[0]
        go = o.grad[0].view(n, nq, -1).permute(1, 0, 2)
        e_gp = max(e_gp, float((maps[l] - P.detach()[0] * (go @ vr.transpose(1, 2))).abs().max()))
        sc = (q.detach()[0] @ kr.transpose(1, 2)) * (q.shape[-1] ** -0.5)
        sc = sc.masked_fill(torch.ones(n, n, dtype=torch.bool).triu(1), float("-inf"))
        e_p = max(e_p, float((torch.softmax(sc, -1) - P.detach()[0]).abs().max()))
    upper = float(maps.triu(1).abs().max())
    top_off = float(maps[-1, :, :-1].abs().max())
    print(f"idx {idx} logit {float(last[idx]):+.6f}  max|map| {scale:.3e}  row sums - out {e_row:.1e}  map - P (G_o V^T) {e_gp:.1e}  "
          f"retained P - fp64 softmax {e_p:.1e}  above the diagonal {upper:.1e}  top layer off the last row {top_off:.1e}")
    assert e_row <= 1e-12 * scale and e_gp <= 1e-12 * scale and upper == 0.0 and top_off == 0.0 and e_p <= 1e-6
    assert float(maps[-1, :, -1].abs().max()) > 0
    return idx, float(last[idx]), maps.numpy(), out.numpy()


def save(path, maps, heads_out, **meta):
    """the per-head maps of every layer as float32, the head sum of every layer in fp64"""
    scale = np.abs(maps).max()
    assert np.abs(heads_out - maps.sum(-1)).max() <= 1e-12 * scale, "row sums do not reproduce the `out` map of the heads fixture"
    np.savez_compressed(path, total=maps.sum(1), per_head=maps.astype(np.float32), head_layers=np.arange(maps.shape[0]), **meta)
    print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) <= MAX_BYTES


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
    ids = torch.randint(0, CFG["vocab"], (S,), generator=torch.Generator().manual_seed(ISEED))
    idx, logit, maps, _ = attn_maps(modeling_llama, hf_models.build_llama_from_weights(CFG, W, attn="eager", dtype=torch.float64), ids)
    save(os.path.join(HERE, "attn_map_llama.npz"), maps, np.load(os.path.join(HERE, "heads_llama.npz"))["out"], cfg_keys=np.array(list(CFG.keys())),
         cfg_vals=np.array([float(v) for v in CFG.values()]), S=S, wseed=WSEED, iseed=ISEED, wsum=wsum(W), ids=ids.numpy(), idx=idx, logit=logit,
         protocol=np.array(PROTOCOL))
    monkey_patch(modeling_qwen3)
    ids = torch.randint(0, 256, (QWEN_S,), generator=torch.Generator().manual_seed(QWEN_ISEED))
    idx, logit, maps, _ = attn_maps(modeling_qwen3, hf_models.build_qwen3(attn="eager").double(), ids)
    save(os.path.join(HERE, "attn_map_qwen3.npz"), maps, np.load(os.path.join(HERE, "heads_qwen3.npz"))["out"], S=QWEN_S, iseed=QWEN_ISEED,
         wsum=hf_models.wsum(hf_models.build_qwen3()), ids=ids.numpy(), idx=idx, logit=logit, protocol=np.array(PROTOCOL))


if __name__ == "__main__":
    main(*sys.argv[1:2])
