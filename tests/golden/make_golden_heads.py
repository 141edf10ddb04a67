#!/usr/bin/env python3
"""Fixture generator (build container only; imports the REAL reference): the per-head attention relevance of `lxt.efficient.monkey_patch`
(ref lxt/efficient/models/llama.py:9-14, qwen3.py; lxt/efficient/patches.py: patch_attention) run on the CPU in fp64, eager attention, the
arg-max logit of the last position seeded with 1.
  heads_llama.npz: the seeded Llama of latent_llama.npz (4 layers, 8 + 2 heads of 32, S 128, weight seed 2, id seed 12);
  heads_qwen3.npz: tests.golden.hf_models.build_qwen3() (3 layers, 4 + 2 heads of 32, per-head q / k norms), S 80, id seed 99.

Protocol (what a user of the reference does with retain_grad()):
  1. after monkey_patch, the module's eager_attention_forward is wrapped once more; the wrapper retains the gradient of the query, key and
     value it receives.  It sits OUTSIDE the reference's divide_gradient, so the 1/4, 1/4, 1/2 are in those gradients already;
  2. the module's repeat_kv is replaced by a wrapper that retains the gradient of its outputs: key / value per QUERY head.  Those sit INSIDE
     divide_gradient: their gradients are multiplied by 1/4 and 1/2 here;
  3. a forward pre-hook retains the gradient of every o_proj input.
Frozen (fp64): ids [S], idx, logit;  out, q, k, v [L, nq, S] = sum_d x (*) x.grad per query head and position (out: at the o projection's
input; q / k / v: at the attention function's operands, k / v per query head at the source position);  k_kv, v_kv [L, nk, S]: the same sums
at the kv-head level.  Asserted before anything is written: the group sums of k / v equal k_kv / v_kv; sum_t v[h] = 1/2 sum_t out[h]; in the
top layer q is 0 off the last column."""
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
QWEN_S, QWEN_ISEED = 80, 99
PROTOCOL = ("lxt.efficient.monkey_patch(modeling module), fp64, CPU, eager attention; retain_grad on the operands of eager_attention_forward "
            "(outside divide_gradient), on the outputs of repeat_kv (inside: x 1/4, x 1/2) and on every o_proj input; arg-max logit of the "
            "last position seeded 1")


def wsum(W):
    tot = float(W["embed"].double().abs().sum() + W["lm_head"].double().abs().sum())
    for L in W["layers"]:
        tot += sum(float(v.double().abs().sum()) for v in L.values())
    return tot


def head_maps(mod, model, ids):
    """-> (idx, logit, dict of the frozen maps) of one explanation of `model` (an instance of the already monkey-patched module `mod`)"""
    qkv, reps, oin = [], [], []
    inner, repeat = mod.eager_attention_forward, mod.repeat_kv

    def attention(module, query, key, value, *args, **kw):
        for t in (query, key, value):
            t.retain_grad()
        qkv.append((query, key, value))
        return inner(module, query, key, value, *args, **kw)

    def repeat_kept(x, n_rep):
        y = repeat(x, n_rep)
        if y is x:                                   # (n_rep == 1: the operand itself; a view of its own keeps the two gradients apart)
            y = x.view_as(x)
        y.retain_grad()
        reps.append(y)
        return y

    def keep_in(m, args):
        args[0].retain_grad()
        oin.append(args[0])

    mod.eager_attention_forward, mod.repeat_kv = attention, repeat_kept
    hooks = [L.self_attn.o_proj.register_forward_pre_hook(keep_in) for L in model.model.layers]
    try:
        e = model.get_input_embeddings()(ids[None]).detach().requires_grad_()
        last = model(inputs_embeds=e, use_cache=False).logits[0, -1]
        idx = int(last.argmax())
        last[idx].backward()
    finally:
        mod.eager_attention_forward, mod.repeat_kv = inner, repeat
        for h in hooks:
            h.remove()
    nL, n = len(model.model.layers), ids.numel()
    assert len(qkv) == nL and len(reps) == 2 * nL and len(oin) == nL
    dot = lambda x, f=1.0: (x * x.grad * f)[0].sum(-1).detach()            # noqa: E731  [1, heads, S, d] -> [heads, S]
    nq = qkv[0][0].shape[1]
    out = torch.stack([(o * o.grad)[0].view(n, nq, -1).sum(-1).T for o in oin]).detach()
    maps = dict(out=out, q=torch.stack([dot(q) for q, _, _ in qkv]), k=torch.stack([dot(reps[2 * l], 0.25) for l in range(nL)]),
                v=torch.stack([dot(reps[2 * l + 1], 0.5) for l in range(nL)]), k_kv=torch.stack([dot(k) for _, k, _ in qkv]),
                v_kv=torch.stack([dot(v) for _, _, v in qkv]))
    nk = maps["k_kv"].shape[1]
    grp = lambda m: m.view(nL, nk, nq // nk, n).sum(2)                     # noqa: E731
    e_k, e_v = float((grp(maps["k"]) - maps["k_kv"]).abs().max()), float((grp(maps["v"]) - maps["v_kv"]).abs().max())
    e_h = float((maps["v"].sum(-1) - 0.5 * maps["out"].sum(-1)).abs().max())
    off = float(maps["q"][-1, :, :-1].abs().max())
    print(f"idx {idx} logit {float(last[idx]):+.6f}  group sums k {e_k:.1e} v {e_v:.1e}  sum_t v - 1/2 R_head {e_h:.1e}  "
          f"top-layer q off the last column {off:.1e}  max|out| {float(out.abs().max()):.3e}")
    scale = float(out.abs().max())
    assert e_k <= 1e-12 * scale and e_v <= 1e-12 * scale and e_h <= 1e-12 * scale and off == 0.0
    return idx, float(last[idx]), {k: v.numpy() for k, v in maps.items()}


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
    idx, logit, maps = head_maps(modeling_llama, hf_models.build_llama_from_weights(CFG, W, attn="eager", dtype=torch.float64), ids)
    np.savez_compressed(os.path.join(HERE, "heads_llama.npz"), cfg_keys=np.array(list(CFG.keys())),
                        cfg_vals=np.array([float(v) for v in CFG.values()]), S=S, wseed=WSEED, iseed=ISEED, wsum=wsum(W), ids=ids.numpy(),
                        idx=idx, logit=logit, protocol=np.array(PROTOCOL), **maps)
    monkey_patch(modeling_qwen3)
    ids = torch.randint(0, 256, (QWEN_S,), generator=torch.Generator().manual_seed(QWEN_ISEED))
    idx, logit, maps = head_maps(modeling_qwen3, hf_models.build_qwen3(attn="eager").double(), ids)
    np.savez_compressed(os.path.join(HERE, "heads_qwen3.npz"), S=QWEN_S, iseed=QWEN_ISEED, wsum=hf_models.wsum(hf_models.build_qwen3()),
                        ids=ids.numpy(), idx=idx, logit=logit, protocol=np.array(PROTOCOL), **maps)


if __name__ == "__main__":
    main(*sys.argv[1:2])
