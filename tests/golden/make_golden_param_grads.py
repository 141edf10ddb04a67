#!/usr/bin/env python3
"""Fixture generator (build container only; imports the REAL reference): the plain parameter gradients `p.grad` that
`lxt.efficient.monkey_patch` leaves on a model whose parameters all require grad -- run on the CPU in fp64, eager attention, the arg-max logit
of the last position (BERT: the arg-max class logit) seeded with 1.  Stored as fp32; `p * p.grad` is the parameter's relevance.

    python tests/golden/make_golden_param_grads.py [family ...]        (one process per family: the reference's patches are process-global)

Every file holds ids, idx, logit, wsum, protocol, one array "g:<parameter name>" per kept parameter and `zero`: the names of kept parameters
whose gradient is zero in exact arithmetic (BERT's key biases), which carry no array.  A committed file stays under 1 MiB, so:
  param_grads_llama.npz   the seeded Llama of make_golden_weight_relevance.py (same CFG / WSEED / id seeds: weight_relevance_llama_* describe the
                          same model and pin its Linears); the NORM weights only -- per prompt ("p0:", "p1:") and summed over the two prompts
                          ("g:"), as two explanations without zero_grad leave them.
  param_grads_qwen2.npz   tests.golden.hf_models.build_qwen2 (q / k / v biases), param_grads_qwen3.npz build_qwen3 (per-head q / k norms),
  param_grads_gemma3.npz  build_gemma3 ((1 + w) norms; norm weights re-seeded, HF initialises them to zero), param_grads_gpt2.npz build_gpt2
                          (Conv1D weights in their stored [in, out] layout, LayerNorms, biases): EVERY vector parameter and the matrices of the
                          FIRST decoder layer; the matrices of the LAST layer go to param_grads_<family>_top.npz (the two layers together are
                          over 1 MiB).  Embeddings, the head and the middle layers' matrices are not kept.
  param_grads_bert.npz    build_bert (BERT-base: one 768 x 768 matrix alone is over 1 MiB): EVERY vector parameter (LayerNorm weights and
                          biases, Linear biases) and the classifier weight [2, 768]; the rules are the reference's primitives spliced into HF's
                          modeling_bert as in make_golden_hf.py (the reference's vendored BERT does not run under transformers 5.x)."""
import os
import subprocess
import sys
import warnings
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")

from tests.golden import hf_models                                      # noqa: E402
from tests.golden.make_golden_weight_relevance import CFG, S, WSEED, ISEEDS      # noqa: E402

PROTOCOL = ("lxt.efficient.monkey_patch(modeling module), every parameter requires_grad, fp64, CPU, eager attention; arg-max logit of the last "
            "position (BERT: arg-max class logit) seeded 1; p.grad after logit.backward()")
FAMILY_IDS = dict(qwen2=(256, 48, 41), qwen3=(256, 48, 42), gemma3=(512, 48, 43), gpt2=(256, 48, 44), bert=(30522, 128, 1234))     # vocab, S, seed
LIMIT = 1 << 20


def seed_norms(model, seed):
    """Gemma's (1 + w) norm weights start at zero: seeded values, so w * w.grad is not trivially zero (shared with the GPU test)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "norm" in n:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return model


def build(family, attn="eager"):
    """the seeded fp32 model of a family, every parameter trainable (the GPU test builds its models here too)"""
    if family == "llama":
        from oracle import llama as ol
        m = hf_models.build_llama_from_weights(CFG, ol.random_weights(CFG, seed=WSEED), attn=attn)
    elif family == "gemma3":
        m = seed_norms(hf_models.build_gemma3(attn=attn), 103)
    else:
        m = getattr(hf_models, f"build_{family}")(attn=attn)
    for p in m.parameters():
        p.requires_grad_(True)
    return m


def family_ids(family):
    if family == "llama":
        return torch.stack([torch.randint(0, CFG["vocab"], (S,), generator=torch.Generator().manual_seed(s)) for s in ISEEDS])
    vocab, n, seed = FAMILY_IDS[family]
    return torch.randint(0, vocab, (1, n), generator=torch.Generator().manual_seed(seed))


def explain(model, ids, zero=True):
    """one explanation of one prompt -> (idx, logit); the gradients stay on the parameters"""
    if zero:
        model.zero_grad(set_to_none=True)
    e = model.get_input_embeddings()(ids[None])            # (not detached: the embedding table gets its gradient too)
    out = model(inputs_embeds=e, use_cache=False) if hasattr(model, "lm_head") else model(inputs_embeds=e)
    last = out.logits[0, -1] if out.logits.dim() == 3 else out.logits[0]
    idx = int(last.argmax())
    last[idx].backward()
    return idx, float(last[idx])


def layer_index(name):
    for part in name.split("."):
        if part.isdigit():
            return int(part)
    return None


def kept(family, model):
    """-> (names of the main file, names of the _top file)"""
    named = dict(model.named_parameters())
    if family == "llama":
        return [n for n in named if "norm" in n], []
    vec = [n for n, p in named.items() if p.dim() == 1]
    if family == "bert":
        return vec + ["classifier.weight"], []
    top = max(layer_index(n) for n in named if layer_index(n) is not None)
    mats = lambda l: [n for n, p in named.items() if p.dim() == 2 and layer_index(n) == l]          # noqa: E731
    return vec + mats(0), mats(top)


def patch_reference(family):
    from lxt.efficient import monkey_patch
    import importlib
    mod = importlib.import_module(f"transformers.models.{family}.modeling_{family}")
    if family != "bert":
        return monkey_patch(mod)
    import lxt.efficient.patches as lp
    from lxt.efficient.rules import identity_rule_implicit
    from transformers.models.bert.modeling_bert import BertIntermediate, BertPooler

    def inter_fwd(self, h):
        return identity_rule_implicit(self.intermediate_act_fn, self.dense(h))

    def pool_fwd(self, h):
        return identity_rule_implicit(self.activation, self.dense(h[:, 0]))
    monkey_patch(mod, {torch.nn.LayerNorm: partial(lp.patch_method, lp.layer_norm_forward),
                       torch.nn.Dropout: partial(lp.patch_method, lp.dropout_forward),
                       BertIntermediate: partial(lp.patch_method, inter_fwd), BertPooler: partial(lp.patch_method, pool_fwd),
                       mod: lp.patch_attention})


def save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"  {name}: {len(arrays)} arrays, {size} bytes")
    assert size < LIMIT, f"{name} is over 1 MiB"


def main(family, reference=os.environ.get("LXT_REFERENCE", "")):
    if reference:
        sys.path.insert(0, reference)
    torch.set_num_threads(8)
    patch_reference(family)
    model32 = build(family)
    ws = hf_models.wsum(model32)
    model = model32.double()
    ids = family_ids(family)
    main_names, top_names = kept(family, model)
    named = dict(model.named_parameters())
    f32 = lambda t: t.detach().to(torch.float32).numpy()               # noqa: E731
    meta = dict(ids=ids.numpy(), protocol=np.array(PROTOCOL), wsum=ws)
    if family == "llama":
        res, per = [], []
        for row in ids:
            res.append(explain(model, row))
            per.append({n: named[n].grad.clone() for n in main_names})
        arrays = {f"p{i}:{n}": f32(g[n]) for i, g in enumerate(per) for n in main_names}
        arrays.update({f"g:{n}": f32(per[0][n] + per[1][n]) for n in main_names})
        save("param_grads_llama.npz", **meta, idx=np.array([r[0] for r in res]), logit=np.array([r[1] for r in res]), wseed=WSEED,
             iseeds=np.array(ISEEDS), **arrays)
        return
    idx, logit = explain(model, ids[0])
    missing = [n for n, p in named.items() if p.grad is None]
    assert not missing, missing
    print(f"  [{family}] idx={idx} logit={logit:.6f}  {len(main_names)} + {len(top_names)} parameters kept of {len(named)}")
    # a gradient that is zero in exact arithmetic (BERT's key biases: softmax is invariant to a shift of a row's scores) comes out of fp64
    # as noise ~1e-16 of its siblings; it has no scale of its own to normalise an error by, so it is recorded by NAME only ("zero")
    scale = max(float(named[n].grad.abs().max()) for n in main_names)
    zero = [n for n in main_names if float(named[n].grad.abs().max()) < 1e-10 * scale]
    main_names = [n for n in main_names if n not in zero]
    print(f"  [{family}] gradients that are zero in exact arithmetic: {zero}")
    meta.update(idx=idx, logit=logit, zero=np.array(zero, dtype=str))
    save(f"param_grads_{family}.npz", **meta, **{f"g:{n}": f32(named[n].grad) for n in main_names})
    if top_names:
        save(f"param_grads_{family}_top.npz", **meta, **{f"g:{n}": f32(named[n].grad) for n in top_names})


if __name__ == "__main__":
    fams = sys.argv[1:] or ["llama", "qwen2", "qwen3", "gemma3", "bert", "gpt2"]
    if len(fams) == 1:
        main(fams[0])
    else:
        for f in fams:
            subprocess.run([sys.executable, os.path.abspath(__file__), f], check=True)
