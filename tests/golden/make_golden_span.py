#!/usr/bin/env python3
"""Fixture generator (build container only; imports the REAL reference): span_{llama,qwen3,qwen3_moe}.npz = answer-span explanations of
`lxt.efficient.monkey_patch(modeling module)` run on the CPU in fp64 with eager attention -- what a user of the reference writes as
`f = sum_t w[t] * logits[0, pos[t], tgt[t]]` (or the same over `log_softmax(logits[0, pos[t]])`), `f.backward()`, `(e * e.grad).sum(-1)`.

Models: a seeded Llama at the latent_llama dimensions (oracle.llama.random_weights, make_golden_latent.CFG), the tiny Qwen3 of
qwen_models.py (case qwen3_d128) and the tiny Qwen3-MoE of moe_engine_models.py; a checksum of the weights is stored with each.
Cases, all at S = 48 (key prefix `a/`, `b/`, `c/`, `d/`):
  a  one prompt, T = 3 scattered positions (column 0, a middle one, S - 1), objective logit, weights 1;
  b  the same positions, objective logprob, weights (0.75, 0, -1.5);
  c  two prompts LEFT-padded to S with lengths (48, 31): a contiguous answer at the end of each (5 and 3 tokens, the rows that predict them),
     the shorter one's two spare slots pointed at other valid columns with weight 0; objective logprob.  The reference runs each prompt
     un-padded (RoPE is relative); its rows are placed at the prompt's own columns, pads are 0;
  d  the T single-position explanations of case a (objective logit, weight 1), stacked [T, ...].
Stored per case: ids [B, S], positions / target / weights [B, T], lengths [B], objective, logit / logprob [B, T] (the model's values at every
slot), R_tok [B, S], layer_R [L + 1, B] = sum (h * h.grad) at the embedding (index 0) and at every decoder layer's output; for case a on
Llama also R_head_out [L, B, nq, S] = sum_d (o * o.grad) per query head at the o projection's input.  Targets are the next token of the
prompt (teacher forcing) and the row's arg-max at column S - 1.
The whole pass is fp64 (all_fp64 below: HF's eager softmax and the reference's RMSNorm patch otherwise compute in fp32 whatever the dtype).
The generator asserts linearity on the reference itself: case a's R_tok equals the sum of case d's rows to 1e-10 (normalised max)."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")

S = 48
POS_A = (0, 17, S - 1)
W_B = (0.75, 0.0, -1.5)
LENGTHS_C = (48, 31)
POS_C = ((42, 43, 44, 45, 46), (44, 45, 46, 20, 33))
W_C = ((1.0, 1.0, 1.0, 1.0, 1.0), (1.0, 1.0, 1.0, 0.0, 0.0))
PROTOCOL = ("lxt.efficient.monkey_patch(modeling module), fp64, CPU, eager attention; f = sum_t w_t logits[0, p_t, tgt_t] (logit) or "
            "sum_t w_t log_softmax(logits[0, p_t])[tgt_t] (logprob); f.backward(); hooks on decoder-layer outputs, the input embedding and "
            "o_proj inputs; padded prompts run un-padded")


def explain(model, ids, pos, tgt, w, objective, heads=False):
    """one prompt ids [n]; pos / tgt / w lists of T (tgt entries None: next token, arg-max at the last column) -> dict of fp64 results"""
    outs, oins = [], []

    def keep_out(mod, args, out):
        h = out[0] if isinstance(out, tuple) else out
        h.retain_grad()
        outs.append(h)

    def keep_in(mod, args):
        args[0].retain_grad()
        oins.append(args[0])

    hooks = [L.register_forward_hook(keep_out) for L in model.model.layers]
    if heads:
        hooks += [L.self_attn.o_proj.register_forward_pre_hook(keep_in) for L in model.model.layers]
    e = model.get_input_embeddings()(ids[None]).detach().requires_grad_()
    logits = model(inputs_embeds=e, use_cache=False).logits[0]
    for h in hooks:
        h.remove()
    n = ids.numel()
    tgt = [int(ids[p + 1]) if t is None and p < n - 1 else int(logits[p].argmax()) if t is None else int(t) for p, t in zip(pos, tgt)]
    lp = torch.log_softmax(logits, -1)
    src = logits if objective == "logit" else lp
    f = sum(float(wt) * src[p, t] for p, t, wt in zip(pos, tgt, w))
    model.zero_grad()
    f.backward()
    hs = [e] + outs
    res = dict(target=tgt, logit=[float(logits[p, t]) for p, t in zip(pos, tgt)], logprob=[float(lp[p, t]) for p, t in zip(pos, tgt)],
               R_tok=(e * e.grad)[0].sum(-1).detach(),
               layer_R=torch.stack([(h * h.grad).sum() if h.grad is not None else torch.zeros((), dtype=h.dtype) for h in hs]).detach())
    if heads:
        nq = model.config.num_attention_heads
        res["R_head_out"] = torch.stack([(o * o.grad)[0].view(n, nq, -1).sum(-1).T for o in oins]).detach()       # [L, nq, n]
    return res


def run_case(model, ids, lengths, positions, weights, objective, heads=False):
    """ids [B, S] left-padded to S by lengths -> the stored arrays of one case"""
    B, T = len(positions), len(positions[0])
    out = dict(ids=ids.numpy(), lengths=np.asarray(lengths), positions=np.asarray(positions), weights=np.asarray(weights, dtype=np.float64),
               objective=np.array(objective))
    per = []
    for b in range(B):
        off = S - lengths[b]
        per.append(explain(model, ids[b, off:], [p - off for p in positions[b]], [None] * T, weights[b], objective, heads))
    L1 = per[0]["layer_R"].numel()
    R_tok, layer_R = torch.zeros(B, S, dtype=torch.float64), torch.zeros(L1, B, dtype=torch.float64)
    for b, r in enumerate(per):
        R_tok[b, S - lengths[b]:] = r["R_tok"]
        layer_R[:, b] = r["layer_R"]
    out.update(target=np.asarray([r["target"] for r in per]), logit=np.asarray([r["logit"] for r in per]),
               logprob=np.asarray([r["logprob"] for r in per]), R_tok=R_tok.numpy(), layer_R=layer_R.numpy())
    if heads:
        assert B == 1 and lengths[0] == S
        out["R_head_out"] = per[0]["R_head_out"][:, None].numpy()
    return out


def nmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def model_cases(name, model, vocab, iseed, heads):
    g = torch.Generator().manual_seed(iseed)
    ids = torch.randint(0, vocab, (1, S), generator=g)
    ids_c = torch.randint(0, vocab, (2, S), generator=g)
    for b, n in enumerate(LENGTHS_C):
        ids_c[b, : S - n] = 0
    ones = (1.0,) * len(POS_A)
    a = run_case(model, ids, (S,), (POS_A,), (ones,), "logit", heads)
    b = run_case(model, ids, (S,), (POS_A,), (W_B,), "logprob")
    c = run_case(model, ids_c, LENGTHS_C, POS_C, W_C, "logprob")
    singles = [run_case(model, ids, (S,), ((p,),), ((1.0,),), "logit") for p in POS_A]
    d = {k: np.stack([s[k] for s in singles]) for k in singles[0]}
    lin = nmax(sum(s["R_tok"] for s in singles), a["R_tok"])
    lin_l = nmax(sum(s["layer_R"] for s in singles), a["layer_R"])
    print(f"[{name}] a: target {a['target'].tolist()} logit {a['logit'].round(4).tolist()} sum R_tok {a['R_tok'].sum():+.6f} "
          f"layer_R[L] {a['layer_R'][-1].tolist()}; linearity sum_t d vs a: R_tok {lin:.1e} layer_R {lin_l:.1e}; "
          f"c: logprob {c['logprob'].round(3).tolist()} max|R_tok| {np.abs(c['R_tok']).max():.3e}")
    assert lin <= 1e-10 and lin_l <= 1e-10, (lin, lin_l)
    assert [int(singles[t]["target"][0, 0]) for t in range(len(POS_A))] == a["target"][0].tolist() == b["target"][0].tolist()
    out = {}
    for key, case in (("a", a), ("b", b), ("c", c), ("d", d)):
        out.update({f"{key}/{k}": v for k, v in case.items()})
    return out


class Fp64Torch:
    """`torch` as the reference's patches module sees it during this run: float32 names float64, everything else is torch's"""
    float32 = torch.float64

    def __getattr__(self, name):
        return getattr(torch, name)


def all_fp64():
    """Two places compute in fp32 whatever the model's dtype, so that a "fp64" run rounds activations AND the gradients through them to fp32
    (measured: linearity of the backward in its seed then holds to 5e-8 only): HF's eager attention and the MoE router ask for
    `softmax(..., dtype=torch.float32)`, and the reference's RMSNorm patch casts its input `.to(torch.float32)`.  For this run an fp64 input
    keeps its dtype in both: the softmax request is dropped, and the reference's patches module reads float64 for the name float32.  The
    rules themselves are untouched: the fixtures are the reference's rules in fp64 throughout"""
    import lxt.efficient.patches as patches
    patches.torch = Fp64Torch()
    F = torch.nn.functional
    orig = F.softmax

    def softmax(x, dim=None, _stacklevel=3, dtype=None):
        return orig(x, dim=dim, dtype=None if x.dtype == torch.float64 else dtype)

    F.softmax = softmax


def main(reference=os.environ.get("LXT_REFERENCE", "")):
    if reference:
        sys.path.insert(0, reference)
    all_fp64()
    from lxt.efficient import monkey_patch
    from transformers.models.llama import modeling_llama
    from transformers.models.qwen3 import modeling_qwen3
    from transformers.models.qwen3_moe import modeling_qwen3_moe
    from oracle import llama as ol
    from tests.golden import moe_engine_models, qwen_models
    from tests.golden.hf_models import build_llama_from_weights
    from tests.golden.make_golden_latent import CFG, WSEED, wsum
    for mod in (modeling_llama, modeling_qwen3, modeling_qwen3_moe):
        monkey_patch(mod)
    W = ol.random_weights(CFG, seed=WSEED)
    jobs = (("llama", lambda: build_llama_from_weights(CFG, W, attn="eager", dtype=torch.float64), CFG["vocab"], wsum(W), 31, True),
            ("qwen3", lambda: qwen_models.build("qwen3_d128").double(), qwen_models.VOCAB, None, 32, False),
            ("qwen3_moe", lambda: moe_engine_models.build().double(), 256, None, 33, False))
    for name, make, vocab, ws, iseed, heads in jobs:
        model = make()
        ws = qwen_models.wsum(model) if ws is None else ws
        np.savez_compressed(os.path.join(HERE, f"span_{name}.npz"), S=S, wsum=ws, iseed=iseed, protocol=np.array(PROTOCOL),
                            **model_cases(name, model, vocab, iseed, heads))


if __name__ == "__main__":
    main(*sys.argv[1:2])
