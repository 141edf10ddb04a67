#!/usr/bin/env python3
"""Fixture generator (build container only; imports the REAL reference): every read-out of Gemma3LRP.explain / Gemma3MMLRP.explain -- layer,
latent, per-head and token-to-token -- from `lxt.efficient.monkey_patch(modeling_gemma3)` (ref lxt/efficient/models/gemma3.py:11-19,
lxt/efficient/patches.py:193-203) run on the CPU in fp64, eager attention, the arg-max logit of the last position seeded with 1.
  gemma3_readouts_tiny.npz: tests.golden.hf_models.build_gemma3() (3 sliding layers of window 32 + 1 global, 4 + 2 heads of 32), S 80;
  gemma3_readouts_d256.npz: gemma3_readout_models.build_gemma3_d256() (sliding, sliding, full; window 48; 4 + 2 heads of 256), S 136;
  gemma3_mm_readouts.npz:   hf_models.build_gemma3_mm() with gemma3_mm_inputs() (image + text): the `out` heads and the "sum" map of the text
                            layers (the SigLIP tower under attn_implementation "eager": its attention keeps plain gradients).

Protocol: the three protocols of make_golden_latent.py, make_golden_heads.py and make_golden_attn_map.py in ONE run --
  forward hooks + retain_grad on every decoder layer's output and on the input embedding, a forward pre-hook + retain_grad on every
  mlp.down_proj and o_proj input; eager_attention_forward wrapped outside the reference's divide_gradient (query, key, value retained: the
  1/4, 1/4, 1/2 are in those gradients), repeat_kv wrapped inside it (key / value per QUERY head: x 1/4, x 1/2 here); the functional dropout
  call inside eager_attention_forward retains the probabilities (rate 0: the identity).
Frozen: ids, idx, logit;  trace [L+1, S], resid [L+1, H], mlp [L, I] (boundary 0: the decoder's input -- the word embeddings, with the image
features scattered in on an image + text prompt);  out, q, k, v [L, nq, S];  total [L, S, S] fp64 and per_head
[len(head_layers), nq, S, S] float32;  window, layer_sliding [L].  d256 also: gap_bf16/<output> = the normalised max error of the reference's
OWN bf16 run of this instance (rotary inv_freq kept fp32, target = idx) against its fp64 run, for every output above and for layer_R; per_head
holds one gap per (layer, head), each map normalised by its own largest value.
Asserted before anything is written (1e-12 of the largest value unless said): the rows of every head's map sum to `out`; the map equals
P (*) (G_o V^T); it is 0 above the diagonal (text prompts) and 0 outside the window on sliding layers; in the top layer only the last row is
live; the group sums of k / v equal the kv-head level sums; sum_t v = 1/2 sum_t out; resid and trace sum to the same per boundary; each file
stays under the size limit of a committed file (else: fewer head_layers, never a smaller S)."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")

TINY_S, TINY_ISEED = 80, 77
MAX_BYTES = 1 << 20
PROTOCOL = ("lxt.efficient.monkey_patch(modeling_gemma3), fp64, CPU, eager attention; hooks + retain_grad on decoder-layer outputs, the input "
            "embedding, mlp.down_proj and o_proj inputs, the operands of eager_attention_forward (outside divide_gradient), the outputs of "
            "repeat_kv (inside: x 1/4, x 1/2) and the probabilities (the input of the functional dropout call); map = P * P.grad; arg-max "
            "logit of the last position seeded 1")


def text_model(model):
    m = model.model
    return getattr(m, "language_model", m)


def readouts(mod, model, run, S, target=None):
    """one explanation of `model` (an instance of the already monkey-patched module `mod`); run(e) -> logits [1, S, V] from the input
    embeddings e.  -> (idx, logit, dict of fp64 / model-dtype tensors, the retained (P, q, k, v, rep) per layer)"""
    layers = text_model(model).layers
    outs, mids, oin, qkv, reps, probs = [], [], [], [], [], []
    F = torch.nn.functional
    inner, repeat, dropout = mod.eager_attention_forward, mod.repeat_kv, F.dropout

    def attention(module, query, key, value, *args, **kw):
        for t in (query, key, value):
            t.retain_grad()
        qkv.append((query, key, value, module.num_key_value_groups, module.scaling))
        return inner(module, query, key, value, *args, **kw)

    def repeat_kept(x, n_rep):
        y = repeat(x, n_rep)
        if y is x:
            y = x.view_as(x)
        y.retain_grad()
        reps.append(y)
        return y

    def dropout_kept(x, *args, **kw):
        if x.dim() == 4 and x.shape[-1] == x.shape[-2] == S:          # (the text decoder's probabilities [1, nq, S, S]; nothing else has that shape)
            x.retain_grad()
            probs.append(x)
        return dropout(x, *args, **kw)

    def keep_out(m, args, out):
        h = out[0] if isinstance(out, tuple) else out
        h.retain_grad()
        outs.append(h)

    def keep(lst):
        def hook(m, args):
            args[0].retain_grad()
            lst.append(args[0])
        return hook

    mod.eager_attention_forward, mod.repeat_kv, F.dropout = attention, repeat_kept, dropout_kept
    dec_in = []

    def keep_decoder_input(m, args, kwargs):          # (image + text: the word embeddings with the image features scattered in, not a leaf)
        x = kwargs.get("inputs_embeds")
        if x is not None and x.requires_grad:
            x.retain_grad()
            dec_in.append(x)

    hooks = [L.register_forward_hook(keep_out) for L in layers] + [text_model(model).register_forward_pre_hook(keep_decoder_input, with_kwargs=True)]
    hooks += [L.mlp.down_proj.register_forward_pre_hook(keep(mids)) for L in layers]
    hooks += [L.self_attn.o_proj.register_forward_pre_hook(keep(oin)) for L in layers]
    try:
        e, logits = run()
        last = logits[0, -1]
        idx = int(last.argmax()) if target is None else target
        last[idx].backward()
    finally:
        mod.eager_attention_forward, mod.repeat_kv, F.dropout = inner, repeat, dropout
        for h in hooks:
            h.remove()
    nL = len(layers)
    assert len(outs) == nL and len(mids) == nL and len(oin) == nL and len(qkv) == nL and len(reps) == 2 * nL and len(probs) == nL
    nq = qkv[0][0].shape[1]
    assert len(dec_in) == 1
    hs = [dec_in[0]] + outs          # boundary 0: the decoder's input
    dot = lambda x, f=1.0: (x * x.grad * f)[0].sum(-1).detach()            # noqa: E731  [1, heads, S, d] -> [heads, S]
    r = dict(trace=torch.stack([(h * h.grad)[0].sum(-1) for h in hs]), resid=torch.stack([(h * h.grad)[0].sum(0) for h in hs]),
             mlp=torch.stack([(m * m.grad)[0].sum(0) for m in mids]),
             out=torch.stack([(o * o.grad)[0].view(S, nq, -1).sum(-1).T for o in oin]),
             q=torch.stack([dot(q) for q, *_ in qkv]), k=torch.stack([dot(reps[2 * l], 0.25) for l in range(nL)]),
             v=torch.stack([dot(reps[2 * l + 1], 0.5) for l in range(nL)]), k_kv=torch.stack([dot(x[1]) for x in qkv]),
             v_kv=torch.stack([dot(x[2]) for x in qkv]), maps=torch.stack([(P * P.grad)[0] for P in probs]))
    r = {k: t.detach() for k, t in r.items()}
    return idx, float(last[idx]), r, (probs, qkv, oin)


def check(r, kept, sliding, window, causal=True):
    """the identities of the docstring, on the fp64 run"""
    probs, qkv, oin = kept
    maps, out = r["maps"], r["out"]
    nL, nq, S = out.shape
    nk = r["k_kv"].shape[1]
    scale, hscale = float(maps.abs().max()), float(out.abs().max())
    e_row = float((maps.sum(-1) - out).abs().max())
    e_gp = 0.0
    for l, (P, (q, k, v, rep_, _), o) in enumerate(zip(probs, qkv, oin)):
        vr = v.detach().repeat_interleave(rep_, 1)[0]
        go = o.grad[0].view(S, nq, -1).permute(1, 0, 2)
        e_gp = max(e_gp, float((maps[l] - P.detach()[0] * (go @ vr.transpose(1, 2))).abs().max()))
    i = torch.arange(S)
    upper = float(maps.triu(1).abs().max()) if causal else 0.0
    outside = (i[None, :] <= i[:, None] - window)                          # HF: a sliding layer sees keys with i - j < window
    e_win = max([float(maps[l][:, outside].abs().max()) for l in range(nL) if sliding[l]] + [0.0]) if causal else 0.0
    bites = any(sliding) and bool(outside.any())
    top_off = float(maps[-1, :, :-1].abs().max())
    grp = lambda m: m.view(nL, nk, nq // nk, S).sum(2)                     # noqa: E731
    e_k, e_v = float((grp(r["k"]) - r["k_kv"]).abs().max()), float((grp(r["v"]) - r["v_kv"]).abs().max())
    e_h = float((r["v"].sum(-1) - 0.5 * out.sum(-1)).abs().max())
    e_tr = float((r["resid"].sum(-1) - r["trace"].sum(-1)).abs().max())
    q_off = float(r["q"][-1, :, :-1].abs().max())
    print(f"  max|map| {scale:.3e}  row sums - out {e_row:.1e}  map - P (G_o V^T) {e_gp:.1e}  above the diagonal {upper:.1e}  outside the "
          f"window {e_win:.1e} (window bites: {bites})  top layer off the last row {top_off:.1e}\n  group sums k {e_k:.1e} v {e_v:.1e}  "
          f"sum_t v - 1/2 R_head {e_h:.1e}  resid - trace sums {e_tr:.1e}  top-layer q off the last column {q_off:.1e}")
    assert e_row <= 1e-12 * scale and e_gp <= 1e-12 * scale and upper == 0.0 and e_win == 0.0 and top_off == 0.0 and q_off == 0.0
    assert e_k <= 1e-12 * hscale and e_v <= 1e-12 * hscale and e_h <= 1e-12 * hscale and e_tr <= 1e-12 * float(r["trace"].abs().max())
    assert float(maps[-1, :, -1].abs().max()) > 0
    return bites


def arrays(r, head_layers, names):
    a = {k: r[k].double().numpy() for k in names if k != "maps"}
    if "maps" in names:
        a["total"] = r["maps"].double().sum(1).numpy()
        a["per_head"] = r["maps"][head_layers].float().numpy()
        a["head_layers"] = np.asarray(head_layers)
    return a


def save(name, **a):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, protocol=np.array(PROTOCOL), **a)
    print(f"{name}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) <= MAX_BYTES, "over the size limit of a committed file: store per-head maps of fewer layers"


ALL = ("trace", "resid", "mlp", "out", "q", "k", "v", "k_kv", "v_kv", "maps")


def nmax(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def text_case(mod, build, ids, bf16=None):
    model = build().double()
    for p in model.parameters():
        p.requires_grad_(False)
    S = ids.numel()

    def run(m):
        def go():
            e = m.get_input_embeddings()(ids[None]).detach().requires_grad_()
            return e, m(inputs_embeds=e, use_cache=False).logits
        return go
    idx, logit, r, kept = readouts(mod, model, run(model), S)
    cfg = model.config
    sliding = [t == "sliding_attention" for t in cfg.layer_types]
    print(f"idx {idx} logit {logit:+.6f}")
    assert check(r, kept, sliding, int(cfg.sliding_window)), "the window does not bite: S is too small"
    extra = {}
    if bf16 is not None:
        mb = bf16(build())
        for p in mb.parameters():
            p.requires_grad_(False)
        _, lb, rb, _ = readouts(mod, mb, run(mb), S, target=idx)
        rb["total"], r["total"] = rb["maps"].double().sum(1), r["maps"].sum(1)
        rb["per_head"], r["per_head"] = rb["maps"], r["maps"]
        rb["layer_R"], r["layer_R"] = rb["trace"].double().sum(-1), r["trace"].sum(-1)
        for k in ("trace", "resid", "mlp", "out", "q", "k", "v", "total", "layer_R"):
            extra["gap_bf16/" + k] = nmax(rb[k], r[k])
        nL, nq = r["maps"].shape[:2]          # every head's map is an output of its own (R_attn_heads[n]): one gap per (layer, head)
        extra["gap_bf16/per_head"] = np.array([[nmax(rb["maps"][l, h], r["maps"][l, h]) for h in range(nq)] for l in range(nL)])
        extra["logit_bf16"] = lb
        print("  the reference's own bf16 against its fp64: " + "  ".join(f"{k.split('/')[1]} {np.max(v):.2e}" for k, v in extra.items() if "/" in k))
    return dict(ids=ids.numpy(), idx=idx, logit=logit, S=S, window=int(cfg.sliding_window), layer_sliding=np.array(sliding), **extra), r


def main(reference=os.environ.get("LXT_REFERENCE", "")):
    if reference:
        sys.path.insert(0, reference)
    from lxt.efficient import monkey_patch
    from transformers.models.gemma3 import modeling_gemma3
    from tests.golden import hf_models
    from tests.golden import gemma3_readout_models as gm
    monkey_patch(modeling_gemma3)
    ids = torch.randint(0, 512, (TINY_S,), generator=torch.Generator().manual_seed(TINY_ISEED))
    meta, r = text_case(modeling_gemma3, lambda: hf_models.build_gemma3(attn="eager"), ids)
    save("gemma3_readouts_tiny.npz", wsum=hf_models.wsum(hf_models.build_gemma3()), iseed=TINY_ISEED, **meta, **arrays(r, [0, 1, 2, 3], ALL))
    meta, r = text_case(modeling_gemma3, lambda: gm.build_gemma3_d256(attn="eager"), gm.d256_ids(), bf16=gm.to_bf16_rotary_fp32)
    save("gemma3_readouts_d256.npz", wsum=hf_models.wsum(gm.build_gemma3_d256()), iseed=gm.D256_ISEED, **meta, **arrays(r, [0, 1, 2], ALL))
    # image + text: the whole image block attends in both directions, so "above the diagonal" is not checked (causal=False)
    model = hf_models.build_gemma3_mm(attn="eager").double()
    for p in model.parameters():
        p.requires_grad_(False)
    ids, tt, pv = hf_models.gemma3_mm_inputs()

    def run():
        e = model.get_input_embeddings()(ids).detach().requires_grad_()
        return e, model(inputs_embeds=e, pixel_values=pv.double(), token_type_ids=tt, use_cache=False).logits
    idx, logit, r, kept = readouts(modeling_gemma3, model, run, ids.shape[1])
    print(f"idx {idx} logit {logit:+.6f}")
    tc = model.config.text_config
    check(r, kept, [t == "sliding_attention" for t in tc.layer_types], int(tc.sliding_window), causal=False)
    img = tt[0].bool()
    assert float(r["maps"][:, :, img][:, :, :, img].triu(1).abs().max()) > 0, "no image row looks ahead inside its block"
    a = arrays(r, [], ("out", "maps"))
    save("gemma3_mm_readouts.npz", wsum=hf_models.wsum(hf_models.build_gemma3_mm()), ids=ids.numpy(), token_type_ids=tt.numpy(), idx=idx,
         logit=logit, S=ids.shape[1], layer_R=r["trace"].sum(-1).numpy(), out=a["out"], total=a["total"])


if __name__ == "__main__":
    main(*sys.argv[1:2])
