"""Whole-model AttnLRP engine for Llama-style decoders: fused forward + LRP backward on the HIP
kernels, one call per batch of prompts.

This is the hot path named by BASELINE.json: it reproduces the user protocol of the reference
(docs/source/quickstart.rst:120-141; examples/paper/llama.py:27-46 --  embed ids -> forward ->
pick max(logits[0,-1]) -> seed the backward -> sum_h emb (*) grad) with the rule placement of
lxt/efficient/models/llama.py:9-14 (mode="efficient") or of the explicit composite
lxt/explicit/models/llama.py:83-93,226-260,273-281,379-391,481-488 (mode="explicit").

MI355X-first decisions:
  * everything an eps-rule needs (every Linear output z, pre/post-RoPE q/k, attention o + lse,
    residual sums) is STASHED in HBM during the forward (~0.3 GB/layer at S=2048 bf16; 288 GB
    available) -- the backward never recomputes a GEMM, it runs one dgrad GEMM per Linear;
  * every weight is kept ONCE, in its forward layout W [out,in] (QKV and gate+up fused along the output dim; gate / up rows interleaved
    in blocks of 32 so that the gated-MLP rules run inside the GEMM epilogues): the forward is an NT
    GEMM, the backward the NN form  c = s W  of the same kernel (the transposed MFMA operand is gathered in LDS by
    ds_read_b64_tr_b16); only the fp32 parity engine falls back to a W^T copy (ops.linear_dgrad);
  * bf16 / head_dim 128 attention reads its transposed operands out of row-major LDS tiles as well; fp32 and the other head dims keep
    head-transposed copies of q/k/v/Gho (attention.hip, `attn_t`);
  * only the last token's logits are formed (the explained logit lives there), and the LM head
    + final norm backward is a single row per prompt; explain(positions=...) forms and seeds the T explained rows of each prompt
    instead (answer-span attribution): still one forward and one backward;
  * explain() keeps no KV cache (it needs every activation of the forward); generate(), forward only, has one and produces the model's own
    answer on the same resident weights for explain_generated() to explain.
Python only sequences kernel launches on the current stream; it performs no arithmetic.
"""
import collections
import math
import operator

import torch

from . import ops
from .engine_cp import cp_layer_bwd, cp_request

EXPLICIT = dict(lin=1e-8, add=1e-8, qk=1e-8, mask=1e-8, pv=1e-6, rope=1e-8, act=None)
EFFICIENT = dict(lin=0.0, add=0.0, qk=0.0, mask=0.0, pv=0.0, rope=0.0, act=1e-10)


_STATIC_ROPE = ("default", "linear", "llama3", "yarn")


def rope_kind(hf_cfg):
    """rope type of a HF config: transformers 5 keeps it in `rope_parameters`, transformers 4.x in `rope_scaling` (key 'rope_type', legacy
    key 'type') next to `rope_theta` -- Llama-3.1 / 3.2 there carry {'rope_type': 'llama3', ...}, which must not be dropped silently"""
    rp = getattr(hf_cfg, "rope_parameters", None)
    if isinstance(rp, dict):
        return rp.get("rope_type", rp.get("type", "default"))
    rs = getattr(hf_cfg, "rope_scaling", None)
    if rs is None:
        return "default"
    if isinstance(rs, dict) and (rs.get("rope_type") or rs.get("type")):
        return rs.get("rope_type") or rs.get("type")
    raise NotImplementedError(f"LlamaLRP: cannot interpret rope_scaling={rs!r}")


def config_from_hf(hf_cfg):
    """HF LlamaConfig -> engine cfg.  Everything the fused driver does not implement is refused LOUDLY here instead of
    being ignored: other model types (use lxt_amd.efficient.monkey_patch for those), attention / MLP biases, and rope
    types whose frequencies depend on the running sequence length ("dynamic", "longrope").  The rotary frequencies and
    the cos/sin post-scale are taken from HF's own initialiser for the config's rope_type (Llama-3.1/3.2: "llama3"),
    exactly what LlamaRotaryEmbedding.__init__ does -- the reference inherits them from HF unchanged."""
    mt = getattr(hf_cfg, "model_type", "llama")
    if mt != "llama":
        raise NotImplementedError(f"LlamaLRP drives Llama-architecture decoders only (model_type={mt!r}); "
                                  "other families run through lxt_amd.efficient.monkey_patch")
    if getattr(hf_cfg, "attention_bias", False) or getattr(hf_cfg, "mlp_bias", False):
        raise NotImplementedError("LlamaLRP: attention_bias / mlp_bias = True are not supported by the fused driver "
                                  "(use the monkey_patch drop-in path)")
    hd = getattr(hf_cfg, "head_dim", None) or hf_cfg.hidden_size // hf_cfg.num_attention_heads
    theta = None
    rp = getattr(hf_cfg, "rope_parameters", None)
    if isinstance(rp, dict):
        theta = rp.get("rope_theta")
    if theta is None:
        theta = getattr(hf_cfg, "rope_theta", 10000.0)
    cfg = dict(hidden=hf_cfg.hidden_size, inter=hf_cfg.intermediate_size, n_layers=hf_cfg.num_hidden_layers,
               n_heads=hf_cfg.num_attention_heads, n_kv=hf_cfg.num_key_value_heads, head_dim=hd,
               vocab=hf_cfg.vocab_size, rope_theta=float(theta), rms_eps=float(hf_cfg.rms_norm_eps),
               act=getattr(hf_cfg, "hidden_act", "silu"))
    kind = rope_kind(hf_cfg)
    if kind not in _STATIC_ROPE:
        raise NotImplementedError(f"LlamaLRP: rope_type {kind!r} (sequence-length dependent frequencies) is not supported")
    if kind != "default":
        from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS
        inv_freq, att = ROPE_INIT_FUNCTIONS[kind](hf_cfg, "cpu")      # (the installed transformers' own initialiser for its own config class)
        cfg["inv_freq"], cfg["attention_scaling"] = inv_freq.float().cpu(), float(att)
    return cfg


def weights_from_hf(model):
    """plain (cfg, W) view of a HF LlamaForCausalLM (no copies; tensors stay where they are)"""
    m = model.model
    W = dict(embed=m.embed_tokens.weight.detach(), norm=m.norm.weight.detach(), lm_head=model.lm_head.weight.detach(),
             layers=[])
    for L in m.layers:
        a, mlp = L.self_attn, L.mlp
        W["layers"].append(dict(ln1=L.input_layernorm.weight.detach(), ln2=L.post_attention_layernorm.weight.detach(),
                                wq=a.q_proj.weight.detach(), wk=a.k_proj.weight.detach(), wv=a.v_proj.weight.detach(),
                                wo=a.o_proj.weight.detach(), wg=mlp.gate_proj.weight.detach(),
                                wu=mlp.up_proj.weight.detach(), wd=mlp.down_proj.weight.detach()))
    return config_from_hf(model.config), W


PITCH_PAD = True          # module attribute, not an environment knob: A/B runs set `engine.PITCH_PAD = False`


def pitch_pad(cols, elem_size):
    """extra elements per row for a K-contiguous GEMM operand: a row pitch that is a multiple of 4 KiB puts the same K offset of every row
    on the same memory channels; measured on MI355X at M = 8192, N = 4096 (tools/pitch_probe.py, profiles/r03_gemm_experiments.txt):
    K = 28672 NT 1357 -> 1553 TFLOP/s with 128 bytes of padding on both operands, K = 14336 1460 -> 1545 (hipBLASLt gains too:
    1533 -> 1603); no effect at K <= 6144 or on the C pitch"""
    nbytes = cols * elem_size
    if not PITCH_PAD:
        return 0
    return 128 // elem_size if (nbytes >= 16384 and nbytes % 4096 == 0) else 0


def weight_pitch_pad(cols, elem_size, rows=0):
    """extra elements per ROW of a stored weight W [out, in] that is larger than the chip's caches: the dgrad c = s W reads it in the NN form --
    512-byte segments of consecutive contraction ROWS, i.e. with the weight's row pitch as the stride -- and a pitch that is a multiple of 4 KiB
    (in = 4096 in bf16) puts a column block of every row on the same memory channels.  Measured on MI355X, M = 8192 (tools/nn_pitch_probe.py,
    profiles/r05_gemm_experiments.txt): the [28672, 4096] gate/up weight 1418 -> 1274 us with 128 bytes of padding per row, 1237 us (1357 -> 1555
    TFLOP/s) with 256; the [6144, 4096] qkv weight 271 -> 267 us; the cache-resident [4096, 4096] o weight and the [4096, 14336] down weight:
    nothing.  256 bytes where the pitch is a multiple of 1 KiB and the weight is at least 32 MB."""
    nbytes = cols * elem_size
    # (round 5, Gemma-3-4B's [20480, 2560] gate/up weight: a pitch of 5 KiB -- a multiple of 1 KiB, not of 4 -- aliases too: dgrad 751 -> 650 us,
    # forward 612 -> 588 us with the same 256 bytes, tools/gemma_pitch_probe.py; the L2-resident qkv / o weights and SigLIP's: nothing)
    if not PITCH_PAD or nbytes % 1024 != 0 or rows * nbytes < (32 << 20):
        return 0
    return 256 // elem_size


# ---- the fused dense Llama layer (M = B S rows): ONE implementation for LlamaLRP and the drop-in's DecoderLayerFn

def fused_layout(H, I, nq, nk, d, dtype):
    """row pitches (elements) of the stored weights Wqkv, Wgu, Wd and the activations m, Agu, Aqkv of a fused layer, in ONE place (Aqkv: the dQ
    kernel stores a row segment per lane into it; a pitch on the 4-KiB grid puts them all on the same channels)"""
    es = dtype.itemsize
    nqkv = (nq + 2 * nk) * d
    return dict(Wqkv=H + weight_pitch_pad(H, es, nqkv), Wgu=H + weight_pitch_pad(H, es, 2 * I), Wd=I + pitch_pad(I, es),
                m=I + pitch_pad(I, es), Agu=2 * I + pitch_pad(2 * I, es), Aqkv=nqkv + (64 if PITCH_PAD and (nqkv * es) % 4096 == 0 else 0))


def fold_rows(dst, srcs, ln):
    """dst <- concat(srcs) diag(ln) (a norm weight folded into the Linear after it): fp32 product, ONE rounding, in 4096-row blocks; srcs may be (dst,)"""
    lnf = ln.detach().to(device=dst.device, dtype=torch.float32)
    r0 = 0
    for w in srcs:
        for b0 in range(0, w.shape[0], 4096):
            blk = w[b0: b0 + 4096].detach()
            dst[r0 + b0: r0 + b0 + blk.shape[0]].copy_((blk.float() * lnf).to(dst.dtype))
        r0 += w.shape[0]
    return dst


FusedOk = collections.namedtuple("FusedOk", "coef norm prep full")


def fused_layer_ok(M, W, meta, dtype, cache):
    """which parts of the fused layer apply at M rows, cached per (M, A/B knobs): coef -- the gated rules as a coefficient stash; norm -- coef and
    the six GEMMs around the norms on the K1n epilogues, at fused_layout's pitches; prep -- the dQ kernel forms D and Gho = 1/2 (Aa Wo) runs on the
    row-scale epilogue; full -- all of it, every NORM_FUSION part and RoPE's backward in the attention backward.  W: wqkv, wo, wgu, wd"""
    key = (M, PITCH_PAD, repr(ops.NORM_FUSION), ops.GATED_FUSION, ops.PREP_FUSION, ops.ROPE_BWD_FUSION)
    hit = cache.get(key)
    if hit is None:
        nq, nk, d, _, act, _ = meta
        H, I, nqkv = W["wo"].shape[0], W["wd"].shape[1], (nq + 2 * nk) * d
        pt = fused_layout(H, I, nq, nk, d, dtype)
        ldo, ldqkv, ldgu, ldd = (W[k].stride(0) for k in ("wo", "wqkv", "wgu", "wd"))
        coef = ops.gated_coef_ok(M, I, H, H, ldgu, H, ldd, act, dtype)
        norm = coef and all(ops.norm_fused_ok(*a, dtype) for a in (
            (M, H, nq * d, nq * d, ldo, False),             # h1 = h + o Wo^T
            (M, H, I, pt["m"], ldd, False),                 # h' = h1 + m Wd^T
            (M, nqkv, H, H, ldqkv, False),                  # qkv = rstd (h W'qkv^T)
            (M, 2 * I, H, H, ldgu, False),                  # gate/up = rstd (h1 W'gu^T)
            (M, H, nqkv, pt["Aqkv"], ldqkv, True),          # G_h = rstd (Aqkv W'qkv) + G_res
            (M, H, 2 * I, pt["Agu"], ldgu, True)))          # G_h1 = rstd (Agu W'gu) + G
        prep = ops.attn_dq_d_ok(dtype, d) and ops.norm_fused_ok(M, nq * d, H, H, ldo, True, dtype)        # (Aa [M, H] contiguous)
        full = (norm and prep and all(ops.norm_fusion_part(p) for p in ("fwd", "bwd_gu", "bwd_qkv")) and ops.ROPE_BWD_FUSION
                and d in (64, 128))
        hit = cache[key] = FusedOk(bool(coef), bool(norm), bool(prep), bool(full))
    return hit


def fused_qkv_fwd(h, rstd1, Wqkv, cos, sin, S, meta, alloc, explicit=False, bias=None, qk_norm=None):
    """-> (qkv, qkr): rstd1 (.) (h Wqkv^T) with RoPE in the GEMM's epilogue where the kernel takes it, else a rope_fwd pass (always in the
    explicit placement: RoPE's stabiliser needs the un-rotated q / k).  meta = (nq, nk, d, eps, act, scale); alloc(tag, rows, cols, pad, dtype).
    The two dense Qwen variants (efficient placement; the defaults are the Llama sequence):
      bias [(nq + 2 nk) d] (Qwen2): added in the same epilogue, in fp32 and ahead of the rotation (HF rotates x W^T + b); the norm-weight fold
        scales columns of W only, the bias is used as stored;
      qk_norm = (wq [d], wk [d]) (Qwen3): the per-head RMSNorm of q and k sits between the projection and RoPE, so the GEMM leaves qkv un-rotated
        and one site kernel norms and rotates; -> (qkv, qkr, rstd_q, rstd_k), the head norms' 1 / rms for fused_layer_bwd."""
    nq, nk, d = meta[:3]
    M, nqk = h.shape[0], (nq + nk) * d
    qkv = alloc("qkv", M, (nq + 2 * nk) * d, 0, h.dtype)
    if qk_norm is not None:
        if bias is None:
            ops.gemm_nt_rs(h, Wqkv, rstd1, qkv)
        else:
            ops.gemm_nt_rs_bias(h, Wqkv, rstd1, bias, qkv)
        qkr = alloc("qkr", M, nqk, 0, h.dtype)
        rstd_q, rstd_k = alloc("rstd_q", 1, M * nq, 0, torch.float32)[0], alloc("rstd_k", 1, M * nk, 0, torch.float32)[0]
        ops.qk_norm_rope_fwd(qkv, qk_norm[0], qk_norm[1], qkr[:, : nq * d], qkr[:, nq * d:], rstd_q, rstd_k, cos, sin, S, nq, nk, d, meta[3])
        return qkv, qkr, rstd_q, rstd_k
    if bias is not None:
        if not explicit and ops.gemm_nt_rs_bias_rope_ok(h, Wqkv, qkv, S, nqk, d):
            return qkv, ops.gemm_nt_rs_bias_rope(h, Wqkv, rstd1, bias, cos, sin, qkv, S, nqk, d)[:, :nqk]
        ops.gemm_nt_rs_bias(h, Wqkv, rstd1, bias, qkv)
        return qkv, ops.rope_fwd(qkv, alloc("qkr", M, nqk, 0, h.dtype), cos, sin, S, nq + nk, d)
    if not explicit and ops.gemm_nt_rs_rope_ok(h, Wqkv, qkv, S, nqk, d):
        return qkv, ops.gemm_nt_rs_rope(h, Wqkv, rstd1, cos, sin, qkv, S, nqk, d)[:, :nqk]
    ops.gemm_nt_rs(h, Wqkv, rstd1, qkv)
    return qkv, ops.rope_fwd(qkv, alloc("qkr", M, nqk, 0, h.dtype), cos, sin, S, nq + nk, d)


def fused_attn_fwd(h, qkv, qkr, W, B, S, meta, alloc, row_iv=None, explicit=False):
    """the attention half of fused_layer_fwd (the MoE driver runs it on its own): attention, h1 = h + o Wo^T with its sums of squares in the
    epilogue -> (dict(o, lse, h1, a, rstd2), ssq)"""
    nq, nk, d, rms_eps, _, scale = meta
    M, H, dt = B * S, h.shape[1], h.dtype
    new = lambda tag, cols: alloc(tag, M, cols, 0, dt)      # noqa: E731
    v = qkv[:, (nq + nk) * d:]
    v_t = ops.transpose_heads(v, B, S, nk, d) if ops.attn_needs_transposed(v, d) else None
    st = dict(o=new("o", nq * d), lse=alloc("lse", B * nq, S, 0, torch.float32).view(B, nq, S))
    ops.attn_fwd(qkr[:, : nq * d], qkr[:, nq * d:], v, v_t, st["o"], st["lse"], B, S, nq, nk, d, scale, True, 0, row_iv=row_iv)
    ssq = alloc("ssq", H // 64, M, 0, torch.float32)
    st.update(h1=new("h1", H), a=new("a", H) if explicit else None)
    ops.gemm_res_ssq(st["o"], W["wo"], h, st["h1"], ssq, raw=st["a"])
    st["rstd2"] = ops.rms_rstd(ssq, M, H, rms_eps, alloc("rstd2", 1, M, 0, torch.float32)[0])
    return st, ssq


def fused_layer_fwd(h, rstd1, qkv, qkr, W, cos, sin, B, S, meta, alloc, row_iv=None, explicit=False, eps=(EFFICIENT["act"], EFFICIENT["lin"]),
                    chain=True):
    """attention, h1 = h + o Wo^T with its sums of squares in the epilogue, the gate/up GEMM on rstd2 (.) h1 with the coefficient stash of the
    gated rule (eps = (eps_g, eps_lin)); chain: the down projection leaves h_out and ITS rstd the same way, else dn = m Wd^T.  explicit: the
    Linears' own outputs a / dn are kept for their stabilisers.  -> dict(o, lse, h1, a, rstd2, gu, m, dn[, h_out, rstd_out]) (m: wherever the
    allocator put it -- a scratch buffer unless the caller keeps it per layer)"""
    nq, nk, d, rms_eps, act, scale = meta
    M, H, I, dt = B * S, h.shape[1], W["wd"].shape[1], h.dtype
    new = lambda tag, cols, pitch=None: alloc(tag, M, cols, (pitch or cols) - cols, dt)      # noqa: E731
    vec = lambda tag: alloc(tag, 1, M, 0, torch.float32)[0]                                  # noqa: E731
    st, ssq = fused_attn_fwd(h, qkv, qkr, W, B, S, meta, alloc, row_iv, explicit)
    pt = fused_layout(H, I, nq, nk, d, dt)
    st["gu"], m = ops.gemm_gated_fwd_coef(st["h1"], W["wgu"], new("gu", 2 * I), new("m", I, pt["m"]), *eps, act, rs=st["rstd2"])
    st["m"] = m
    if chain:
        st["h_out"], st["dn"] = new("h_out", H), new("dn", H) if explicit else None
        ops.gemm_res_ssq(m, W["wd"], st["h1"], st["h_out"], ssq, raw=st["dn"])
        st["rstd_out"] = ops.rms_rstd(ssq, M, H, rms_eps, vec("rstd_out"))
    else:
        st["dn"] = ops.linear_fwd(m, W["wd"], out=new("dn", H))
    return st


def fused_layer_bwd(G, st, W, cos, sin, B, S, meta, alloc, row_iv=None, qk_norm=None, heads=None, attn_map=None, weights=None):
    """efficient placement: G at the layer's output -> G at its input in 7 GEMMs, rules / norms in their epilogues, D and RoPE's backward in the
    attention backward.  st: what the forward left, plus rstd1; alloc("half", 1, M, ...) returns fp32 rows already set to 1/2 (no fill per layer).
    A q / k / v bias (Qwen2) changes nothing here: it receives relevance and passes none on, G_h is the same GEMM.  qk_norm = (wq, wk) (Qwen3;
    st then holds rstd_q, rstd_k): the dQ kernel leaves the gradient of the ROTATED q, and one site kernel builds the whole Aqkv operand -- RoPE
    transposed, the head norms' row-constant scale, the GQA group sums -- in place of gqa_reduce_rope + gqa_reduce.
    heads: a HeadSink (explain(heads=...)) that reads the per-head relevance off the buffers while they are live; None: nothing is launched.
    attn_map: an AttnMapSink (explain(attn_map=...)), the token-to-token maps off the same buffers; None: nothing is launched.
    weights: a WeightSink (explain(weights=...)), the per-weight relevance W (*) G^T X of the four Linears off the same buffers (st["m"] must
    then be the layer's own: keep_m); the norms are folded on this path, so the Linears behind them read the un-normed stream with rs = rstd."""
    nq, nk, d = meta[:3]
    M, H, I, dt = B * S, G.shape[1], W["wd"].shape[1], G.dtype
    pt = fused_layout(H, I, nq, nk, d, dt)
    new = lambda tag, cols, pitch=None: alloc(tag, M, cols, (pitch or cols) - cols, dt)      # noqa: E731
    Agu = ops.gemm_gated_bwd_coef(G, W["wd"], st["gu"], new("Agu", 2 * I, pt["Agu"]))
    if weights is not None:
        weights("down", G, st["m"], W["wd"])
        weights("gate_up", Agu, st["h1"], W["wgu"], rs=st["rstd2"])
    Gs1 = ops.gemm_nn_rs_res(Agu, W["wgu"], st["rstd2"], G, new("Gs1", H))
    return fused_attn_bwd(Gs1, st, W, cos, sin, B, S, meta, alloc, row_iv, qk_norm, heads, attn_map, weights)


def fused_attn_bwd(Gs1, st, W, cos, sin, B, S, meta, alloc, row_iv=None, qk_norm=None, heads=None, attn_map=None, weights=None):
    """the attention half of fused_layer_bwd (the MoE driver runs it on its own): Gs1, the gradient at h1 -> G at the layer's input; everything
    from the o projection's dgrad on.  Arguments as fused_layer_bwd's"""
    nq, nk, d, _, _, scale = meta
    M, H, dt, nqk, nqkv = B * S, Gs1.shape[1], Gs1.dtype, (nq + nk) * d, (nq + 2 * nk) * d
    pt = fused_layout(H, 0, nq, nk, d, dt)          # (Aqkv's pitch does not depend on I)
    new = lambda tag, cols, pitch=None: alloc(tag, M, cols, (pitch or cols) - cols, dt)      # noqa: E731
    Gho = ops.gemm_nn_rs(Gs1, W["wo"], alloc("half", 1, M, 0, torch.float32)[0], new("Gho", nq * d))      # ("half": the allocator's 1/2 rows)
    q, k, v = st["qkr"][:, : nq * d], st["qkr"][:, nq * d:], st["qkv"][:, nqk:]
    D = alloc("D", B * nq, S, 0, torch.float32).view(B, nq, S)
    Aqkv, dk_h, dv_h = new("Aqkv", nqkv, pt["Aqkv"]), new("dk_h", nq * d), new("dv_h", nq * d)
    if heads is not None:
        heads("out", st["o"], Gho, scale=2.0)          # (Gho = 1/2 G_o out of the dgrad's epilogue)
    if weights is not None:
        weights("o", Gs1, st["o"], W["wo"])
    if attn_map is not None:
        attn_map(q, k, v, Gho, st["lse"], 2.0, row_iv)
    if qk_norm is not None:
        dq = ops.attn_bwd_dq_d(q, k, v, Gho, st["o"], st["lse"], D, new("dq", nq * d), B, S, nq, nk, d, scale, row_iv=row_iv)
        ops.attn_bwd_dkv(q, k, v, None, Gho, None, st["lse"], D, dk_h, dv_h, B, S, nq, nk, d, scale, 0.0, 0.0, row_iv=row_iv)
        if heads is not None:
            heads("q", q, dq)
            heads("k", k, dk_h, nq // nk)
            heads("v", v, dv_h, nq // nk)
        ops.qkv_bwd_pack(dq, dk_h, dv_h, qk_norm[0], qk_norm[1], st["rstd_q"], st["rstd_k"], cos, sin, Aqkv, S, nq, nk, d)
        if weights is not None:
            weights("qkv", Aqkv, st["h"], W["wqkv"], rs=st["rstd1"])
        return ops.gemm_nn_rs_res(Aqkv, W["wqkv"], st["rstd1"], Gs1, new("Gh", H))
    ops.attn_bwd_dq_d(q, k, v, Gho, st["o"], st["lse"], D, Aqkv[:, : nq * d], B, S, nq, nk, d, scale, row_iv=row_iv, rope=(cos, sin))
    ops.attn_bwd_dkv(q, k, v, None, Gho, None, st["lse"], D, dk_h, dv_h, B, S, nq, nk, d, scale, 0.0, 0.0, row_iv=row_iv)
    if heads is not None:
        heads("q", q, Aqkv[:, : nq * d], rope=(cos, sin))          # RoPE^T(dq) against the rotated q: lrp_headdot rotates it back
        heads("k", k, dk_h, nq // nk)
        heads("v", v, dv_h, nq // nk)
    ops.gqa_reduce_rope(dk_h, Aqkv[:, nq * d: nqk], M, S, nk, nq // nk, d, cos, sin)
    ops.gqa_reduce(dv_h, Aqkv[:, nqk:], M, nk, nq // nk, d)
    if weights is not None:
        weights("qkv", Aqkv, st["h"], W["wqkv"], rs=st["rstd1"])
    return ops.gemm_nn_rs_res(Aqkv, W["wqkv"], st["rstd1"], Gs1, new("Gh", H))


FUSED_SCRATCH = frozenset(("ssq", "m", "half", "Agu", "Gs1", "Gho", "D", "Aqkv", "dk_h", "dv_h", "dq"))      # temporaries: one buffer serves every layer


# ---- the scaffolding of the fused drivers (LlamaLRP here, Gemma3LRP / Gemma3MMLRP / BertLRP in their modules): one owner per decision

def pack_flat(top, layer, n_layers, dtype, device, align=64):
    """ONE flat buffer holds every weight of a model (a multi-GPU start-up is then a single broadcast of it, lxt_amd.dist.broadcast_weights).
    top / layer: {name: (shape, row pitch or None)} of the model-wide weights and of one layer's, in storage order; the buffer's size follows
    from these lists alone; layer may be a list of n_layers specs (layers of different forms: the MoE driver).  -> (flat, {name: view}, one
    {name: view} per layer).  Every view starts 128-byte aligned; with a row pitch it is a
    [rows, cols] view of [rows, pitch] storage (align: the grid of the view starts in ELEMENTS -- 64 of a 2-byte type; the uint8 buffer of the
    quantised weights passes 128).  device="meta" gives the layout without memory."""
    up = lambda n: (n + align - 1) // align * align                      # noqa: E731
    stored = lambda shape, pitch: (*shape[:-1], pitch or shape[-1])      # noqa: E731  (the [rows, pitch] block behind a view)
    specs = [top] + (list(layer) if isinstance(layer, (list, tuple)) else [layer] * n_layers)
    flat = torch.empty(sum(up(math.prod(stored(*e))) for spec in specs for e in spec.values()), device=device, dtype=dtype)
    views, o = [], 0
    for spec in specs:
        views.append({})
        for name, (shape, pitch) in spec.items():
            full = stored(shape, pitch)
            views[-1][name] = flat[o: o + math.prod(full)].view(full)[..., : shape[-1]]
            o += up(math.prod(full))
    return flat, views[0], views[1:]


def put_rows(dst, *srcs):
    """dst <- srcs stacked along the rows, in dst's device and dtype"""
    o = 0
    for t in srcs:
        dst[o: o + t.shape[0]].copy_(t.to(device=dst.device, dtype=dst.dtype, non_blocking=True))
        o += t.shape[0]
    return dst


def put_gate_up(dst, wg, wu):
    """gate / up rows interleaved in blocks of 32 (ops.interleave_gate_up): the gated-MLP rules then run inside the GEMM epilogues"""
    return ops.interleave_gate_up(wg.to(device=dst.device, dtype=dst.dtype), wu.to(device=dst.device, dtype=dst.dtype), out=dst)


WEIGHT_FORMATS = (None, "mxfp4")
MX_MATRICES = ("wqkv", "wo", "wgu", "wd")          # the Linears of a decoder layer: what weight_format="mxfp4" stores as codes + scales


def weight_format_request(weight_format, cfg):
    """LlamaLRP(weight_format=...) -> the format; raises ValueError before any device work: an unknown name, or (mxfp4: blocks of 32 along the
    contraction dimension K of every stored [N, K] Linear) a K off the 32 grid -- hidden (q/k/v, gate/up), n_heads * head_dim (o), inter (down)"""
    if weight_format not in WEIGHT_FORMATS:
        raise ValueError(f"weight_format must be one of {WEIGHT_FORMATS}, got {weight_format!r}")
    if weight_format == "mxfp4":
        for name, K in (("hidden", cfg["hidden"]), ("n_heads * head_dim", cfg["n_heads"] * cfg["head_dim"]), ("inter", cfg["inter"])):
            if K % ops.MX_BLOCK:
                raise ValueError(f"weight_format='mxfp4': {name} = {K} is not a multiple of {ops.MX_BLOCK} (one scale per {ops.MX_BLOCK} "
                                 "elements along a Linear's contraction dimension)")
    return weight_format


def quant_layout(layer):
    """one layer's spec of flat_layout -> (the spec without the four Linears, the Linears alone, the uint8 spec of their MXFP4 storage:
    name_c -- codes [N, K / 2], name_s -- scales [N, K / 32] with the row pitch on the 4-byte grid)"""
    rest = {k: v for k, v in layer.items() if k not in MX_MATRICES}
    lin = {k: layer[k] for k in MX_MATRICES}
    q = {}
    for k, ((N, K), _) in lin.items():
        q[k + "_c"] = ((N, K // 2), None)
        q[k + "_s"] = ((N, K // ops.MX_BLOCK), (K // ops.MX_BLOCK + 3) // 4 * 4)
    return rest, lin, q


def rope_tables(inv_freq, attention_scaling, max_seq, dtype, device):
    """-> (cos, sin) [max_seq, d] of the rotary frequencies inv_freq [d / 2].  HF hands cos / sin to the layers in the model dtype; keep that
    rounding, store as fp32 tables"""
    fr = torch.arange(max_seq, dtype=torch.float32)[:, None] * inv_freq.float().cpu()[None, :]
    emb = torch.cat((fr, fr), dim=-1)
    return ((emb.cos() * attention_scaling).to(dtype).to(torch.float32).to(device).contiguous(),
            (emb.sin() * attention_scaling).to(dtype).to(torch.float32).to(device).contiguous())


class Arena:
    """Workspace arena: every activation stash and every temporary of one explanation lives in a flat buffer keyed by a tag; the
    buffers persist across calls (same B*S -> no allocator traffic in the per-layer loops, and stable addresses for hipGraph
    replay).  A tag is (name, layer or None); temporaries share one tag across layers.  new / f32 / zeros / wide: the forms the drivers
    allocate, in the model dtype unless named."""

    def __init__(self, device, dtype):
        self.device, self.dtype, self.buf = device, dtype, {}
        self.gen = 0          # bumped whenever a buffer is REPLACED by a larger one: captured graphs hold the old address (GraphCache drops them)

    def get(self, tag, shape, dtype, zero=False, pad=0):
        """pad: extra elements per row of a 2-D buffer (the view returned is [rows, cols] with row pitch cols + pad)"""
        full = tuple(shape[:-1]) + (shape[-1] + pad,) if pad else tuple(shape)
        n = math.prod(full)
        t = self.buf.get((tag, dtype))
        if t is None or t.numel() < n:
            if t is not None:
                self.gen += 1
            t = torch.empty(max(n, 1), device=self.device, dtype=dtype)
            self.buf[(tag, dtype)] = t
        v = t[:n].view(*full)
        if zero:
            v.zero_()
        return v[..., : shape[-1]] if pad else v

    def new(self, tag, *shape):
        return self.get(tag, shape, self.dtype)

    def f32(self, tag, *shape):
        return self.get(tag, shape, torch.float32)

    def zeros(self, tag, *shape):
        return self.get(tag, shape, self.dtype, zero=True)

    def wide(self, tag, rows, cols):
        """a long-K GEMM operand: row pitch off the 4-KiB grid (pitch_pad)"""
        return self.get(tag, (rows, cols), self.dtype, pad=pitch_pad(cols, self.dtype.itemsize))

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self.buf.values())


def explain_inputs(input_ids, inputs_embeds, lengths, target, vocab, max_seq, dtype, device, seed=None):
    """The checks and conversions in front of an explanation; every ValueError is raised before a kernel of the model runs.
    input_ids [B, S] or inputs_embeds [B, S, H] -> (B, S, emb [B S, H] on the device or None, row_iv, idx):
      lengths [B]: prompts LEFT-padded to S -> row_iv = (lo, hi) int32 [B, S], the per-row key intervals of the attention kernels (pad rows:
      empty); else None;  target [B] -> idx int32 vocabulary indices (None: the caller takes the arg-max);  seed [B, V]: instead of target."""
    B, S = input_ids.shape if inputs_embeds is None else inputs_embeds.shape[:2]
    if S > max_seq:
        raise ValueError(f"sequence length {S} exceeds max_seq={max_seq}")
    row_iv = None
    if lengths is not None:
        lens = torch.as_tensor(lengths, device=device).to(torch.int32).reshape(B)
        if int(lens.min()) < 1 or int(lens.max()) > S:
            raise ValueError("lengths must lie in [1, S]")
        i = torch.arange(S, device=device, dtype=torch.int32)
        first = (S - lens)[:, None]
        lo = first.expand(B, S).contiguous()
        hi = torch.where(i[None] >= first, (i + 1)[None].expand(B, S), torch.zeros_like(lo)).contiguous()   # pad rows: empty
        row_iv = (lo, hi)
    idx = None
    if target is not None:
        tgt = torch.as_tensor(target).reshape(-1).cpu().long()
        if tgt.numel() != B or int(tgt.min()) < 0 or int(tgt.max()) >= vocab:
            raise ValueError(f"target must hold {B} vocabulary indices in [0, {vocab})")
        idx = tgt.to(device=device, dtype=torch.int32).contiguous()
    if seed is not None:
        if target is not None:
            raise ValueError("pass either target or seed, not both")
        if tuple(seed.shape) != (B, vocab):
            raise ValueError(f"seed must have shape ({B}, {vocab}), got {tuple(seed.shape)}")
    emb = None if inputs_embeds is None else inputs_embeds.to(device=device, dtype=dtype).reshape(B * S, -1).contiguous()
    return B, S, emb, row_iv, idx


def generate_request(input_ids, inputs_embeds, max_new_tokens, lengths, eos_token_id, pad_token_id, vocab, max_seq):
    """The checks in front of generate(); every ValueError is raised before a kernel runs.  -> (ids int64 [B, S] on the host, lens int64 [B] on
    the host, eos: list of ints (empty: no stopping), pad: int or None (only a finished prompt is ever fed it))"""
    if inputs_embeds is not None or input_ids is None:
        raise ValueError("generate takes input_ids: every new token is fed back through the embedding table, inputs_embeds have no ids to continue")
    try:
        ids = torch.as_tensor(input_ids).cpu()
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"input_ids must be an integer tensor [B, S], got {input_ids!r}") from None
    if ids.dim() != 2 or ids.shape[0] < 1 or ids.shape[1] < 1 or ids.is_floating_point() or ids.dtype == torch.bool:
        raise ValueError(f"input_ids must be integers of shape [B, S], got {tuple(ids.shape)} {ids.dtype}")
    ids = ids.long()
    B, S = ids.shape
    if int(ids.min()) < 0 or int(ids.max()) >= vocab:
        raise ValueError(f"input_ids must hold vocabulary indices in [0, {vocab})")
    if isinstance(max_new_tokens, bool) or not isinstance(max_new_tokens, int) or max_new_tokens < 1:
        raise ValueError(f"max_new_tokens must be an integer >= 1, got {max_new_tokens!r}")
    if S + max_new_tokens > max_seq:
        raise ValueError(f"S + max_new_tokens = {S + max_new_tokens} exceeds max_seq={max_seq} (the RoPE tables and the cache end there)")
    if lengths is None:
        lens = torch.full((B,), S, dtype=torch.long)
    else:
        try:
            lens = torch.as_tensor(lengths).cpu()
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"lengths must be {B} integers, got {lengths!r}") from None
        if lens.numel() != B or lens.is_floating_point() or lens.dtype == torch.bool or int(lens.min()) < 1 or int(lens.max()) > S:
            raise ValueError(f"lengths must be {B} integers in [1, {S}]")
        lens = lens.long().reshape(B)

    def token(name, t):
        if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < vocab:
            raise ValueError(f"{name} must be a vocabulary index in [0, {vocab}), got {t!r}")
        return t

    if eos_token_id is None:
        eos = []
    elif isinstance(eos_token_id, (list, tuple)):
        if not eos_token_id:
            raise ValueError("eos_token_id: an empty list stops nothing (pass None)")
        eos = [token("eos_token_id", t) for t in eos_token_id]
    else:
        eos = [token("eos_token_id", eos_token_id)]
    pad = None if pad_token_id is None else token("pad_token_id", pad_token_id)
    if pad is None and eos:
        pad = eos[0]
    return ids, lens, eos, pad


def force_request(force_tokens, B, max_new_tokens, vocab, device):
    """generate(force_tokens=...) -> None or int32 [B, max_new_tokens] on the device; ValueError before a kernel runs"""
    if force_tokens is None:
        return None
    forced = torch.as_tensor(force_tokens).cpu()
    if tuple(forced.shape) != (B, max_new_tokens) or forced.is_floating_point() or int(forced.min()) < 0 or int(forced.max()) >= vocab:
        raise ValueError(f"force_tokens must hold vocabulary indices in [0, {vocab}) of shape ({B}, {max_new_tokens})")
    return forced.to(device=device, dtype=torch.int32)


SampleSpec = collections.namedtuple("SampleSpec", "temperature top_k top_p min_p seeds streams")


def sample_request(do_sample, temperature, top_k, top_p, min_p, seed, B, force_tokens):
    """generate(do_sample=..., temperature=..., top_k=..., top_p=..., min_p=..., seed=...) -> None (greedy) or a SampleSpec: the scalars as
    ops.sample_rows takes them, seeds int64 [B] and streams int32 [B] on the host.  seed an int: prompt b draws from (seed, stream b);
    seed a list of B ints: prompt b draws from (seed[b], stream 0) -- its continuation then does not depend on the batch it sits in.
    Seeds are taken modulo 2^64.  No device, no weights; ValueError before a kernel runs: a sampling argument or a seed without do_sample,
    do_sample without seed or with force_tokens, temperature <= 0 or not finite, top_k not an int >= 0, top_p outside (0, 1], min_p outside
    [0, 1], seed neither an int nor B ints."""
    if not do_sample:
        if (temperature, top_k, top_p, min_p) != (1.0, 0, 1.0, 0.0) or isinstance(top_k, bool) or seed is not None:
            raise ValueError("temperature, top_k, top_p, min_p and seed apply to do_sample=True only (the default continuation is greedy)")
        return None
    if seed is None:
        raise ValueError("do_sample=True needs seed=int or a list of B ints: a sampled continuation is reproducible from its seed only")
    if force_tokens is not None:
        raise ValueError("do_sample=True together with force_tokens: the forced answer leaves nothing to draw")

    def real(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
        return float(v)

    temperature, top_p, min_p = real("temperature", temperature), real("top_p", top_p), real("min_p", min_p)
    if temperature <= 0.0:
        raise ValueError(f"temperature must be > 0, got {temperature} (greedy decoding is do_sample=False, or top_k=1)")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0:
        raise ValueError(f"top_k must be an integer >= 0 (0: off), got {top_k!r}")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p must lie in (0, 1] (1: off), got {top_p}")
    if not 0.0 <= min_p <= 1.0:
        raise ValueError(f"min_p must lie in [0, 1] (0: off), got {min_p}")
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)      # noqa: E731
    if is_int(seed):
        seeds, streams = [seed] * B, list(range(B))
    elif isinstance(seed, (list, tuple)) and len(seed) == B and all(is_int(v) for v in seed):
        seeds, streams = list(seed), [0] * B
    else:
        raise ValueError(f"seed must be an int or a list of {B} ints, got {seed!r}")
    seeds = [((v & (2 ** 64 - 1)) ^ 2 ** 63) - 2 ** 63 for v in seeds]          # (modulo 2^64, as the int64 that carries the bits)
    return SampleSpec(temperature, top_k, top_p, min_p, torch.tensor(seeds, dtype=torch.int64), torch.tensor(streams, dtype=torch.int32))


PenaltySpec = collections.namedtuple("PenaltySpec", "repetition_penalty presence_penalty frequency_penalty bias")
PenaltyState = collections.namedtuple("PenaltyState", "spec hist out bias")


def penalty_request(repetition_penalty, presence_penalty, frequency_penalty, logit_bias, vocab, force_tokens):
    """generate(repetition_penalty=..., presence_penalty=..., frequency_penalty=..., logit_bias=...) -> None when all four are neutral
    (1.0, 0.0, 0.0, None), else a PenaltySpec: the three scalars as ops.logit_penalty takes them and bias, fp32 [vocab] on the host or None.
    logit_bias: a {token: float} dict or an fp32 [vocab] tensor; -inf bans a token.  No device, no weights; ValueError before a kernel runs:
    repetition_penalty <= 0 or not finite, a presence / frequency penalty that is not finite, a bias key outside [0, vocab), a bias value
    that is NaN or +inf, a bias that bans every column, a tensor that is not fp32 [vocab], any non-neutral setting with force_tokens."""
    def real(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
        return float(v)

    rp, pp, fp = (real(n, v) for n, v in (("repetition_penalty", repetition_penalty), ("presence_penalty", presence_penalty),
                                          ("frequency_penalty", frequency_penalty)))
    if rp <= 0.0:
        raise ValueError(f"repetition_penalty must be > 0 (1: off), got {rp}")
    bias = None
    if torch.is_tensor(logit_bias):
        if logit_bias.dtype != torch.float32 or tuple(logit_bias.shape) != (vocab,):
            raise ValueError(f"logit_bias as a tensor must be float32 [{vocab}], got {logit_bias.dtype} {tuple(logit_bias.shape)}")
        bias = logit_bias.detach().cpu().contiguous()
    elif isinstance(logit_bias, dict):
        if logit_bias:
            bias = torch.zeros(vocab, dtype=torch.float32)
            for k, v in logit_bias.items():
                if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < vocab:
                    raise ValueError(f"logit_bias keys must be vocabulary indices in [0, {vocab}), got {k!r}")
                if isinstance(v, bool) or not isinstance(v, (int, float)):
                    raise ValueError(f"logit_bias[{k}] must be a number, got {v!r}")
                bias[k] = float(v)
    elif logit_bias is not None:
        raise ValueError(f"logit_bias must be a {{token: float}} dict or a float32 [{vocab}] tensor, got {type(logit_bias).__name__}")
    if bias is not None:
        if bool(torch.isnan(bias).any()) or bool((bias == float("inf")).any()):
            raise ValueError("logit_bias values must not be NaN or +inf (-inf bans a token)")
        if bool((bias == -float("inf")).all()):
            raise ValueError(f"logit_bias bans all {vocab} columns: nothing is left to choose")
    if (rp, pp, fp) == (1.0, 0.0, 0.0) and bias is None:
        return None
    if force_tokens is not None:
        raise ValueError("repetition_penalty, presence_penalty, frequency_penalty and logit_bias together with force_tokens: scoring a given "
                         "answer has nothing to penalise")
    return PenaltySpec(rp, pp, fp, bias)


OBJECTIVES = ("logit", "logprob")

SpanRequest = collections.namedtuple("SpanRequest", "T rows idx auto w w_each objective per_position")


def position_request(positions, position_weights, objective, per_position, B, S, vocab, device, input_ids=None, target=None, lengths=None,
                     seed=None, graph=False, mode="efficient", readouts=False):
    """explain(positions=..., position_weights=..., objective=..., per_position=...) -> None without positions, else a SpanRequest, all in
    slot order [B, T] (R = B T explained rows; row p of prompt b predicts the token after column p -- teacher forcing):
      T;  rows int64 [R] = b S + p, the explained rows of the [B S, .] activations;  idx int32 [R], the explained vocabulary indices --
      target [B, T], else input_ids[b, p + 1] for p < S - 1;  auto int64 [n], the slots with p = S - 1 and no target (the caller fills them
      with the row's arg-max once the logits exist), or None;  w fp32 [R], the slot weights (default ones);  w_each fp32 [T, R] for
      per_position (pass t keeps slot t's weight and zeroes the others), else None;  objective, per_position.
    The tensors are built on the host and moved to `device` (a CPU device serves the checks).  Raises ValueError before a kernel of the model
    runs: positions that are not [B, T] integers with T >= 1, outside [0, S), repeated within a prompt or on a pad column (< S - lengths[b]);
    weights or target of another shape, non-finite weights, a target outside [0, vocab), no target with inputs_embeds; an unknown objective;
    positions together with seed or graph=True; mode="explicit" (its seed is a relevance, not a gradient: no span form is defined for it);
    per_position together with a read-out keyword (readouts); position_weights / objective / per_position without positions."""
    if objective not in OBJECTIVES:
        raise ValueError(f"objective must be one of {OBJECTIVES}, got {objective!r}")
    if positions is None:
        if position_weights is not None or per_position or objective != "logit":
            raise ValueError("position_weights / objective / per_position need positions=...")
        return None
    if seed is not None:
        raise ValueError("positions: pass either positions (with target) or seed, not both")
    if graph:
        raise ValueError("positions: graph=True is not supported (the explained rows are an input of the call)")
    if mode != "efficient":
        raise ValueError(f"positions: span targets are defined for the efficient placement only, not mode={mode!r}")
    if per_position and readouts:
        raise ValueError("per_position=True returns R_tok_each only; it does not combine with layer_relevance / return_G / latent / heads / "
                         "attn_map / weights / experts")
    try:
        pos = torch.as_tensor(positions).cpu()
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"positions must be an integer tensor or nested list [B, T], got {positions!r}") from None
    if pos.dim() != 2 or pos.shape[0] != B or pos.shape[1] < 1 or pos.is_floating_point() or pos.is_complex() or pos.dtype == torch.bool:
        raise ValueError(f"positions must be integers of shape [{B}, T] with T >= 1, got {tuple(pos.shape)} {pos.dtype}")
    pos = pos.long()
    T = pos.shape[1]
    if int(pos.min()) < 0 or int(pos.max()) >= S:
        raise ValueError(f"positions must be column indices in [0, {S})")
    if bool((pos.sort(1).values.diff(dim=1) == 0).any()):
        raise ValueError("positions must be distinct within a prompt (point a spare slot at another column and give it weight 0)")
    if lengths is not None:
        first = S - torch.as_tensor(lengths).cpu().long().reshape(B, 1)
        if bool((pos < first).any()):
            raise ValueError("positions must lie inside the prompt's own columns (>= S - lengths[b]), not on its padding")
    if position_weights is None:
        w = torch.ones(B, T, dtype=torch.float32)
    else:
        try:
            w = torch.as_tensor(position_weights).cpu().to(torch.float32)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"position_weights must be a float tensor [B, T], got {position_weights!r}") from None
        if tuple(w.shape) != (B, T) or not bool(torch.isfinite(w).all()):
            raise ValueError(f"position_weights must be finite floats of shape ({B}, {T})")
    auto = None
    if target is not None:
        tgt = torch.as_tensor(target).cpu()
        if tuple(tgt.shape) != (B, T) or tgt.is_floating_point() or int(tgt.min()) < 0 or int(tgt.max()) >= vocab:
            raise ValueError(f"target must hold vocabulary indices in [0, {vocab}) of shape ({B}, {T}), one per position")
        idx = tgt.long()
    else:
        if input_ids is None:
            raise ValueError("positions with inputs_embeds needs target [B, T] (there are no next-token ids to default to)")
        ids = torch.as_tensor(input_ids).cpu().long().reshape(B, S)
        idx = torch.gather(ids, 1, (pos + 1).clamp(max=S - 1))          # (p = S - 1: a placeholder until the arg-max is known)
        slots = torch.nonzero((pos == S - 1).reshape(-1))[:, 0]
        auto = slots.to(device) if slots.numel() else None
    rows = (torch.arange(B)[:, None] * S + pos).reshape(-1)
    w_each = None
    if per_position:
        w_each = (torch.eye(T, dtype=torch.float32)[:, None, :] * w[None]).reshape(T, B * T).contiguous().to(device)
    return SpanRequest(T, rows.to(device), idx.reshape(-1).to(torch.int32).contiguous().to(device), auto, w.reshape(-1).contiguous().to(device),
                       w_each, objective, bool(per_position))


LATENT = ("trace", "resid", "mlp")


def latent_request(latent, H, I, dtype):
    """explain(latent=...) -> frozenset of the requested read-outs of a latent feature attribution ("trace": per-token relevance at every
    residual boundary, "resid": token-summed per residual dimension, "mlp": token-summed per MLP neuron); None -> the empty set.  Raises
    ValueError before a kernel of the model runs: an unknown name, or a request the column read-out cannot serve (lrp_colsum_dot reads rows
    of a multiple of 16 bytes: H for "resid", I for "mlp")"""
    if latent is None:
        return frozenset()
    try:
        names = (latent,) if isinstance(latent, str) else tuple(latent)
    except TypeError:
        raise ValueError(f"latent must be an iterable of names from {LATENT}, got {latent!r}") from None
    bad = [n for n in names if n not in LATENT]
    if bad:
        raise ValueError(f"latent: unknown read-out(s) {bad}; choose from {LATENT}")
    req = frozenset(names)
    for name, n in (("resid", H), ("mlp", I)):
        if name in req and (n * dtype.itemsize) % 16:
            raise ValueError(f"latent={name!r} needs rows of a multiple of 16 bytes ({n} elements of {dtype} are not)")
    return req


HEADS = ("out", "q", "k", "v")


def head_request(heads, d, dtype):
    """explain(heads=...) -> frozenset of the requested per-head read-outs ("out": the relevance each head writes, at the o projection's input;
    "q" / "k" / "v": at the attention's query / key / value input, k and v per QUERY head); None -> the empty set.  Raises ValueError before a
    kernel of the model runs: an unknown name, a non-iterable, or a head dim lrp_headdot cannot read (rows of a head are 16-byte vectors,
    d <= 256)"""
    if heads is None:
        return frozenset()
    try:
        names = (heads,) if isinstance(heads, str) else tuple(heads)
    except TypeError:
        raise ValueError(f"heads must be an iterable of names from {HEADS}, got {heads!r}") from None
    bad = [n for n in names if n not in HEADS]
    if bad:
        raise ValueError(f"heads: unknown read-out(s) {bad}; choose from {HEADS}")
    req = frozenset(names)
    if req and (not isinstance(d, int) or d < 1 or d > 256 or (d * dtype.itemsize) % 16):
        raise ValueError(f"heads: the per-head read-out needs a head dim <= 256 whose rows are a multiple of 16 bytes ({d} elements of {dtype} are not)")
    return req


class HeadSink:
    """the per-head read-outs of one explanation: out[name] [L, B, nq, S] fp32, one ops.headdot per requested name and layer on the buffers the
    attention backward has just left (the fused-layer functions and LlamaLRP.backward call it; a name that was not requested launches nothing).
    rope_scale: 1 / s^2 for rotary tables that carry an attention_scaling s (the rotated read-out applies the tables a second time)"""

    def __init__(self, req, nL, B, S, nq, d, device, rope_scale=1.0):
        self.B, self.S, self.nq, self.d, self.rope_scale, self.li = B, S, nq, d, rope_scale, None
        self.out = {n: torch.empty(nL, B, nq, S, device=device, dtype=torch.float32) for n in HEADS if n in req}

    def layer(self, li):
        self.li = li
        return self

    def __call__(self, name, x, g, rep=1, scale=1.0, rope=None):
        if name in self.out:
            ops.headdot(x, g, self.B, self.S, self.nq, rep, self.d, scale * (self.rope_scale if rope is not None else 1.0), rope,
                        out=self.out[name][self.li])

    def last(self, name, x_l, g_l):
        """the sparse top layer: one live query row per prompt -- the last column from those rows, exactly 0 elsewhere"""
        if name in self.out:
            dst = self.out[name][self.li].zero_()
            dst[:, :, self.S - 1].copy_(ops.headdot(x_l, g_l, self.B, 1, self.nq, 1, self.d)[:, :, 0])


ATTN_MAP_SUM = "sum"


def attn_map_request(attn_map, nL, nq, d, dtype, mode, bf16_dims=(64, 128)):
    """explain(attn_map=...) -> (want_sum, pairs): "sum" asks for the token-to-token attention relevance summed over the query heads of every
    layer, a (layer, head) pair for the map of one query head; an iterable may mix both, repeated entries count once and the pairs keep the
    order of their first mention.  None -> (False, ()).  Raises ValueError before a kernel of the model runs: an unknown name, a non-iterable,
    a pair outside [0, nL) x [0, nq) (negative indices are not wrapped), a head dim or dtype the caller's map kernel does not serve (bf16:
    bf16_dims -- lrp_attn_relmap's 64 and 128, the Gemma-3 drivers add lrp_attn_relmap_d256's 256; fp32: a multiple of 4 up to 256), or the
    explicit placement (its Gho carries the eps_pv ratio: a different quantity, pinned by no fixture)"""
    if attn_map is None:
        return False, ()
    if isinstance(attn_map, str):
        items = (attn_map,)
    else:
        try:
            items = tuple(attn_map)
        except TypeError:
            raise ValueError(f'attn_map must be "{ATTN_MAP_SUM}" or an iterable of (layer, head) pairs, got {attn_map!r}') from None
    want_sum, pairs = False, []
    for it in items:
        if isinstance(it, str):
            if it != ATTN_MAP_SUM:
                raise ValueError(f'attn_map: unknown request {it!r}; choose "{ATTN_MAP_SUM}" or (layer, head) pairs')
            want_sum = True
            continue
        try:
            l, h = (operator.index(x) for x in it)
        except (TypeError, ValueError):
            raise ValueError(f'attn_map: {it!r} is neither "{ATTN_MAP_SUM}" nor a (layer, head) pair of integers') from None
        if not (0 <= l < nL and 0 <= h < nq):
            raise ValueError(f"attn_map: pair ({l}, {h}) outside the model's {nL} layers x {nq} query heads")
        if (l, h) not in pairs:
            pairs.append((l, h))
    if want_sum or pairs:
        if mode != "efficient":
            raise ValueError(f"attn_map: token-to-token maps are defined for the efficient placement only, not mode={mode!r}")
        ok = isinstance(d, int) and ((dtype == torch.bfloat16 and d in bf16_dims) or (dtype == torch.float32 and 1 <= d <= 256 and d % 4 == 0))
        if not ok:
            raise ValueError(f"attn_map: no kernel for head dim {d} in {dtype} (bf16: 64 or 128; fp32: a multiple of 4 up to 256)")
    return want_sum, tuple(pairs)


class AttnMapSink:
    """the token-to-token maps of one explanation: total [L, B, S, S] fp32 ("sum": all query heads) and per_head [n, B, S, S] (the requested
    (layer, head) pairs, in request order), one ops.attn_relmap per output and layer on the buffers the attention backward is about to read
    (rotated q / k, v, Gho, lse); a layer nothing was requested of launches nothing"""

    def __init__(self, req, nL, B, S, nq, nk, d, scale, device):
        want_sum, self.pairs = req
        self.B, self.S, self.nq, self.nk, self.d, self.scale, self.li = B, S, nq, nk, d, scale, None
        self.total = torch.empty(nL, B, S, S, device=device, dtype=torch.float32) if want_sum else None
        self.per_head = torch.empty(len(self.pairs), B, S, S, device=device, dtype=torch.float32) if self.pairs else None

    def layer(self, li):
        self.li = li
        return self

    def __call__(self, q, k, v, g, lse, gscale, row_iv=None, causal=True):
        """causal=False: row_iv holds COMPLETE per-row key intervals (Gemma-3 image + text prompts: an image block sees itself in both
        directions); a sliding window arrives folded into row_iv's lower ends"""
        a = (q, k, v, g, lse, self.B, self.S, self.nq, self.nk, self.d, self.scale)
        if self.total is not None:
            ops.attn_relmap(*a, gscale=gscale, causal=causal, row_iv=row_iv, out=self.total[self.li])
        for n, (l, h) in enumerate(self.pairs):
            if l == self.li:
                ops.attn_relmap(*a, heads=(h, h + 1), gscale=gscale, causal=causal, row_iv=row_iv, out=self.per_head[n])

    def top(self, ar, q, k, v, Gho, lse, gscale, last, row_iv=None, causal=True):
        """the sparse top layer: Gho is dense with one live row per prompt, and lse is written for those rows only -- every other row gets an
        empty key interval, so it is exactly 0 whatever its lse holds.  The interval vectors are arena buffers (ar), as every temporary of
        the backward"""
        M = self.B * self.S
        hi_live = ar.get("am_hi_l", (last.numel(),), torch.int32)
        if row_iv is None:
            lo, hi_live = ar.get("am_lo", (M,), torch.int32, zero=True), hi_live.fill_(self.S)
        else:
            lo, hi_live = row_iv[0].reshape(M), torch.index_select(row_iv[1].reshape(M), 0, last, out=hi_live)
        hi = ar.get("am_hi", (M,), torch.int32, zero=True).index_copy_(0, last, hi_live)
        self(q, k, v, Gho, lse, gscale, (lo, hi), causal)


WEIGHTS = ("qkv", "o", "gate_up", "down")


def weight_shapes(cfg):
    """{name: (N, K)} of the four decoder Linears in HF row order (qkv = q | k | v rows, gate_up = gate rows then up rows)"""
    H, I, nq, nk, d = cfg["hidden"], cfg["inter"], cfg["n_heads"], cfg["n_kv"], cfg["head_dim"]
    return dict(qkv=((nq + 2 * nk) * d, H), o=(H, nq * d), gate_up=(2 * I, H), down=(H, I))


def weight_request(weights, weight_layers, weights_out, cfg, nL, dtype, mode="efficient", graph=False):
    """explain(weights=..., weight_layers=..., weights_out=...) -> (names, layers): the requested per-weight relevance matrices in WEIGHTS
    order and the ascending layer indices (default: every layer); weights=None -> ((), ()).  Raises ValueError before a kernel of the model
    runs: an unknown name, a non-iterable, layer indices that are not ascending integers in [0, nL) (negative indices are not wrapped),
    weight_layers / weights_out without weights, the explicit placement (the reference's explicit rules define no weight gradient),
    graph=True (the outputs of a dataset-level accumulation are the caller's, not a graph's static buffers), a bf16 Linear whose sizes are
    off lrp_wgrad_rel's grid of 8, or a weights_out that is not a previous call's R_W for the same names and layers"""
    if weights is None:
        if weight_layers is not None or weights_out is not None:
            raise ValueError("weight_layers / weights_out need weights=...")
        return (), ()
    try:
        names = (weights,) if isinstance(weights, str) else tuple(weights)
    except TypeError:
        raise ValueError(f"weights must be an iterable of names from {WEIGHTS}, got {weights!r}") from None
    bad = [n for n in names if n not in WEIGHTS]
    if bad:
        raise ValueError(f"weights: unknown matrix name(s) {bad}; choose from {WEIGHTS}")
    names = tuple(n for n in WEIGHTS if n in names)
    if weight_layers is None:
        layers = tuple(range(nL))
    else:
        try:
            layers = tuple(operator.index(l) for l in weight_layers)
        except TypeError:
            raise ValueError(f"weight_layers must be an iterable of layer indices, got {weight_layers!r}") from None
        if any(not 0 <= l < nL for l in layers) or any(a >= b for a, b in zip(layers, layers[1:])):
            raise ValueError(f"weight_layers must be ascending layer indices in [0, {nL}), got {list(layers)}")
    if not names or not layers:
        if weights_out is not None:
            raise ValueError("weights_out without a matrix or a layer to accumulate")
        return (), ()
    if mode != "efficient":
        raise ValueError(f"weights: the per-weight relevance is defined for the efficient placement only, not mode={mode!r}")
    if graph:
        raise ValueError("weights: graph=True is not supported (R_W is allocated, or accumulated into the caller's tensors, per call)")
    shapes = weight_shapes(cfg)
    if dtype == torch.bfloat16:
        for n in names:
            if shapes[n][0] % 8 or shapes[n][1] % 8:
                raise ValueError(f"weights: the bf16 kernel needs both sizes of {n!r} {shapes[n]} to be multiples of 8")
    if weights_out is not None:
        if not isinstance(weights_out, dict) or set(weights_out) != set(names):
            raise ValueError(f"weights_out must be a previous call's R_W with exactly the matrices {list(names)}")
        for n in names:
            t = weights_out[n]
            if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (len(layers), *shapes[n]) or not t.is_contiguous():
                raise ValueError(f"weights_out[{n!r}] must be a contiguous float32 [{len(layers)}, {shapes[n][0]}, {shapes[n][1]}] tensor")
    return names, layers


class WeightSink:
    """the per-weight relevance of one explanation: out[name] [len(layers), N, K] fp32 in HF row order, one ops.wgrad_rel per requested
    matrix and layer on the buffers the backward has just left (the fused-layer functions and LlamaLRP.backward call it; a layer or a name
    that was not requested launches nothing).  prev: a previous call's R_W -- this call's values are ADDED to it in place (every matrix of
    every layer is visited exactly once per explanation, with all tokens of all prompts in one contraction)"""

    def __init__(self, req, cfg, device, prev=None):
        names, self.layers = req
        shapes = weight_shapes(cfg)
        self.slot, self.accumulate, self.li = {l: i for i, l in enumerate(self.layers)}, prev is not None, None
        if prev is not None and any(t.device != torch.empty(0, device=device).device for t in prev.values()):          # ("cuda" -> "cuda:N")
            raise ValueError(f"weights_out must live on {device}")
        self.out = {n: torch.empty(len(self.layers), *shapes[n], device=device, dtype=torch.float32) for n in names} if prev is None else prev
        self.row_map = ops.gate_up_row_map(cfg["inter"], device) if "gate_up" in names else None      # (wgu is stored gate / up interleaved)

    def layer(self, li):
        """-> the sink positioned at layer li, or None when nothing of that layer was requested"""
        self.li = li
        return self if li in self.slot else None

    def __call__(self, name, G, X, W, rs=None):
        """G: the gradient at the Linear's output, X: its input (with rs = the 1 / rms of a norm in front of it when X is un-normed)"""
        if name in self.out:
            ops.wgrad_rel(G, X, W, out=self.out[name][self.slot[self.li]], rs=rs, row_map=self.row_map if name == "gate_up" else None,
                          accumulate=self.accumulate, check_map=False)


class GraphCache:
    """hipGraph capture and replay of whole explanations, one graph per key.  The first call of a key warms up on a side stream (sizes the
    workspace, loads the kernels), then captures run(*inputs) on static copies of the inputs; every call copies its inputs into those and
    replays.  The returned tensors are the graph's static outputs (copy them before the next call).  gen(): the workspace generation -- a
    graph captured before the arena re-allocated one of its buffers (a later, larger call) points into freed memory: it is dropped and
    captured again against the arena as it is now."""

    def __init__(self, device, gen=lambda: 0):
        self.device, self.gen, self.graphs = device, gen, {}

    def clear(self):
        self.graphs = {}

    def __call__(self, key, run, *inputs):
        g = self.graphs.get(key)
        if g is not None and g[3] != self.gen():
            del self.graphs[key]
            g = None
        if g is None:
            static = [None if t is None else t.clone() for t in inputs]
            side = torch.cuda.Stream(self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):                        # warm-up outside the capture
                run(*static)
            torch.cuda.current_stream(self.device).wait_stream(side)
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg):
                out = run(*static)
            g = self.graphs[key] = (cg, static, out, self.gen())
        cg, static, out, _ = g
        for s, t in zip(static, inputs):
            if s is not None:
                s.copy_(t)
        cg.replay()
        return out


def greedy_decode(logits, step, cols, ids, lens, max_new_tokens, eos, pad, forced, return_logits, penalty=None, sampler=None):
    """the token loop of generate(), shared by the drivers: logits fp32 [B, V] of the prefill's last rows; step(tok int64 [B], pos int32 [1])
    -> (logits, arg-max idx) of one decode step (eager or a GraphCache replay); cols int32 [max_new_tokens]: cols[t - 1: t] is the column of
    step t's input token; ids int64 [B, S] on the device, lens int64 [B] on the host; eos / pad as generate_request returns them; forced
    int32 [B, max_new_tokens] or None.  -> generate()'s dict.  B flags are read back per token with eos, nothing without.
    sampler: a SampleSpec (sample_request) -- token t is ops.sample_rows of step t's logits at Philox counter t in place of the arg-max, one
    launch per token next to span_seed's (outside the captured step); logit / logprob stay the model's own, untempered values of the drawn
    token, and the dict gains sample_logprob [B, T'] = log(q_tok / Z) under the temperature and the filters
    penalty: a PenaltyState (generate_cached: the PenaltySpec, the history table of the prompt, the processed-logits buffer, the bias on the
    device) -- ops.logit_penalty turns step t's raw logits into processed ones, counting the token fed into step t first, one launch per token
    outside the captured step; the token is the arg-max or the draw of the PROCESSED logits, while logit / logprob / return_logits stay the
    model's raw values and sample_logprob is under the processed distribution"""
    dev, B = ids.device, ids.shape[0]
    eos_t = torch.tensor(eos, device=dev, dtype=torch.int32) if eos else None
    fin = torch.zeros(B, device=dev, dtype=torch.bool)
    n_new = torch.zeros(B, device=dev, dtype=torch.long)
    toks, logit, logprob, rows = [], [], [], []
    idx = ops.argmax_rows(logits)[0] if penalty is None else None
    if sampler is not None:
        seeds, streams, slp = sampler.seeds.to(dev), sampler.streams.to(dev), []
    last = None
    for t in range(max_new_tokens):
        if t:
            logits, idx = step(toks[-1], cols[t - 1: t])
        scores = logits
        if penalty is not None:
            scores = ops.logit_penalty(logits, penalty.hist, last, *penalty.spec[:3], bias=penalty.bias, out=penalty.out)
            if sampler is None:
                idx = ops.argmax_rows(scores)[0]
        if sampler is not None:
            idx, lq, _, _ = ops.sample_rows(scores, sampler.temperature, sampler.top_k, sampler.top_p, sampler.min_p, seeds, streams, step=t)
            slp.append(lq)
        if forced is not None:
            idx = forced[:, t]
        if eos:
            idx = torch.where(fin, torch.full_like(idx, pad), idx)          # (a copy: idx may be a graph's static output)
        lg, lp, _, _ = ops.span_seed(logits, idx.contiguous())
        toks.append(idx.long())
        if penalty is not None:
            last = idx.contiguous()
        logit.append(lg)
        logprob.append(lp)
        if return_logits:
            rows.append(logits.clone())
        n_new += ~fin
        if eos:
            fin |= torch.isin(idx, eos_t)
            if bool(fin.all()):
                break
    new = torch.stack(toks, 1)
    out = dict(sequences=torch.cat((ids, new), 1), new_tokens=new, n_new=n_new, logit=torch.stack(logit, 1), logprob=torch.stack(logprob, 1),
               lengths=lens.to(dev) + new.shape[1])
    if return_logits:
        out["logits"] = torch.stack(rows, 1)
    if sampler is not None:
        out["sample_logprob"] = torch.stack(slp, 1)
    return out


def generated_span(out, position_weights):
    """generate()'s dict -> (positions [B, T'], weights) of explain_generated(): the rows S - 1 .. S + T' - 2 that predict the new tokens;
    weights None: 1 for t < n_new[b], else 0; "mean": 1 / n_new[b] instead; anything else is handed on as given"""
    new, n_new = out["new_tokens"], out["n_new"]
    S, T = out["sequences"].shape[1] - new.shape[1], new.shape[1]
    if position_weights is None or (isinstance(position_weights, str) and position_weights == "mean"):
        w = (torch.arange(T, device=n_new.device)[None] < n_new[:, None]).to(torch.float32)
        if position_weights is not None:
            w = w / n_new[:, None].to(torch.float32)
    else:
        w = position_weights
    return torch.arange(S - 1, S + T - 1).expand(new.shape[0], T), w


def head_fwd(ar, h, branch, top, last, norm, lm_head, eps, w_offset=0.0):
    """final residual add h + branch, norm and LM head on the explained (last) row of each prompt; top: the sparse top layer has left one row
    per prompt already.  -> dict(hL_last, dn_last, rstd_f, logits) for the explanation's backward"""
    B = last.shape[0]
    if not top:
        h = h.index_select(0, last)
        branch = None if branch is None else branch.index_select(0, last)
    hL_last = ar.new("hL_last", B, h.shape[1])
    xn, rstd_f = ops.add_rmsnorm_fwd(h, branch, norm, eps, w_offset, hsum_out=hL_last)
    logits = ops.linear_fwd(xn, lm_head, out=ar.f32("logits", B, lm_head.shape[0]))
    return dict(hL_last=hL_last, dn_last=branch, rstd_f=rstd_f, logits=logits)


def top_attn_operands(ar, Gof_l, o_l, Gs1_l, last, S, nq, d, eps_pv):
    """the sparse top layer's backward has one live row per prompt: the attention's output-gradient prep on those rows, then the scatter into
    the dense [M, .] operands of the attention backward (library launches only: zero fill + row scatter; D's live column S - 1 is a strided
    2-D scatter of the same kind).  -> (Gho, D, Gs1)"""
    B = last.shape[0]
    Gho_l, D_l = ar.new("Gho_l", B, nq * d), ar.f32("D_l", B, nq, 1)
    ops.attn_bwd_prep(Gof_l, o_l, Gho_l, D_l, B, 1, nq, d, eps_pv, 0.5)
    Gho = ar.zeros("Gho", B * S, nq * d).index_copy_(0, last, Gho_l)
    D = ar.get("D", (B, nq, S), torch.float32, zero=True)
    D.view(B * nq, S)[:, S - 1].copy_(D_l.view(B * nq))
    Gs1 = ar.zeros("Gs1", B * S, Gs1_l.shape[1]).index_copy_(0, last, Gs1_l)
    return Gho, D, Gs1


def explanation(emb, G, idx, logits, B, S, return_G=False):
    """what explain() returns: dict(idx [B], logit [B], R_tok [B, S] fp32 = sum_h emb (*) G, logits [B, V][, G_emb, emb [B, S, H]])"""
    logits = logits.clone()                                  # (the arena's buffer is overwritten by the next call)
    out = dict(idx=idx, logit=logits.gather(1, idx.long()[:, None])[:, 0], R_tok=ops.readout(emb, G).view(B, S), logits=logits)
    if return_G:
        out["G_emb"], out["emb"] = G.view(B, S, -1).clone(), emb.view(B, S, -1)
    return out


def readout_outputs(out, B, S, layer_R, lat, want_layer_R, want_trace, hs, am, device, span_rows=None):
    """the read-outs of one explanation added to explain()'s dict under LlamaLRP.explain's names (README);
    layer_R: [rel_last [B], per-token rows [M] from the top boundary down to the embedding] or None.  span_rows int64 [B T]
    (explain(positions=...)): rel_last has one entry per explained row; they are placed at their columns (distinct rows: a copy, exactly
    0 elsewhere), so a prompt's head sum is the same fixed-order row sum as every other layer's and R_trace[L].sum(-1) IS layer_R[L]"""
    if span_rows is not None and (want_layer_R or want_trace):
        head_rows = torch.zeros(B * S, device=device, dtype=torch.float32).index_copy_(0, span_rows, layer_R[0]).view(B, S)
    if want_layer_R:
        rows = [layer_R[0] if span_rows is None else head_rows.sum(1)] + [r.view(B, S).sum(1) for r in layer_R[1:]]
        out["layer_R"] = torch.stack(rows[::-1], 0)          # [L+1, B], index 0 = embedding
    if want_trace:
        # the per-token rows layer_R sums: index l = the input of layer l (l = 0: R_tok itself), index L = the head's explained rows
        nL = len(layer_R) - 1
        trace = torch.zeros(nL + 1, B, S, device=device, dtype=torch.float32)
        trace[0] = out["R_tok"]
        for li in range(1, nL):
            trace[li] = layer_R[nL - li].view(B, S)
        if span_rows is None:
            trace[nL, :, S - 1] = layer_R[0]
        else:
            trace[nL] = head_rows
        out["R_trace"] = trace
    out.update(lat)
    if hs is not None:
        out.update({"R_head_" + n: t for n, t in hs.out.items()})
        if "out" in hs.out:
            out["R_head"] = hs.out["out"].sum(-1)
    if am is not None:
        if am.total is not None:
            out["R_attn"] = am.total
        if am.per_head is not None:
            out["R_attn_heads"], out["attn_map_heads"] = am.per_head, list(am.pairs)
    return out


def head_seed_bwd(ar, fw, idx, norm, lm_head, eps_lin, w_offset=0.0, seed=None):
    """LM head eps rule + final-norm identity rule ((w + w_offset) rstd, the rstd detached) on the explained row of each prompt -> Gh_last
    [R, H], the gradient at h_L.  fw["span"] (explain(positions=...)): the same on the R = B T explained rows in slot order -- lrp_span_seed
    leaves span["logit"] / span["logprob"], the row scale w (*) rstd_f of the one-hot route ("logit"), or the dense seed w (delta - softmax)
    in the engine dtype ("logprob": the route of seed=, without its casts).  seed [B, V]: a dense seed over the last-position logits
    (contrastive explanations): a gradient where eps_lin = 0, else a relevance (coef = R / (z + eps)); G_xn = coef @ W_lm (ops.linear_dgrad:
    W streamed once from its stored layout), then the final norm's row scale"""
    R, H, span = fw["last"].shape[0], lm_head.shape[1], fw.get("span")
    if span is not None:
        dense = span["objective"] == "logprob"
        sd = ar.new("span_seed", R, lm_head.shape[0]) if dense else None
        span["logit"], span["logprob"], rs, _ = ops.span_seed(fw["logits"], idx, span["w"], fw["rstd_f"], span["objective"], seed=sd,
                                                              logit=ar.f32("span_logit", R), logprob=ar.f32("span_logprob", R),
                                                              rs=ar.f32("span_rs", R))
        if not dense:
            return ops.head_seed(lm_head, fw["logits"], idx, norm, rs, ar.new("Gh_last", R, H), w_offset, eps_lin)
        coef = sd
    elif seed is None:
        return ops.head_seed(lm_head, fw["logits"], idx, norm, fw["rstd_f"], ar.new("Gh_last", R, H), w_offset, eps_lin)
    else:
        coef = seed.to(device=ar.device, dtype=torch.float32).reshape(R, -1).contiguous()
        if eps_lin != 0.0:
            coef = ops.eps_scale(coef, fw["logits"], 1.0, eps_lin, relevance=True)
        coef = coef.to(ar.dtype)
    g_xn = ops.linear_dgrad(coef, lm_head, out_dtype=torch.float32)
    return ops.head_norm_bwd(g_xn, norm, fw["rstd_f"], ar.new("Gh_last", R, H), w_offset)


def explain_pipeline(drv, forward, backward, emb, B, S, idx, attn_scale, rope_scale=1.0, return_G=False, layer_relevance=False,
                     latent=frozenset(), heads=frozenset(), attn_map=(False, ()), span=None):
    """forward + backward + read-outs of one explanation on the current stream, the one sequence behind LlamaLRP._run and
    Gemma3LRP.explain_emb -> (explain()'s dict, G at the embedding).  Library launches only, no host synchronisation (capturable); with no
    request the buffers, the launches and every output are those of the plain call.  What differs between the drivers is handed in:
      forward(**rows) -> the driver's forward state (rows=span.rows for a span: the explained rows, the top layer then runs dense);
      backward(fw, idx, layer_relevance, latent, heads, attn_map) -> (G, layer_R rows or None, dict of the token-summed read-outs);
      attn_scale, rope_scale: the softmax scale the AttnMapSink applies and the HeadSink's 1 / s^2 of rotary tables with a post-scale.
    idx int32 [B] or None (the arg-max of the explained row; a dense seed explains no single logit, idx / logit then report the arg-max for
    convenience); latent / heads / attn_map: CHECKED requests; span: a SpanRequest (position_request) or None."""
    c, nL, dev = drv.cfg, len(drv.layers), drv.device
    fw = forward(**({} if span is None else dict(rows=span.rows)))
    if span is not None:
        T, idx = span.T, span.idx
        if span.auto is not None:          # the slots at column S - 1 without a target: that row's arg-max (a row copy, no arithmetic)
            idx.index_copy_(0, span.auto, ops.argmax_rows(fw["logits"])[0].index_select(0, span.auto))
        fw["span"] = sp = dict(w=span.w, objective=span.objective)
        head = lambda: dict(idx=idx.view(B, T), logit=sp["logit"].view(B, T).clone(), logprob=sp["logprob"].view(B, T).clone())      # noqa: E731
        if span.per_position:
            # T backward passes over the SAME forward state, pass t seeded at slot t alone (the other slots' weights are 0, so their rows of
            # the gradient are exactly 0): the backward writes temporaries and gradient buffers only, never a buffer the forward stashed
            # (logit / logprob do not depend on the weights; one more head pass is not run for them)
            each = torch.empty(B, T, S, device=dev, dtype=torch.float32)
            for t in range(T):
                sp["w"] = span.w_each[t]
                G = backward(fw, idx, False, frozenset(), None, None)[0]
                each[:, t] = ops.readout(emb, G).view(B, S)
            return dict(head(), R_tok_each=each, R_tok=each.sum(1)), G
    elif idx is None:
        idx, _ = ops.argmax_rows(fw["logits"])
    hs = HeadSink(heads, nL, B, S, c["n_heads"], c["head_dim"], dev, rope_scale) if heads else None
    am = AttnMapSink(attn_map, nL, B, S, c["n_heads"], c["n_kv"], c["head_dim"], attn_scale, dev) if attn_map[0] or attn_map[1] else None
    G, layer_R, lat = backward(fw, idx, layer_relevance or "trace" in latent, latent, hs, am)
    if span is None:
        out = explanation(emb, G, idx, fw["logits"], B, S, return_G)
    else:          # (no logits: R V fp32 is hundreds of MB at a 128 k vocabulary)
        out = dict(head(), R_tok=ops.readout(emb, G).view(B, S))
        if return_G:
            out["G_emb"], out["emb"] = G.view(B, S, -1).clone(), emb.view(B, S, -1)
    return readout_outputs(out, B, S, layer_R, lat, layer_relevance, "trace" in latent, hs, am, dev, None if span is None else span.rows), G


def generate_cached(drv, embed, prefill_kv, graph_key, input_ids, max_new_tokens, lengths, eos_token_id, pad_token_id, graph, return_logits,
                    inputs_embeds, force_tokens, do_sample, temperature, top_k, top_p, min_p, seed, repetition_penalty=1.0, presence_penalty=0.0,
                    frequency_penalty=0.0, logit_bias=None):
    """the body of the drivers' generate() (its arguments and its dict): the requests, the prefill -- the forward explain() runs --, the KV
    caches [L, B, cap, nk d] of the arena with the prefill's rows copied in, cap = S + max_new_tokens, and the token loop on
    drv._decode_step, eager or one GraphCache graph per graph_key(B, cap).  The driver supplies that key, embed(ids [n]) -> its embedding
    rows [n, H] and prefill_kv(st) -> (rotated K rows [B S, nk d], V rows) of one layer's forward stash.  Every ValueError is raised before
    a kernel runs and before the driver's device, arena or weights are looked at"""
    c = drv.cfg
    ids, lens, eos, pad = generate_request(input_ids, inputs_embeds, max_new_tokens, lengths, eos_token_id, pad_token_id, c["vocab"], drv.max_seq)
    B, S = ids.shape
    sampler = sample_request(do_sample, temperature, top_k, top_p, min_p, seed, B, force_tokens)
    spec = penalty_request(repetition_penalty, presence_penalty, frequency_penalty, logit_bias, c["vocab"], force_tokens)
    dev, ar, L, nkd, nq, d = drv.device, drv._arena, len(drv.layers), c["n_kv"] * c["head_dim"], c["n_heads"], c["head_dim"]
    cap = S + max_new_tokens
    forced = force_request(force_tokens, B, max_new_tokens, c["vocab"], dev)
    _, _, _, row_iv, _ = explain_inputs(ids, None, None if lengths is None else lens, None, c["vocab"], drv.max_seq, drv.dtype, dev)
    ids = ids.to(dev)
    fw = drv.forward(embed(ids.reshape(-1)), B, S, row_iv)
    kc, vc = ar.new("kcache", L, B, cap, nkd), ar.new("vcache", L, B, cap, nkd)
    for li, st in enumerate(fw["stash"]):
        k, v = prefill_kv(st)
        kc[li, :, :S].copy_(k.view(B, S, nkd))
        vc[li, :, :S].copy_(v.view(B, S, nkd))
    lo = ar.get("dec_lo", (B,), torch.int32).copy_(S - lens)
    ws = ar.get("dec_ws", (ops.attn_decode_ws(B, nq, d, cap),), torch.uint8)
    cols = torch.arange(S, cap, device=dev, dtype=torch.int32)          # cols[t - 1: t]: the column of step t's input token
    if graph:
        step = lambda tok, pos: drv._graphs(graph_key(B, cap), lambda t_, p_: drv._decode_step(t_, p_, lo, kc, vc, ws), tok, pos)      # noqa: E731
    else:
        step = lambda tok, pos: drv._decode_step(tok, pos, lo, kc, vc, ws)      # noqa: E731
    kw = {}
    if spec is not None:          # the history of the prompt (its pads are none), one table and one processed-logits buffer per call
        V = c["vocab"]
        hist = ops.token_hist_init(ids, lo, V, hist=ar.get("pen_hist", (B, V), torch.int32))
        kw["penalty"] = PenaltyState(spec, hist, ar.get("pen_logits", (B, V), torch.float32), None if spec.bias is None else spec.bias.to(dev))
    return greedy_decode(fw["logits"], step, cols, ids, lens, max_new_tokens, eos, pad, forced, return_logits, sampler=sampler, **kw)


def explain_answer(drv, input_ids, max_new_tokens, lengths, eos_token_id, pad_token_id, graph, objective, position_weights, do_sample,
                   temperature, top_k, top_p, min_p, seed, readout_kw, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                   logit_bias=None):
    """the body of the drivers' explain_generated(): drv.generate(), then drv.explain() on the rows that predict the new tokens
    (generated_span) -> explain's dict plus sequences, new_tokens, n_new"""
    out = drv.generate(input_ids, max_new_tokens, lengths, eos_token_id, pad_token_id, graph=graph, do_sample=do_sample,
                       temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p, seed=seed, repetition_penalty=repetition_penalty,
                       presence_penalty=presence_penalty, frequency_penalty=frequency_penalty, logit_bias=logit_bias)
    positions, w = generated_span(out, position_weights)
    res = drv.explain(out["sequences"], lengths=out["lengths"], positions=positions, position_weights=w, objective=objective, **readout_kw)
    res.update(sequences=out["sequences"], new_tokens=out["new_tokens"], n_new=out["n_new"])
    return res


class LlamaLRP:
    """Device-resident weights (each ONCE, forward layout, one flat buffer) + explain().  weight_format="mxfp4": the four Linears of every
    layer are resident as MXFP4 codes + scales only (`flat_q`) and dequantised layer by layer into one scratch layer."""

    def __init__(self, cfg, W, dtype=torch.bfloat16, device="cuda", mode="efficient", max_seq=4096, sparse_top=True, fold_norm=None,
                 weight_format=None, rule="attnlrp"):
        self.rule = cp_request(rule, mode, dtype=dtype, head_dim=cfg.get("head_dim"))
        self.weight_format = weight_format_request(weight_format, cfg)
        if not torch.cuda.is_available():
            raise RuntimeError("LlamaLRP needs a HIP device: the LRP kernels have no CPU fallback")
        self.cfg, self.dtype, self.device = dict(cfg), dtype, torch.device(device)
        self._arena = Arena(self.device, dtype)
        self._graphs = GraphCache(self.device, lambda: self._arena.gen)
        self.set_mode(mode)
        # top-layer sparsity: above the last attention layer only the LAST token of a prompt feeds the
        # explained logit and carries relevance, so the last layer's o-proj / MLP (forward and backward) and
        # its attention rows are evaluated for one row per prompt (M = B instead of B*S)
        self.sparse_top = bool(sparse_top)
        self.act = cfg.get("act", "silu")
        dev = self.device
        # fold_norm (default: the bf16 engine): the weights of the two per-layer RMSNorms are multiplied into the COLUMNS of the Linears that
        # consume them (W'qkv = Wqkv diag(w1), W'gu = Wgu diag(w2)) and replaced by ones -- the same network (w (.) x rstd) W^T = (x rstd) W'^T,
        # and the same relevance under every rule of both placements: a contribution x_i w_ji of the eps-rule is unchanged, the norm's
        # identity rule does not see its weight.  What it buys: the norm is then a pure row scale, which commutes with the Linear --
        # rstd (.) (h W'^T) -- so for M = B S rows the efficient placement runs it inside the GEMM epilogues (K1n, _norm_fused below).
        self.folded = bool(dtype == torch.bfloat16 if fold_norm is None else fold_norm)
        self._nf_cache = {}                 # (row count, A/B knobs) -> fused_layer_ok

        # ONE flat device buffer holds every weight in its forward layout (embedding, norms, LM head, per layer the fused
        # [q;k;v] and [gate;up] matrices, o, down): the tensors below are views into it, so the multi-GPU start-up is a
        # single broadcast of `self.flat` (lxt_amd.dist.broadcast_weights) followed by the LOCAL W^T copies
        nq, hd = cfg["n_heads"], cfg["head_dim"]
        self.meta = (nq, cfg["n_kv"], hd, cfg["rms_eps"], self.act, hd ** -0.5)      # (the layer description of the fused-layer functions above)
        # weight_format="mxfp4": the four Linears of every layer live ONLY as e2m1 codes + e8m0 scales in the uint8 buffer flat_q (0.27 of
        # their bf16 bytes); embedding, LM head, norms and biases stay in `flat`.  ONE scratch layer in the model dtype, at fused_layout's
        # pitches, allocated once (stable addresses for graph capture): every layer's dict points its four matrices at it, a layer is loaded
        # through it (_put_layer as ever, then the quantiser) and dequantised into it in front of its forward and its backward (_load_layer),
        # so fused_layer_ok, the pitches and every kernel dispatch see what they see without it
        self.flat_q = self.scratch = self._qlayers = None
        top_spec, layer_spec = self.flat_layout(cfg, dtype)
        if self.weight_format is None:
            self.flat, top, self.layers = pack_flat(top_spec, layer_spec, len(W["layers"]), dtype, dev)
        else:
            rest, lin, qspec = quant_layout(layer_spec)
            self.flat, top, self.layers = pack_flat(top_spec, rest, len(W["layers"]), dtype, dev)
            self.flat_q, _, self._qlayers = pack_flat({}, qspec, len(W["layers"]), torch.uint8, dev, align=128)
            self.scratch, _, (views,) = pack_flat({}, lin, 1, dtype, dev)
            self.scratch.zero_()                  # (the pitch padding is never written: the load's finiteness check reads the whole buffer)
            for Lw in self.layers:
                Lw.update(views)
        self.embed, self.norm = put_rows(top["embed"], W["embed"]), put_rows(top["norm"], W["norm"])
        self.lm_head = put_rows(top["lm_head"], W["lm_head"]) if "lm_head" in top else self.embed      # (cfg["tied"]: one stored copy serves both)
        self.lm_head_t = None                        # [H, V] copy, made on the first dense-seed explanation
        for li, (Lw, L) in enumerate(zip(self.layers, W["layers"])):
            self._put_layer(Lw, L)
            if self.flat_q is not None:
                self._quantize_layer(li)
        self.attn_t = ops.attn_needs_transposed(self.embed, hd)
        inv = cfg.get("inv_freq")                    # scaled rope types: HF's own frequencies (config_from_hf)
        if inv is None:
            inv = 1.0 / (cfg["rope_theta"] ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
        self.cos, self.sin = rope_tables(inv, float(cfg.get("attention_scaling", 1.0)), max_seq, dtype, dev)
        self.max_seq = max_seq
        torch.cuda.synchronize(dev)

    def _put_layer(self, Lw, L):
        """one layer's weights L (the caller's tensors) into its views Lw of the flat buffer"""
        for k in ("ln1", "ln2", "wo", "wd") + (("qn", "kn") if "qn" in Lw else ()):
            put_rows(Lw[k], L[k])
        if "bqkv" in Lw:
            put_rows(Lw["bqkv"], L["bq"], L["bk"], L["bv"])
        put_rows(Lw["wqkv"], L["wq"], L["wk"], L["wv"])
        put_gate_up(Lw["wgu"], L["wg"], L["wu"])
        if self.folded:          # (in place, on the weights as stored: the product sees the storage dtype's rounding of W)
            fold_rows(Lw["wqkv"], (Lw["wqkv"],), L["ln1"])
            fold_rows(Lw["wgu"], (Lw["wgu"],), L["ln2"])
            Lw["ln1"].fill_(1.0)
            Lw["ln2"].fill_(1.0)

    def _quantize_layer(self, li):
        """the scratch layer, as _put_layer has just left it (fused rows, interleave, folded norms) -> layer li's codes and scales"""
        if not bool(torch.isfinite(self.scratch).all()):
            raise ValueError(f"weight_format={self.weight_format!r}: layer {li} holds non-finite weights")
        Lw, Q = self.layers[li], self._qlayers[li]
        for k in MX_MATRICES:
            ops.mxfp4_quantize(Lw[k], Q[k + "_c"], Q[k + "_s"])

    def _load_layer(self, li, only=MX_MATRICES):
        """weight_format="mxfp4": layer li's four Linears, dequantised into the scratch layer on the current stream -- in front of the layer's
        forward and of its backward, each matrix once per layer and pass (capturable: kernel launches only); nothing otherwise.  The W^T
        copies ops.weight_t caches on a weight (fp32 parity engine, odd shapes) are keyed on the scratch: dropped at every load.
        only: the subset of MX_MATRICES to load (the decode step: the matrices it does not read as codes); an empty one launches nothing"""
        if self.flat_q is None or not only:
            return
        Lw, Q = self.layers[li], self._qlayers[li]
        for k in MX_MATRICES:
            if k in only:
                ops.mxfp4_dequant(Q[k + "_c"], Q[k + "_s"], Lw[k])
        ops.clear_weight_cache(self.scratch)

    def weight_bytes(self):
        """exact bytes of device memory the weights hold: resident -- `flat` (+ `flat_q`); scratch -- the one scratch layer of a quantised engine"""
        nb = lambda t: 0 if t is None else t.numel() * t.element_size()      # noqa: E731
        return dict(resident=nb(self.flat) + nb(self.flat_q), scratch=nb(self.scratch))

    def dequantized_weights(self):
        """-> (cfg, W) in the form LlamaLRP(cfg, W) takes, holding what this engine computes with: the Linears dequantised (q / k / v split,
        gate / up de-interleaved), the norm vectors as stored -- ones when folded, so an ordinary engine built from it folds by exactly 1.0 and
        ends up with the same bits in its matrices.  Copies on the device, the whole model in the model dtype: for checks, not for serving"""
        c = self.cfg
        nq, nk, d, I = c["n_heads"], c["n_kv"], c["head_dim"], c["inter"]
        W = dict(embed=self.embed.clone(), norm=self.norm.clone(), layers=[])
        if self.lm_head is not self.embed:
            W["lm_head"] = self.lm_head.clone()
        for li, Lw in enumerate(self.layers):
            self._load_layer(li)
            wq, wk, wv = (t.clone() for t in Lw["wqkv"].split((nq * d, nk * d, nk * d), 0))
            gu = Lw["wgu"].unflatten(0, (I // ops.GATED_IL, 2, ops.GATED_IL))
            L = dict(ln1=Lw["ln1"].clone(), ln2=Lw["ln2"].clone(), wq=wq, wk=wk, wv=wv, wo=Lw["wo"].clone(),
                     wg=gu[:, 0].reshape(I, -1).clone(), wu=gu[:, 1].reshape(I, -1).clone(), wd=Lw["wd"].clone())
            if "bqkv" in Lw:
                L["bq"], L["bk"], L["bv"] = (t.clone() for t in Lw["bqkv"].split((nq * d, nk * d, nk * d), 0))
            if "qn" in Lw:
                L.update(qn=Lw["qn"].clone(), kn=Lw["kn"].clone())
            W["layers"].append(L)
        torch.cuda.synchronize(self.device)
        return dict(c), W

    # ops.linear_fwd / ops.linear_dgrad pick the kernel by row count: W-streaming small-M kernels and the split-K skinny path for the
    # one-row-per-prompt top layer and the LM head, the 256x256 ping-pong GEMM (NT forward, NN backward) for M = B*S rows
    def _lin_fwd(self, x, W, out):
        return ops.linear_fwd(x, W, out=out)

    def _decode_served(self, B):
        """the matrices of MX_MATRICES a decode step at B rows reads as codes (ops.linear_stream_fwd_q): a quantised
        bf16 engine, and per matrix the quantised stream kernel serves the step's operand AND the scratch matrix would take the plain stream
        kernel (ops.linear_fwd's rule), so the step's bits are those of the dequantise-then-stream path.  Every layer has the same shapes,
        pitches and alignment: layer 0 decides.  Empty for an unquantised or fp32 engine, tiny models, B > 128"""
        if self.flat_q is None or self.dtype != torch.bfloat16 or not self.layers or B > ops.SKINNY_MAX:
            return frozenset()
        c, ar = self.cfg, self._arena
        x, o, m = ar.new("dec_x", B, c["hidden"]), ar.new("dec_o", B, c["n_heads"] * c["head_dim"]), ar.new("dec_m", B, c["inter"])
        Lw, Q = self.layers[0], self._qlayers[0]
        return frozenset(k for k, a in (("wqkv", x), ("wo", o), ("wgu", x), ("wd", m))
                         if ops.linear_stream_q_ok(a, Q[k + "_c"], Q[k + "_s"]) and ops.linear_stream_ok(a, Lw[k]))

    def _lin_bwd(self, A, W, out):
        return ops.linear_dgrad(A, W, out=out)

    def _fused(self, M):
        """fused_layer_ok of this engine's layers at M rows (every layer has the same shapes and pitches)"""
        return fused_layer_ok(M, self.layers[0], self.meta, self.dtype, self._nf_cache) if self.layers else FusedOk(False, False, False, False)

    @staticmethod
    def _qk_norm(Lw):
        """(q_norm, k_norm) weights [d] of a layer that has them (QwenLRP's Qwen3 layers), else None"""
        return (Lw["qn"], Lw["kn"]) if "qn" in Lw else None

    def _gated_coef(self, M):
        """the gated-MLP rules run as a coefficient stash inside the two GEMMs around them (ops.gemm_gated_fwd_coef / _bwd_coef) at this row count"""
        return self._fused(M).coef

    def _norm_fused(self, M, fwd_only=False):
        """K1n applies: folded norm weights, efficient placement (no stabiliser on the residual add / the Linears: eps = 0), and every GEMM on
        both sides of the two norms is a problem the ping-pong kernel's fused epilogues take (bf16, >= 190 tiles, N % 256 == 0).  fwd_only: the
        FORWARD half is the same computation under both placements (the explicit one additionally keeps each Linear's own output: round 6)"""
        return bool(self.folded and ops.NORM_FUSION and (self.mode == "efficient" or fwd_only) and self._fused(M).norm)

    def _alloc(self, li, keep=()):
        """arena allocator of the fused-layer functions for layer li (the gradient a layer hands down alternates between two buffers); keep:
        scratch tags that get a buffer of their own per layer instead (latent "mlp": m)"""
        def alloc(tag, rows, cols, pad, dtype):
            key = tag if tag in FUSED_SCRATCH and tag not in keep else ("Gs", li & 1) if tag == "Gh" else (tag, li)
            return self._arena.get(key, (rows, cols), dtype, pad=pad)
        return alloc

    def build_transposes(self):
        """kept for callers of the round-2 API (bench.py, dist tests): the bf16 engine holds no W^T copies any more; the fp32 parity
        engine makes them lazily (ops.weight_t, cached on the weight) -- dropping the cache here makes a weight broadcast visible"""
        for L in self.layers:
            ops.clear_weight_cache(L["wqkv"], L["wo"], L["wgu"], L["wd"])
        self.lm_head_t = None

    @staticmethod
    def flat_layout(cfg, dtype):
        """(shape, row pitch) of the weights in `flat` (pack_flat): the model-wide ones, then one layer's; the Linears at fused_layout's pitches.
        Optional cfg keys of the dense Qwen driver (engine_qwen.QwenLRP; absent = the Llama layout): tied -- no lm_head copy; qkv_bias -- the
        concatenated [bq; bk; bv]; qk_norm -- the per-head q / k norm weights [d]"""
        H, I, nq, nk, d, V = cfg["hidden"], cfg["inter"], cfg["n_heads"], cfg["n_kv"], cfg["head_dim"], cfg["vocab"]
        pt = fused_layout(H, I, nq, nk, d, dtype)
        top = dict(embed=((V, H), None), lm_head=((V, H), None), norm=((H,), None))
        layer = dict(ln1=((H,), None), ln2=((H,), None), wqkv=(((nq + 2 * nk) * d, H), pt["Wqkv"]), wo=((H, nq * d), None),
                     wgu=((2 * I, H), pt["Wgu"]), wd=((H, I), pt["Wd"]))
        if cfg.get("tied"):
            del top["lm_head"]
        if cfg.get("qkv_bias"):
            layer["bqkv"] = (((nq + 2 * nk) * d,), None)
        if cfg.get("qk_norm"):
            layer.update(qn=((d,), None), kn=((d,), None))
        return top, layer

    @classmethod
    def from_hf(cls, model, **kw):
        cfg, W = weights_from_hf(model)
        kw.setdefault("dtype", next(model.parameters()).dtype)
        return cls(cfg, W, **kw)

    def set_mode(self, mode):
        if mode not in ("explicit", "efficient"):
            raise ValueError(f"mode must be 'explicit' or 'efficient', got {mode!r}")
        cp_request(getattr(self, "rule", "attnlrp"), mode)
        self.mode = mode
        self._graphs.clear()
        self.eps = dict(EXPLICIT if mode == "explicit" else EFFICIENT)
        # identity rule (*) gate Linear eps: act/(g+eps_lin) in explicit form, act/(g+1e-10) efficient
        self.eps_g = self.eps["lin"] if mode == "explicit" else self.eps["act"]

    def set_rule(self, rule):
        """"attnlrp" (the default: AttnLRP on every path, as without the keyword) or "cp" (CP-LRP, DESIGN.md section 25: q, k and the MLP's
        gate detached; engine_cp.cp_layer_bwd is then every layer's backward).  The forward, the logits and generate() do not depend on it"""
        cp_request(rule, self.mode, dtype=self.dtype, head_dim=self.cfg.get("head_dim"))
        if rule == "cp" and type(self).forward is not LlamaLRP.forward:
            raise ValueError(f'rule="cp" is served by the dense Llama / Qwen drivers, not by {type(self).__name__}')
        self.rule = rule
        self._graphs.clear()

    # ---------------------------------------------------------------------------------------------
    def release(self):
        """drop the arena (and the captured graphs that point into it)"""
        self._arena = Arena(self.device, self.dtype)
        self._graphs.clear()

    def forward(self, emb, B, S, row_iv=None, keep_m=False, rows=None, cp=False):
        """keep_m: every dense layer's m (the down projection's input) in a buffer of its own, ("m", li), for the latent "mlp" read-out;
        the arithmetic is the same, only where m lands changes.  rows int64 [R] (explain(positions=...)): the explained rows of the
        [B S, .] activations in place of each prompt's last one; the top layer then runs dense like every other layer.  cp: the forward a
        CP-LRP backward reads (engine_cp): the same network with every layer's pre-activations gu stored -- no coefficient stash and no
        fused layer (which stashes coefficients)"""
        c = self.cfg
        H, I, d, nq, nk = c["hidden"], c["inter"], c["head_dim"], c["n_heads"], c["n_kv"]
        M = B * S
        dev = self.device
        nqk, nqkv = (nq + nk) * d, (nq + 2 * nk) * d
        scale = d ** -0.5
        ar = self._arena
        stash = []
        h_prev, branch = emb, None
        last = torch.arange(B, device=dev) * S + (S - 1) if rows is None else rows
        coef = self._gated_coef(M) and not cp
        explicit = self.mode == "explicit"
        nf = not cp and self._norm_fused(M, fwd_only=True) and ops.norm_fusion_part("fwd")          # K1n: the two norms + residual sums of a layer inside the GEMM epilogues around them
        ready = None                      # (h, rstd1) of this layer, left by the previous layer's down-projection epilogue
        nL = len(self.layers)
        for li, Lw in enumerate(self.layers):
            self._load_layer(li)
            st = {}
            top = self.sparse_top and li == nL - 1 and rows is None
            if ready is not None:
                st["h"], st["rstd1"] = ready
                ready = None
                qkv, qkr, *hn = fused_qkv_fwd(st["h"], st["rstd1"], Lw["wqkv"], self.cos, self.sin, S, self.meta, self._alloc(li), explicit,
                                              Lw.get("bqkv"), self._qk_norm(Lw))
                st.update(zip(("rstd_q", "rstd_k"), hn))
            else:
                x, st["rstd1"] = ar.new("x", M, H), ar.f32(("rstd1", li), M)
                if branch is None:
                    st["h"] = h_prev
                    ops.add_rmsnorm_fwd(h_prev, None, Lw["ln1"], c["rms_eps"], y=x, rstd=st["rstd1"])
                else:
                    st["h"] = ar.new(("h", li), M, H)
                    ops.add_rmsnorm_fwd(h_prev, branch, Lw["ln1"], c["rms_eps"], hsum_out=st["h"], y=x, rstd=st["rstd1"])
                qkv, qkn = ops.linear_fwd(x, Lw["wqkv"], Lw.get("bqkv"), out=ar.new(("qkv", li), M, nqkv)), self._qk_norm(Lw)
                if qkn is not None:      # (QwenLRP: the per-head q / k norm between the projection and RoPE)
                    qn = ar.new("qkn", M, nqk)
                    st["rstd_q"], st["rstd_k"] = ar.f32(("rstd_q", li), M * nq), ar.f32(("rstd_k", li), M * nk)
                    ops.head_rmsnorm_fwd(qkv[:, : nq * d], qkn[0], qn[:, : nq * d], st["rstd_q"], nq, d, c["rms_eps"])
                    ops.head_rmsnorm_fwd(qkv[:, nq * d: nqk], qkn[1], qn[:, nq * d:], st["rstd_k"], nk, d, c["rms_eps"])
                qkr = ops.rope_fwd(qkv if qkn is None else qn, ar.new(("qkr", li), M, nqk), self.cos, self.sin, S, nq + nk, d)
            if nf and not top:
                # (not chained in the last layer: the tail below wants h1 and dn of the explained rows separately)
                st.update(fused_layer_fwd(st["h"], st["rstd1"], qkv, qkr, Lw, self.cos, self.sin, B, S, self.meta,
                                          self._alloc(li, ("m",) if keep_m else ()), row_iv, explicit,
                                          (self.eps_g, self.eps["lin"]), chain=li + 1 < nL), qkv=qkv, qkr=qkr, coef=True)
                stash.append(st)
                ready = (st["h_out"], st["rstd_out"]) if li + 1 < nL else None
                h_prev, branch = st["h1"], st["dn"]             # (read after the last layer only)
                continue
            v = qkv[:, nqk:]
            v_t = ops.transpose_heads(v, B, S, nk, d) if self.attn_t else None
            o = ar.new(("o", li), M, nq * d)
            lse = ar.f32(("lse", li), B, nq, S)
            if top:
                ops.attn_fwd(qkr[:, : nq * d], qkr[:, nq * d:], v, v_t, o, lse, B, S, nq, nk, d, scale, True, 0, q_begin=S - 1, row_iv=row_iv)
                o_l, h_l = o.index_select(0, last), st["h"].index_select(0, last)
                a_l = self._lin_fwd(o_l, Lw["wo"], ar.new("a_l", B, H))
                h1_l = ar.new("h1_l", B, H)
                x2_l, rstd2_l = ops.add_rmsnorm_fwd(h_l, a_l, Lw["ln2"], c["rms_eps"], hsum_out=h1_l)
                gu_l, m_l = ops.gemm_gated_fwd(x2_l, Lw["wgu"], ar.new("gu_l", B, 2 * I), ar.new("m_l", B, I), self.act)
                dn_l = self._lin_fwd(m_l, Lw["wd"], ar.new("dn_l", B, H))
                st.update(top=True, qkv=qkv, qkr=qkr, lse=lse, o_l=o_l, a_l=a_l, h1_l=h1_l, rstd2_l=rstd2_l, gu_l=gu_l, m_l=m_l, dn_l=dn_l)
                stash.append(st)
                h_prev, branch = h1_l, dn_l
                break
            ops.attn_fwd(qkr[:, : nq * d], qkr[:, nq * d:], v, v_t, o, lse, B, S, nq, nk, d, scale, True, 0, row_iv=row_iv)
            a = self._lin_fwd(o, Lw["wo"], ar.new(("a", li), M, H))
            h1 = ar.new(("h1", li), M, H)
            x2, st["rstd2"] = ar.new("x2", M, H), ar.f32(("rstd2", li), M)
            ops.add_rmsnorm_fwd(st["h"], a, Lw["ln2"], c["rms_eps"], hsum_out=h1, y=x2, rstd=st["rstd2"])
            gu, m = ar.new(("gu", li), M, 2 * I), ar.wide(("m", li) if keep_m else "m", M, I)
            if coef:      # the gated rules inside the two GEMMs around them: the backward's coefficients are stashed in gu's place (g, u never stored)
                gu, m = ops.gemm_gated_fwd_coef(x2, Lw["wgu"], gu, m, self.eps_g, self.eps["lin"], self.act)
            else:
                gu, m = ops.gemm_gated_fwd(x2, Lw["wgu"], gu, m, self.act)
            dn = self._lin_fwd(m, Lw["wd"], ar.new(("dn", li), M, H))
            st.update(qkv=qkv, qkr=qkr, o=o, lse=lse, a=a, h1=h1, gu=gu, coef=coef, m=m, dn=dn)
            stash.append(st)
            h_prev, branch = h1, dn
        # last token only: final residual add + norm + LM head
        top = bool(stash) and stash[-1].get("top", False)
        return dict(stash=stash, last=last, row_iv=row_iv, **head_fwd(ar, h_prev, branch, top, last, self.norm, self.lm_head, c["rms_eps"]))

    def _head_bwd(self, fw, idx, seed, layer_relevance):
        """LM head eps rule + final-norm identity rule on the single explained row of each prompt, then add2 at h_L = h1 + dn and the eps scale
        of the last down_proj, still one row per prompt -> (Gh_last, Gs_last, A_last, rel_last or None).  fw["span"] (explain(positions=...)):
        the same on the R = B T explained rows, seeded by lrp_span_seed"""
        E, H, ar = self.eps, self.cfg["hidden"], self._arena
        Gh_last = head_seed_bwd(ar, fw, idx, self.norm, self.lm_head, E["lin"], seed=seed)
        R = Gh_last.shape[0]
        # add2 at h_L = h1 + dn and the eps scale of the last down_proj, still one row per prompt
        Gs_last, A_last = ar.new("Gs_last", R, H), ar.new("A_last", R, H)
        rel_last = ar.f32("rel_last", R) if layer_relevance else None
        ops.rmsnorm_bwd_add2(Gh_last, None, None, None, fw["hL_last"], fw["dn_last"], Gs_last, A_last, rel_last,
                             0.0, E["add"], E["lin"])
        return Gh_last, Gs_last, A_last, rel_last

    # ---------------------------------------------------------------------------------------------
    def backward(self, fw, emb, idx, B, S, layer_relevance=False, seed=None, latent=frozenset(), heads=None, attn_map=None, weights=None):
        """-> (G at the embedding, layer_R rows or None, dict of the token-summed latent read-outs: R_resid [L+1, B, H] / R_mlp [L, B, I]);
        heads: a HeadSink that collects the per-head read-outs layer by layer, or None; attn_map: an AttnMapSink, likewise; weights: a
        WeightSink, likewise (the forward then ran with keep_m when "down" is asked for)"""
        c, E = self.cfg, self.eps
        H, I, d, nq, nk = c["hidden"], c["inter"], c["head_dim"], c["n_heads"], c["n_kv"]
        M, rep = B * S, nq // nk
        dev, dt = self.device, self.dtype
        nqk, nqkv = (nq + nk) * d, (nq + 2 * nk) * d
        scale = d ** -0.5
        ar = self._arena
        Gh_last, Gs_last, A_last, rel_last = self._head_bwd(fw, idx, seed, layer_relevance)
        nL, lat = len(self.layers), {}
        if "resid" in latent:          # index L: the head's explained rows, the gradient rel_last is formed from (S = 1)
            lat["R_resid"] = torch.empty(nL + 1, B, H, device=dev, dtype=torch.float32)
            ops.colsum_dot(fw["hL_last"], Gh_last, B, fw["last"].shape[0] // B, out=lat["R_resid"][nL])      # (a prompt's explained rows, in slot order)
        if "mlp" in latent:
            lat["R_mlp"] = torch.empty(nL, B, I, device=dev, dtype=torch.float32)
        last, row_iv = fw["last"], fw["row_iv"]
        top_sparse = bool(fw["stash"]) and fw["stash"][-1].get("top", False)
        if not top_sparse:
            Gs = ar.zeros(("Gs", len(self.layers) & 1), M, H).index_copy_(0, last, Gs_last)
            Adn = ar.zeros(("Adn", len(self.layers) & 1), M, H).index_copy_(0, last, A_last)
        layer_R = [rel_last] if layer_relevance else None
        plain_add = E["add"] == 0.0 and E["lin"] == 0.0          # efficient placement: add2 / Linear eps factors are exactly 1
        nfb = plain_add and self._norm_fused(M)                  # K1n in the backward (independent of what the forward ran: both need only rstd)
        full = nfb and self._fused(M).full                       # dense layers: fused_layer_bwd; below, the partial forms (A/B knobs, explicit)
        # attn_bwd_prep folded away (efficient placement, the bf16 kernels that take every operand token-major, M = B S rows)
        fuse_prep = plain_add and E["pv"] == 0.0 and E["mask"] == 0.0 and E["qk"] == 0.0 and not self.attn_t and self._fused(M).prep
        half = ar.f32("half", M).fill_(0.5) if fuse_prep else None              # (fused_layer_bwd reads it too)
        fuse_rope = fuse_prep and ops.ROPE_BWD_FUSION and E["rope"] == 0.0 and E["lin"] == 0.0 and d in (64, 128) and S <= self.max_seq

        def normed(x, rstd, ln, tag):
            """(X, rs) of a Linear behind an RMSNorm for the WeightSink: folded norm weights are ones, so the un-normed stream with rs = rstd
            IS the Linear's input; otherwise the normed rows are formed once more (the forward keeps them in a scratch buffer only)"""
            if self.folded:
                return x, rstd
            y = ar.new(tag, *x.shape)
            ops.add_rmsnorm_fwd(x, None, ln, c["rms_eps"], y=y, rstd=ar.f32(tag + "_rstd", x.shape[0]))
            return y, None

        for li in range(len(self.layers) - 1, -1, -1):
            Lw, st = self.layers[li], fw["stash"][li]
            self._load_layer(li)
            qkv, qkr = st["qkv"], st["qkr"]
            q_begin = 0
            if "mlp" in latent:
                # G_m = Adn Wd: the gradient at the down projection's input (Adn: the eps-scaled branch gradient; = Gs in the efficient placement),
                # one dgrad the backward otherwise folds into Agu.  The sparse top layer has one row per prompt: the other rows' neurons are 0
                if st.get("top", False):
                    Gm = self._lin_bwd(A_last, Lw["wd"], ar.new("Gm_l", B, I))
                    ops.colsum_dot(st["m_l"], Gm, B, 1, out=lat["R_mlp"][li])
                else:
                    Gm = self._lin_bwd(Adn, Lw["wd"], ar.new("Gm", M, I))
                    ops.colsum_dot(st["m"], Gm, B, S, out=lat["R_mlp"][li])
            hs = None if heads is None else heads.layer(li)
            am = None if attn_map is None else attn_map.layer(li)
            ws = None if weights is None else weights.layer(li)
            if self.rule == "cp":
                rel = ar.f32(("rel", li), M) if layer_relevance else None
                Gs = Adn = cp_layer_bwd(self, li, st, Lw, None if st.get("top", False) else Gs, B, S, row_iv,
                                        (Gs_last, A_last, last) if st.get("top", False) else None, Gm if "mlp" in latent else None, rel)
                layer_R = layer_R + [rel] if layer_relevance else None
                if "resid" in latent:
                    ops.colsum_dot(st["h"], Gs, B, S, out=lat["R_resid"][li])
                continue
            if full and not st.get("top", False):          # (Adn = Gs: eps = 0)
                Gs = Adn = fused_layer_bwd(Gs, st, Lw, self.cos, self.sin, B, S, self.meta, self._alloc(li), row_iv, self._qk_norm(Lw), hs, am, ws)
                layer_R = layer_R + [ops.readout(st["h"], Gs, out=ar.f32(("rel", li), M))] if layer_relevance else None
                if "resid" in latent:
                    ops.colsum_dot(st["h"], Gs, B, S, out=lat["R_resid"][li])
                continue
            if st.get("top", False):
                # ---- one row per prompt through MLP, norm/add2 and o-proj; scatter into the dense attention inputs
                gu_l = st["gu_l"]
                Agu = ops.gemm_gated_bwd(A_last, Lw["wd"], gu_l, ar.new("Agu_l", B, 2 * I), self.eps_g, E["lin"], self.act)
                Gx2 = self._lin_bwd(Agu, Lw["wgu"], ar.new("Gx2_l", B, H))
                Gs1_l, Aa_l = ar.new("Gs1_l", B, H), ar.new("Aa_l", B, H)
                ops.rmsnorm_bwd_add2(Gs_last, Gx2, Lw["ln2"], st["rstd2_l"], st["h1_l"], st["a_l"], Gs1_l, Aa_l, None, 0.0,
                                     E["add"], E["lin"])
                Gof_l = self._lin_bwd(Aa_l, Lw["wo"], ar.new("Gof_l", B, nq * d))
                if ws is not None:          # one row per prompt: every other token's contribution to these three matrices is exactly 0
                    ws("down", A_last, st["m_l"], Lw["wd"])
                    x2w, rs2 = normed(st["h1_l"], st["rstd2_l"], Lw["ln2"], "x2w_l")
                    ws("gate_up", Agu, x2w, Lw["wgu"], rs=rs2)
                    ws("o", Aa_l, st["o_l"], Lw["wo"])
                Gho, D, Gs1 = top_attn_operands(ar, Gof_l, st["o_l"], Gs1_l, last, S, nq, d, E["pv"])
                if hs is not None:
                    hs.last("out", st["o_l"], Gof_l)
                q_begin = S - 1
            else:
                gu = st["gu"]
                # ---- MLP
                if st.get("coef", False):
                    Agu = ops.gemm_gated_bwd_coef(Adn, Lw["wd"], gu, ar.wide("Agu", M, 2 * I))
                else:
                    Agu = ops.gemm_gated_bwd(Adn, Lw["wd"], gu, ar.wide("Agu", M, 2 * I), self.eps_g, E["lin"], self.act)
                if ws is not None:
                    ws("down", Adn, st["m"], Lw["wd"])
                    x2w, rs2 = normed(st["h1"], st["rstd2"], Lw["ln2"], "x2w")
                    ws("gate_up", Agu, x2w, Lw["wgu"], rs=rs2)
                Gs1 = ar.new("Gs1", M, H)
                if nfb and ops.norm_fusion_part("bwd_gu"):               # K1n: Gs1 = rstd2 (.) (Agu W'gu) + Gs in the dgrad GEMM's epilogue
                    Aa = ops.gemm_nn_rs_res(Agu, Lw["wgu"], st["rstd2"], Gs, Gs1)
                else:
                    Gx2 = self._lin_bwd(Agu, Lw["wgu"], ar.new("Gx2", M, H))
                    if plain_add:     # no stabiliser on the add / the branch's Linear: the branch gradient IS the residual gradient
                        ops.rmsnorm_bwd_add2(Gs, Gx2, Lw["ln2"], st["rstd2"], None, None, Gs1, None, None, 0.0, 0.0, 0.0)
                        Aa = Gs1
                    else:
                        Aa = ar.new("Aa", M, H)
                        ops.rmsnorm_bwd_add2(Gs, Gx2, Lw["ln2"], st["rstd2"], st["h1"], st["a"], Gs1, Aa, None, 0.0, E["add"], E["lin"])
                if ws is not None:
                    ws("o", Aa, st["o"], Lw["wo"])
                # ---- attention
                Gho = ar.new("Gho", M, nq * d)
                D = ar.f32("D", B, nq, S)
                if fuse_prep:
                    # no attn_bwd_prep pass: Gho = 1/2 (Aa Wo) straight out of the o-projection's dgrad (row scale 1/2: exact), and the dQ
                    # kernel forms D = rowsum(Gho (*) o) from the rows it loads anyway and leaves it for the dK / dV kernel
                    ops.gemm_nn_rs(Aa, Lw["wo"], half, Gho)
                    if hs is not None:
                        hs("out", st["o"], Gho, scale=2.0)
                else:
                    Gof = self._lin_bwd(Aa, Lw["wo"], ar.new("Gof", M, nq * d))
                    ops.attn_bwd_prep(Gof, st["o"], Gho, D, B, S, nq, d, E["pv"], 0.5)
                    if hs is not None:
                        hs("out", st["o"], Gof)
            q, k, v = qkr[:, : nq * d], qkr[:, nq * d:], qkv[:, nqk:]
            if am is not None and q_begin == 0:          # (Gho = 1/2 G_o on every efficient path: the epilogue's row scale, or attn_bwd_prep's factor)
                am(q, k, v, Gho, st["lse"], 2.0, row_iv)
            elif am is not None:
                am.top(ar, q, k, v, Gho, st["lse"], 2.0, last, row_iv)
            k_t = q_t = Gho_t = None
            if self.attn_t:        # kernels that read head-transposed copies (fp32, head dims other than 128)
                k_t = ops.transpose_heads(k, B, S, nk, d)
                q_t = ops.transpose_heads(q, B, S, nq, d)
                Gho_t = ops.transpose_heads(Gho, B, S, nq, d)
            dk_h, dv_h = ar.new("dk_h", M, nq * d), ar.new("dv_h", M, nq * d)
            Aqkv = ar.get("Aqkv", (M, nqkv), dt, pad=fused_layout(H, I, nq, nk, d, dt)["Aqkv"] - nqkv)
            qkn = self._qk_norm(Lw)
            if fuse_prep and q_begin == 0 and fuse_rope and qkn is None:
                # RoPE's backward rides on the dQ store and on dK's group sum (no rope_bwd pass, no dqk round trip): both write Aqkv directly
                ops.attn_bwd_dq_d(q, k, v, Gho, st["o"], st["lse"], D, Aqkv[:, : nq * d], B, S, nq, nk, d, scale, row_iv=row_iv,
                                  rope=(self.cos, self.sin))
                ops.attn_bwd_dkv(q, k, v, None, Gho, None, st["lse"], D, dk_h, dv_h, B, S, nq, nk, d, scale, 0.0, 0.0, row_iv=row_iv)
                if hs is not None:
                    hs("q", q, Aqkv[:, : nq * d], rope=(self.cos, self.sin))
                ops.gqa_reduce_rope(dk_h, Aqkv[:, nq * d: nqk], M, S, nk, rep, d, self.cos, self.sin)
                ops.gqa_reduce(dv_h, Aqkv[:, nqk:], M, nk, rep, d)
            else:
                dqk = ar.new("dqk", M, nqk) if q_begin == 0 else ar.zeros("dqk", M, nqk)
                if fuse_prep and q_begin == 0:
                    ops.attn_bwd_dq_d(q, k, v, Gho, st["o"], st["lse"], D, dqk[:, : nq * d], B, S, nq, nk, d, scale, row_iv=row_iv)
                else:
                    ops.attn_bwd_dq(q, k, v, k_t, Gho, st["lse"], D, dqk[:, : nq * d], B, S, nq, nk, d, scale, E["mask"], E["qk"],
                                    q_begin=q_begin, row_iv=row_iv)
                ops.attn_bwd_dkv(q, k, v, q_t, Gho, Gho_t, st["lse"], D, dk_h, dv_h, B, S, nq, nk, d, scale, E["mask"], E["qk"],
                                 q_begin=q_begin, row_iv=row_iv)
                if hs is not None and q_begin == 0:
                    hs("q", q, dqk[:, : nq * d])
                elif hs is not None:          # (the sparse top layer: dq's only live rows)
                    hs.last("q", q.index_select(0, last), dqk.index_select(0, last)[:, : nq * d])
                ops.gqa_reduce(dk_h, dqk[:, nq * d:], M, nk, rep, d)
                if E["lin"] == 0.0:
                    ops.gqa_reduce(dv_h, Aqkv[:, nqk:], M, nk, rep, d)
                    Gqk = ops.rope_bwd(dqk, None, None, Aqkv[:, :nqk] if qkn is None else ar.new("Gqkn", M, nqk), self.cos, self.sin, S, nq + nk, d,
                                       0.0, 0.0)
                    if qkn is not None:      # the head norms' backward with rstd detached: a row-constant scale per head
                        ops.head_rmsnorm_bwd(Gqk[:, : nq * d], qkn[0], st["rstd_q"], Aqkv[:, : nq * d], nq, d)
                        ops.head_rmsnorm_bwd(Gqk[:, nq * d:], qkn[1], st["rstd_k"], Aqkv[:, nq * d: nqk], nk, d)
                else:
                    dv = ops.gqa_reduce(dv_h, ar.new("dv", M, nk * d), M, nk, rep, d)
                    ops.eps_scale2d(dv, v, Aqkv[:, nqk:], 1.0, E["lin"])
                    ops.rope_bwd(dqk, qkr, qkv[:, :nqk], Aqkv[:, :nqk], self.cos, self.sin, S, nq + nk, d, E["rope"], E["lin"])
            if hs is not None:
                hs("k", k, dk_h, rep)
                hs("v", v, dv_h, rep)
            if ws is not None:
                xw, rs1 = normed(st["h"], st["rstd1"], Lw["ln1"], "xw")
                ws("qkv", Aqkv, xw, Lw["wqkv"], rs=rs1)
            rel = ar.f32(("rel", li), M) if layer_relevance else None
            if nfb and ops.norm_fusion_part("bwd_qkv"):
                # K1n: Gs = rstd1 (.) (Aqkv W'qkv) + Gs1 -- the input norm's identity rule and the residual add in the qkv dgrad's epilogue.  The
                # layer relevance sum_j h_j G_j (a diagnostic) is then one read-out pass over the stored gradient: the SAME kernels serve the call
                # with and without it (a prompt's relevance must not depend on the options of the call)
                Gs = ops.gemm_nn_rs_res(Aqkv, Lw["wqkv"], st["rstd1"], Gs1, ar.new(("Gs", li & 1), M, H))
                Adn = Gs
                if layer_relevance:
                    layer_R.append(ops.readout(st["h"], Gs, out=rel))
                if "resid" in latent:
                    ops.colsum_dot(st["h"], Gs, B, S, out=lat["R_resid"][li])
                continue
            Gx = self._lin_bwd(Aqkv, Lw["wqkv"], ar.new("Gx", M, H))
            # ---- input norm + the residual add below (or the embedding)
            if li > 0:
                prev = fw["stash"][li - 1]
                Gs = ar.new(("Gs", li & 1), M, H)
                if plain_add:
                    ops.rmsnorm_bwd_add2(Gs1, Gx, Lw["ln1"], st["rstd1"], st["h"] if layer_relevance else None, None, Gs, None, rel, 0.0, 0.0, 0.0)
                    Adn = Gs
                else:
                    Adn = ar.new(("Adn", li & 1), M, H)
                    ops.rmsnorm_bwd_add2(Gs1, Gx, Lw["ln1"], st["rstd1"], st["h"], prev["dn"], Gs, Adn, rel, 0.0, E["add"], E["lin"])
            else:
                Gs = ar.new(("Gs", 0), M, H)
                ops.rmsnorm_bwd_add2(Gs1, Gx, Lw["ln1"], st["rstd1"], st["h"] if layer_relevance else None, None, Gs, None,
                                     rel, 0.0, 0.0, 0.0)
            if layer_relevance:
                layer_R.append(rel)
            if "resid" in latent:
                ops.colsum_dot(st["h"], Gs, B, S, out=lat["R_resid"][li])
        return Gs, layer_R, lat

    # ---------------------------------------------------------------------------------------------
    def _weight_sink(self, req, prev):
        """the sink that collects R_W for a weight_request (a subclass with other matrices returns its own)"""
        return WeightSink(req, self.cfg, self.device, prev)

    def _run(self, input_ids, emb, B, S, row_iv, idx, layer_relevance, return_G, seed, latent=frozenset(), heads=frozenset(), attn_map=(False, ()),
             weights=((), ()), weights_out=None, span=None, **opts):
        """forward + backward + read-out on the current stream: library launches only, no host synchronisation (capturable); opts: further
        keywords of a subclass's forward / backward (Qwen3MoeLRP: experts); span: a SpanRequest (explain(positions=...))"""
        if emb is None:
            emb = self._embed(input_ids.reshape(-1))
        wsink = self._weight_sink(weights, weights_out) if weights[0] else None
        keep_m, bopts = "mlp" in latent or "down" in weights[0], opts if wsink is None else dict(opts, weights=wsink)
        if self.rule == "cp":
            opts = dict(opts, cp=True)
        out, _ = explain_pipeline(self, lambda **rows: self.forward(emb, B, S, row_iv, keep_m=keep_m, **opts, **rows),
                                  lambda fw, i, want_R, lat, hs, am: self.backward(fw, emb, i, B, S, want_R, seed=seed, latent=lat, heads=hs,
                                                                                   attn_map=am, **bopts),
                                  emb, B, S, idx, self.meta[-1], float(self.cfg.get("attention_scaling", 1.0)) ** -2, return_G, layer_relevance,
                                  latent, heads, attn_map, span)
        if wsink is not None:
            out["R_W"], out["weight_layers"] = wsink.out, list(wsink.layers)
        return out

    @torch.no_grad()
    def explain(self, input_ids=None, inputs_embeds=None, target=None, layer_relevance=False, return_G=False, lengths=None,
                seed=None, graph=False, latent=None, heads=None, attn_map=None, weights=None, weight_layers=None, weights_out=None,
                positions=None, position_weights=None, objective="logit", per_position=False):
        """input_ids [B,S] (or inputs_embeds [B,S,H]); target: None (arg-max of the last position) or
        int tensor [B].  Returns dict(idx [B], logit [B], R_tok [B,S] fp32, and optionally
        layer_R [L+1, B] (sum_h h (*) G_h at every residual-stream boundary) and G_emb [B,S,H]).
        lengths [B] (optional): prompts of different lengths in ONE call, LEFT-padded to S (prompt b occupies columns
        S-lengths[b] .. S-1, so every prompt's explained position is still the last column).  Pad keys are masked out
        through the attention kernels' per-row key intervals; RoPE is relative, so the result equals the un-padded
        single-prompt explanation up to rounding.  R_tok is exactly 0 at pad positions.
        seed [B,V] (optional, instead of target): what the reference's protocol passes to `logits[:, -1].backward(seed)` --
        a gradient over the last-position logits in efficient mode (contrastive explanations), a relevance over them
        in explicit mode.
        graph=True (input_ids only, no lengths / seed / return_G): the ~1500 launches of one explanation of this (B, S) are captured
        once into a hipGraph and replayed; the returned tensors are the graph's static outputs (copy them before the next call).
        latent (optional): names from {"trace", "resid", "mlp"}, the latent feature attribution read-outs, each one
        more output, fp32: R_trace [L+1, B, S] = sum_h h (*) G_h per token at every residual boundary (index 0 = R_tok, index l = the output
        of layer l - 1, index L = the head's row: only each prompt's last column is non-zero; R_trace[l].sum(-1) is layer_R[l]);
        R_resid [L+1, B, H] = sum_t h (*) G_h per residual dimension at the same boundaries; R_mlp [L, B, I] = sum_t m (*) G_m per MLP neuron
        (m: the down projection's input, HF column order).  R_tok, logit and layer_R do not change with it.
        heads (optional): names from {"out", "q", "k", "v"}, the per-head attention relevance, each one more fp32
        output [L, B, n_heads, S]: R_head_out = sum_d o (*) G_o at the o projection's input, per query head and query position (and R_head
        [L, B, n_heads] = R_head_out.sum(-1): which heads of which layer carry the prediction); R_head_q / R_head_k / R_head_v = sum_d x (*) G_x
        at the attention's query / key / value input (after RoPE and Qwen3's head norm), k and v per QUERY head at the SOURCE position: which
        tokens a head pulls its relevance from.  Pad columns under lengths are exactly 0; nothing else changes with it.
        attn_map (optional): "sum", (layer, head) pairs, or an iterable mixing both -- the token-to-token attention relevance (DESIGN.md
        section 12.2) R[i, j] = P[i, j] (G_o[i] . v[j]), `attn_weights * attn_weights.grad` of eager attention: how much relevance query
        position i draws from source position j.  "sum": R_attn [L, B, S, S] fp32 over all query heads; pairs: R_attn_heads [n, B, S, S] in
        request order and attn_map_heads, the pairs.  A row sums to R_head_out (1/2 of it is the uniform-rule share of P in P V); masked and pad
        (i, j) are exactly 0; efficient placement only; nothing else changes with it.
        weights (optional): names from {"qkv", "o", "gate_up", "down"} -- the per-weight relevance `weight * weight.grad` of those decoder
        Linears: R_W[name] fp32 [len(weight_layers), N, K], summed over every token of every prompt of the call, rows in
        HF order (qkv = q_proj | k_proj | v_proj rows, gate_up = gate_proj rows then up_proj rows), and weight_layers, the layer list.
        weight_layers: ascending layer indices (default: all -- at the 8B shape all four matrices of 32 layers are ~28 GB of fp32).
        weights_out: a previous call's R_W; this call's values are added to it in place and it is returned (dataset-level accumulation).
        Efficient placement only, no graph=True; nothing else changes with it.
        positions (optional): int [B, T], T >= 1 -- answer-span attribution: T explained rows per prompt in ONE forward
        and ONE backward.  Entries are distinct column indices of the prompt's own columns (>= S - lengths[b]); row p predicts the token after
        column p (teacher forcing).  target is then [B, T]; its default is input_ids[b, p + 1], and the row's arg-max for p = S - 1 (required
        with inputs_embeds).  position_weights: fp32 [B, T], default ones; the explained scalar is sum_t w[b, t] f(b, t) (1 / T: a mean; 0:
        a spare slot of a shorter answer -- point it at any other valid column, it contributes exactly 0).  objective: "logit",
        f = logits[b, p, tgt], or "logprob", f = log_softmax(logits[b, p])[tgt] (seed delta - softmax over the row's logits).
        Returns idx, logit, logprob (all [B, T], both objectives) and R_tok [B, S], the relevance of the weighted sum; `logits` is not
        returned.  R_tok is exactly 0 at pads and at every column above max(positions[b]).  Every read-out keyword keeps working (they read
        the backward, which only sees another seed): R_trace[L] is non-zero at the explained columns, layer_R[L] and R_resid[L] sum over a
        prompt's explained rows.  The sparse top layer is not used for such a call.
        per_position=True: one forward, then T backward passes over the same forward state, pass t seeded at slot t alone -> additionally
        R_tok_each [B, T, S] fp32, the answer x prompt map, and R_tok = R_tok_each.sum(1); no read-out keyword with it.
        Efficient placement only; not with seed or graph=True (ValueError, as for every bad position, weight, target or objective, raised
        before a kernel of the model runs).  Without positions nothing changes."""
        cp_request(getattr(self, "rule", "attnlrp"), getattr(self, "mode", "efficient"), heads, attn_map, weights)
        wr = weight_request(weights, weight_layers, weights_out, self.cfg, len(getattr(self, "layers", ())), self.dtype,
                            getattr(self, "mode", "efficient"), graph)
        am = attn_map_request(attn_map, len(getattr(self, "layers", ())), self.cfg.get("n_heads", 0), self.cfg.get("head_dim"), self.dtype,
                              getattr(self, "mode", "efficient"))
        hd = head_request(heads, self.cfg.get("head_dim"), self.dtype)
        lat = latent_request(latent, self.cfg["hidden"], self.cfg["inter"], self.dtype)
        nb, ns = (input_ids.shape if inputs_embeds is None else inputs_embeds.shape[:2]) if positions is not None else (0, 0)
        span = position_request(positions, position_weights, objective, per_position, nb, ns, self.cfg["vocab"], getattr(self, "device", None),
                                input_ids if inputs_embeds is None else None, target, lengths, seed, graph, getattr(self, "mode", "efficient"),
                                bool(layer_relevance or return_G or latent or heads or attn_map or weights))
        if span is not None:
            target = None          # (checked and converted above; explain_inputs sees the plain form)
        B, S, emb, row_iv, idx = explain_inputs(input_ids, inputs_embeds, lengths, target, self.cfg["vocab"], self.max_seq, self.dtype,
                                                self.device, seed)
        if inputs_embeds is None:
            input_ids = input_ids.to(self.device)
        if not graph:
            return self._run(input_ids, emb, B, S, row_iv, idx, layer_relevance, return_G, seed, lat, hd, am, wr, weights_out, span=span)
        if emb is not None or lengths is not None or seed is not None or return_G:
            raise ValueError("graph=True takes input_ids only (no inputs_embeds / lengths / seed / return_G)")
        return self._graphs((B, S, idx is not None, bool(layer_relevance), self.mode, self.rule, tuple(sorted(lat)), tuple(sorted(hd)), am),
                            lambda ids, idx_: self._run(ids, None, B, S, None, idx_, layer_relevance, False, None, lat, hd, am), input_ids, idx)

    # --------------------------------------------------------------------------------------------- generation
    def _embed(self, ids):
        """the embedding rows [n, H] of token ids [n] on the device"""
        return self.embed.index_select(0, ids)

    def _prefill_kv(self, st):
        """(rotated K rows, V rows) [B S, nk d] of one layer's forward stash: what generate() copies into the caches"""
        nq, nk, d = self.meta[:3]
        return st["qkr"][:, nq * d:], st["qkv"][:, (nq + nk) * d:]

    def _decode_step(self, tok, pos, lo, kc, vc, ws):
        """one new token per prompt through every layer on B rows: the sparse top layer's launch sequence (embedding rows, norm, qkv, o
        projection, norm, gated MLP, down projection: the weight-streaming Linears), with lrp_decode_rope_append and lrp_attn_decode in place of
        RoPE and attention.  tok int64 [B] and pos int32 [1] (the column the token sits at) are device INPUTS of the step; nothing is
        incremented inside it, so running it again writes the same cache rows with the same values (what GraphCache's warm-up + capture do).
        kc, vc [L, B, cap, nk d];  lo int32 [B].  -> (logits [B, V] fp32, idx int32 [B] their arg-max); launches only, capturable"""
        c = self.cfg
        H, I, d, nq, nk, eps = c["hidden"], c["inter"], c["head_dim"], c["n_heads"], c["n_kv"], c["rms_eps"]
        B, ar, nqk = tok.shape[0], self._arena, (nq + nk) * d
        h, branch = self.embed.index_select(0, tok), None
        served = self._decode_served(B)          # weight_format="mxfp4": the matrices read as codes (section 22), decided once per step shape
        rest = tuple(k for k in MX_MATRICES if k not in served)

        def lin(li, k, x, out, bias=None):
            """the step's Linear on matrix k of layer li: on its codes where served, else on the scratch matrix _load_layer has filled"""
            if k in served:
                Q = self._qlayers[li]
                return ops.linear_stream_fwd_q(x, Q[k + "_c"], Q[k + "_s"], bias, out=out)
            return ops.linear_fwd(x, self.layers[li][k], bias, out=out)

        for li, Lw in enumerate(self.layers):
            self._load_layer(li, rest)    # (what is not served: one dequantisation of the matrix per token -- the price of one scratch layer)
            x, rstd = ar.new("dec_x", B, H), ar.f32("dec_rstd", B)
            if branch is None:
                ops.add_rmsnorm_fwd(h, None, Lw["ln1"], eps, y=x, rstd=rstd)
            else:
                hs = ar.new("dec_h", B, H)
                ops.add_rmsnorm_fwd(h, branch, Lw["ln1"], eps, hsum_out=hs, y=x, rstd=rstd)
                h = hs
            qkv, qkn = lin(li, "wqkv", x, ar.new("dec_qkv", B, nqk + nk * d), Lw.get("bqkv")), self._qk_norm(Lw)
            qk = qkv[:, :nqk]
            if qkn is not None:
                qk = ar.new("dec_qkn", B, nqk)
                ops.head_rmsnorm_fwd(qkv[:, : nq * d], qkn[0], qk[:, : nq * d], ar.f32("dec_rstd_q", B * nq), nq, d, eps)
                ops.head_rmsnorm_fwd(qkv[:, nq * d: nqk], qkn[1], qk[:, nq * d:], ar.f32("dec_rstd_k", B * nk), nk, d, eps)
            q = ops.decode_rope_append(qk, qkv[:, nqk:], self.cos, self.sin, pos, ar.new("dec_q", B, nq * d), kc[li], vc[li], nq, nk, d)
            o = ops.attn_decode(q, kc[li], vc[li], lo, pos, nq, nk, d, self.meta[-1], out=ar.new("dec_o", B, nq * d), ws=ws)
            a = lin(li, "wo", o, ar.new("dec_a", B, H))
            h1 = ar.new("dec_h1", B, H)
            x2, _ = ops.add_rmsnorm_fwd(h, a, Lw["ln2"], eps, hsum_out=h1, y=x, rstd=rstd)
            gu, m = ar.new("dec_gu", B, 2 * I), ar.new("dec_m", B, I)
            if "wgu" in served:               # (what ops.gemm_gated_fwd composes: the Linear, then the interleaved activation)
                ops.gated_act_fwd_il(lin(li, "wgu", x2, gu), m, self.act)
            else:
                ops.gemm_gated_fwd(x2, Lw["wgu"], gu, m, self.act)
            h, branch = h1, lin(li, "wd", m, ar.new("dec_dn", B, H))
        logits = head_fwd(ar, h, branch, True, tok, self.norm, self.lm_head, eps)["logits"]      # (top form: one row per prompt already)
        return logits, ops.argmax_rows(logits)[0]

    @torch.no_grad()
    def generate(self, input_ids=None, max_new_tokens=1, lengths=None, eos_token_id=None, pad_token_id=None, graph=False, return_logits=False,
                 inputs_embeds=None, force_tokens=None, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, seed=None, repetition_penalty=1.0,
                 presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None):
        """Continuation of input_ids [B, S] on the resident weights, forward only, with a KV cache, greedy by default:
        -> dict(sequences int64 [B, S + T'], new_tokens int64 [B, T'], n_new int64 [B], logit / logprob fp32 [B, T'] = the step's logit and
        log-probability of new_tokens[b, t], lengths int64 [B] = the input lengths + T'[, logits fp32 [B, T', V] with return_logits]).
        The prefill is the forward explain() runs; every layer's rotated K and its V are copied into caches [L, B, cap, nk d] of the arena,
        cap = S + max_new_tokens <= max_seq.  The first new token is the arg-max (lrp_argmax_rows, the one explain() takes its default target
        from) of the prefill's logits; each further one costs one _decode_step.  lengths: prompts LEFT-padded to S as for explain(); the result
        equals the un-padded single-prompt run up to rounding.
        eos_token_id (int or list): a prompt that emits one is finished; it is fed pad_token_id (default: the first EOS id) from then on and its
        later new_tokens are pad_token_id (logit / logprob there are those of the pad id).  n_new[b] counts the tokens up to and including the
        EOS; the loop ends when every prompt has finished, T' = max_b n_new[b] <= max_new_tokens.  Stopping reads B flags back per token;
        without eos_token_id nothing is read back before the end.
        graph=True: the step is captured once per (B, cap) into a hipGraph and replayed, its token ids and its column copied into the graph's
        static inputs before each replay; bitwise the eager result.
        force_tokens int [B, max_new_tokens] (optional): teacher forcing -- token t of the continuation is force_tokens[b, t] in place of the
        arg-max (logit / logprob are then the model's values of the given answer: scoring it through the cache).
        weight_format="mxfp4" bf16 engines read the layers' codes in place at B <= 128 (ops.linear_stream_fwd_q; a matrix the kernel does not
        serve is dequantised once per token).
        do_sample=True: token t is drawn by lrp_sample_rows from step t's logits in place of the arg-max -- temperature
        > 0, top_k (0: off; ties at the k-th logit are kept), top_p in (0, 1] (1: off), min_p in [0, 1] (0: off), applied in HF's order; seed
        is required: an int (prompt b draws from Philox stream b of that seed) or a list of B ints (prompt b draws from its own seed: its
        continuation does not depend on the batch).  Same seed, same tokens, eager or graph.  logit / logprob stay the model's untempered values
        of the drawn tokens (what explain_generated explains); the dict gains sample_logprob [B, T'], the log-probability under the
        temperature and the filters.
        repetition_penalty / presence_penalty / frequency_penalty / logit_bias: lrp_logit_penalty turns step t's raw
        logits into processed ones, and token t is the arg-max (or, with do_sample, the draw) of those.  repetition_penalty > 0 (1: off) is HF's
        RepetitionPenaltyLogitsProcessor over the prompt (its left pads are no history) and the generated tokens: x < 0 ? x rp : x / rp;
        frequency_penalty and presence_penalty are the OpenAI / vLLM ones over the generated tokens only: x - fp count - pp; logit_bias is a
        {token: float} dict or an fp32 [vocab] tensor added last, -inf bans a token.  logit / logprob / logits stay the model's raw values of
        the chosen tokens (what explain_generated explains); sample_logprob is under the processed distribution.  At the neutral values
        nothing is launched or allocated.  No beam search, n-gram blocking, min_new_tokens or per-prompt settings.
        ValueError before any kernel runs: inputs_embeds, max_new_tokens < 1, S + max_new_tokens > max_seq, bad lengths, an eos_token_id,
        pad_token_id or forced token outside [0, vocab), and what sample_request refuses (a sampling argument without do_sample, do_sample
        without seed or with force_tokens, a setting outside its range) and what penalty_request refuses (a penalty outside its range, a bad
        logit_bias, any of them with force_tokens)."""
        return generate_cached(self, self._embed, self._prefill_kv, lambda B, cap: ("decode", B, cap, self.mode), input_ids, max_new_tokens,
                               lengths, eos_token_id, pad_token_id, graph, return_logits, inputs_embeds, force_tokens, do_sample, temperature,
                               top_k, top_p, min_p, seed, repetition_penalty, presence_penalty, frequency_penalty, logit_bias)

    @torch.no_grad()
    def explain_generated(self, input_ids=None, max_new_tokens=1, lengths=None, eos_token_id=None, pad_token_id=None, graph=False,
                          objective="logprob", position_weights=None, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0,
                          seed=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None,
                          **readout_kw):
        """Prompt in, the model's own answer and its attribution out, on one resident copy of the weights: generate() (greedy, or sampled with
        do_sample=True and generate()'s sampling keywords; repetition_penalty, presence_penalty, frequency_penalty and logit_bias as in
        generate()), then
        explain(sequences, lengths=out["lengths"], positions=[S - 1 .. S + T' - 2], position_weights=w, objective=objective, **readout_kw) --
        row S - 1 + t predicts new token t, so the default targets of positions ARE the generated tokens.  w[b, t] = 1 for t < n_new[b], else 0
        (the slots after an EOS are the zero-weight spare slots positions defines); position_weights="mean": 1 / n_new[b] instead; or an
        explicit fp32 [B, T'].  The last column is no explained row: R_tok is exactly 0 there, as at pads.  -> explain's dict plus sequences,
        new_tokens, n_new.  graph applies to the generation; per_position=True and every read-out keyword pass through to explain()."""
        return explain_answer(self, input_ids, max_new_tokens, lengths, eos_token_id, pad_token_id, graph, objective, position_weights,
                              do_sample, temperature, top_k, top_p, min_p, seed, readout_kw, repetition_penalty, presence_penalty,
                              frequency_penalty, logit_bias)
