"""Fused AttnLRP driver for Gemma-3 text decoders (BASELINE config 4): forward + relevance backward of `lxt.efficient` on
Gemma3ForCausalLM as straight sequences of liblrp_hip launches -- no autograd, no module hooks.

What differs from the Llama driver (engine.py), with the reference lines that fix the behaviour:
  * (1 + w) RMSNorm with the rstd detached (ref lxt/efficient/models/gemma3.py:11-12 `gemma3_norm`, HF Gemma3RMSNorm.forward):
    the norm kernels' `w_offset = 1`; the backward is the row-constant scale G (1 + w) rstd;
  * FOUR norms per layer (HF Gemma3DecoderLayer.forward): input -> attention -> post-attention norm -> residual add;
    pre-feed-forward norm -> gated MLP -> post-feed-forward norm -> residual add;
  * per-head q / k RMSNorm (head_dim-wide rows) in front of RoPE (HF Gemma3Attention.forward);
  * gelu-tanh gated MLP under the same identity + uniform rules (ref gemma3.py:15 -> patches.py:145-157 `gated_mlp_forward`);
  * sliding-window layers (5 local : 1 global in the released checkpoints) with their own rotary base, attention scale
    query_pre_attn_scalar ** -0.5, embeddings scaled by sqrt(hidden);
  * attention factors as everywhere in lxt.efficient (ref patches.py:193-203: q, k / 4, v / 2) -- inside the attention kernels.
The reference defines Gemma-3 for the efficient mode only (there is no lxt.explicit Gemma-3), and so does this driver.
Weights are held once (forward layout; dgrads run the NN GEMM on the stored weight), gate/up interleaved for the fused GEMM epilogues,
activations live in the same tagged arena as the Llama driver's.
"""
import torch

from . import ops
from .engine import (EFFICIENT, Arena, GraphCache, attn_map_request, explain_answer, explain_inputs, explain_pipeline, fused_layout,
                     generate_cached, head_fwd, head_request, head_seed_bwd, latent_request, pack_flat, pitch_pad, position_request, put_gate_up,
                     put_rows, rope_tables, top_attn_operands)

_STATIC_ROPE = ("default", "linear")


def config_from_hf(hf_cfg):
    """HF Gemma3TextConfig (or the text_config of a Gemma3Config) -> engine cfg; unsupported features are refused loudly"""
    hf_cfg = getattr(hf_cfg, "text_config", hf_cfg)
    mt = getattr(hf_cfg, "model_type", "")
    if mt not in ("gemma3_text", "gemma3"):
        raise NotImplementedError(f"Gemma3LRP drives Gemma-3 text decoders only (model_type={mt!r})")
    if getattr(hf_cfg, "attention_bias", False):
        raise NotImplementedError("Gemma3LRP: attention_bias = True is not supported by the fused driver (use monkey_patch)")
    if getattr(hf_cfg, "attn_logit_softcapping", None) or getattr(hf_cfg, "final_logit_softcapping", None):
        raise NotImplementedError("Gemma3LRP: logit soft-capping is not supported by the fused driver (use monkey_patch)")
    if not getattr(hf_cfg, "use_bidirectional_attention", False) is False:
        raise NotImplementedError("Gemma3LRP: bidirectional attention is not supported")
    act = getattr(hf_cfg, "hidden_activation", getattr(hf_cfg, "hidden_act", "gelu_pytorch_tanh"))
    if act not in ("gelu_pytorch_tanh", "gelu_tanh", "silu"):
        raise NotImplementedError(f"Gemma3LRP: activation {act!r}")
    rope = {}
    rp_all = getattr(hf_cfg, "rope_parameters", None)
    for lt in sorted(set(hf_cfg.layer_types)):
        if isinstance(rp_all, dict) and isinstance(rp_all.get(lt), dict):
            rp = rp_all[lt]                                   # transformers 5: one parameter set per layer type
        elif lt == "sliding_attention":                       # transformers 4.x schema: rope_local_base_freq for the local layers,
            rp = dict(rope_type="default", rope_theta=getattr(hf_cfg, "rope_local_base_freq", 10000.0))
        else:                                                 # rope_theta (+ rope_scaling, key 'rope_type' or legacy 'type') for the global ones
            rs = dict(getattr(hf_cfg, "rope_scaling", None) or {})
            rp = dict(rs, rope_type=rs.get("rope_type", rs.get("type", "default")), rope_theta=getattr(hf_cfg, "rope_theta", 1e6))
        kind = rp.get("rope_type", "default")
        if kind not in _STATIC_ROPE:
            raise NotImplementedError(f"Gemma3LRP: rope_type {kind!r} (layer type {lt!r}) is not supported by the fused driver")
        d = hf_cfg.head_dim
        inv = 1.0 / (float(rp["rope_theta"]) ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
        if kind == "linear":                                  # HF `_compute_linear_scaling_rope_parameters`: inv_freq / factor, no post-scale
            inv = inv / float(rp["factor"])
        rope[lt] = (inv.float().cpu(), 1.0)
    return dict(hidden=hf_cfg.hidden_size, inter=hf_cfg.intermediate_size, n_layers=hf_cfg.num_hidden_layers,
                n_heads=hf_cfg.num_attention_heads, n_kv=hf_cfg.num_key_value_heads, head_dim=hf_cfg.head_dim,
                vocab=hf_cfg.vocab_size, rms_eps=float(hf_cfg.rms_norm_eps), act="silu" if act == "silu" else "gelu_tanh",
                scale=float(hf_cfg.query_pre_attn_scalar) ** -0.5, layer_types=list(hf_cfg.layer_types),
                window=int(hf_cfg.sliding_window), rope=rope, embed_scale=float(hf_cfg.hidden_size) ** 0.5)


def weights_from_hf(model):
    """plain (cfg, W) view of a HF Gemma3ForCausalLM / the language model of a Gemma3ForConditionalGeneration"""
    lm = model.model if hasattr(model, "lm_head") else model
    m = getattr(lm, "language_model", lm)
    m = getattr(m, "model", m) if not hasattr(m, "layers") else m
    W = dict(embed=m.embed_tokens.weight.detach(), norm=m.norm.weight.detach(), lm_head=model.lm_head.weight.detach(), layers=[])
    for L in m.layers:
        a, mlp = L.self_attn, L.mlp
        W["layers"].append(dict(ln_in=L.input_layernorm.weight.detach(), ln_pa=L.post_attention_layernorm.weight.detach(),
                                ln_pf=L.pre_feedforward_layernorm.weight.detach(), ln_pff=L.post_feedforward_layernorm.weight.detach(),
                                qn=a.q_norm.weight.detach(), kn=a.k_norm.weight.detach(),
                                wq=a.q_proj.weight.detach(), wk=a.k_proj.weight.detach(), wv=a.v_proj.weight.detach(),
                                wo=a.o_proj.weight.detach(), wg=mlp.gate_proj.weight.detach(), wu=mlp.up_proj.weight.detach(),
                                wd=mlp.down_proj.weight.detach()))
    cfg = config_from_hf(model.config)
    return cfg, W


def gemma_attn_map_request(attn_map, nL, nq, d, dtype, mode="efficient"):
    """engine.attn_map_request for the Gemma-3 drivers: the same forms, checks and ValueErrors, and bf16 at d = 256 is served as well
    (lrp_attn_relmap_d256)"""
    return attn_map_request(attn_map, nL, nq, d, dtype, mode, bf16_dims=(64, 128, 256))


class Gemma3LRP:
    """explain(input_ids) -> dict(idx, logit, R_tok, logits): AttnLRP (lxt.efficient) token relevances of a Gemma-3 text decoder; on request
    the layer, latent, per-head and token-to-token read-outs of LlamaLRP.explain, answer-span attribution
    (positions=...), and generate() / explain_generated() on a KV cache"""

    def __init__(self, cfg, W, dtype=torch.bfloat16, device="cuda", max_seq=4096, sparse_top=True):
        if not torch.cuda.is_available():
            raise RuntimeError("Gemma3LRP needs a HIP device: the LRP kernels have no CPU fallback")
        self.cfg, self.dtype, self.device = dict(cfg), dtype, torch.device(device)
        # top-layer sparsity (as LlamaLRP): only the explained position's logit is used, so above the last layer's attention every row but one
        # per prompt is dead in the forward and carries zero gradient in the backward -- its o-projection, norms and MLP run on B rows instead
        # of B S, its attention on one query row per prompt (result-preserving: test_gemma3_engine_top_layer_sparsity_equals_dense)
        self.sparse_top = bool(sparse_top)
        self.eps, self.act = dict(EFFICIENT), cfg["act"]
        self.eps_g = self.eps["act"]
        dev = self.device
        tied = W["lm_head"].data_ptr() == W["embed"].data_ptr()
        self.flat, top, self.layers = pack_flat(*self.flat_layout(cfg, dtype, tied), len(W["layers"]), dtype, dev)   # ONE buffer: a multi-GPU
        self.embed = put_rows(top["embed"], W["embed"])                                                               # start-up is a single broadcast
        self.lm_head = self.embed if tied else put_rows(top["lm_head"], W["lm_head"])
        self.norm = put_rows(top["norm"], W["norm"])
        for Lw, L in zip(self.layers, W["layers"]):
            for k in ("ln_in", "ln_pa", "ln_pf", "ln_pff", "qn", "kn", "wo", "wd"):
                put_rows(Lw[k], L[k])
            put_rows(Lw["wqkv"], L["wq"], L["wk"], L["wv"])
            put_gate_up(Lw["wgu"], L["wg"], L["wu"])
        self.attn_t = ops.attn_needs_transposed(self.embed, cfg["head_dim"])
        self.rope = {lt: rope_tables(inv, att, max_seq, dtype, dev) for lt, (inv, att) in cfg["rope"].items()}     # per layer type
        self.embed_scale = torch.tensor(cfg["embed_scale"], dtype=dtype)   # HF: the scale itself is rounded to the model dtype
        self._embed_scale_dev = self.embed_scale.to(dev)                   # (the decode step is captured: no host-to-device copy inside it)
        self.max_seq = max_seq
        self._arena = Arena(dev, dtype)
        self._graphs = GraphCache(dev, lambda: self._arena.gen)          # generate(graph=True): the decode step, one graph per (B, cap)
        torch.cuda.synchronize(dev)

    @staticmethod
    def flat_layout(cfg, dtype, tied):
        """(shape, row pitch) of the weights in `flat` (pack_flat): the model-wide ones (a tied LM head is the embedding itself), then one layer's;
        gate/up and down at fused_layout's pitches (their dgrads stride over the stored rows), qkv unpadded"""
        H, I, nq, nk, d, V = cfg["hidden"], cfg["inter"], cfg["n_heads"], cfg["n_kv"], cfg["head_dim"], cfg["vocab"]
        pt, vec = fused_layout(H, I, nq, nk, d, dtype), ((H,), None)
        top = dict(embed=((V, H), None), lm_head=((V, H), None), norm=vec)
        if tied:
            del top["lm_head"]
        return top, dict(ln_in=vec, ln_pa=vec, ln_pf=vec, ln_pff=vec, qn=((d,), None), kn=((d,), None), wqkv=(((nq + 2 * nk) * d, H), None),
                         wo=((H, nq * d), None), wgu=((2 * I, H), pt["Wgu"]), wd=((H, I), pt["Wd"]))

    @classmethod
    def from_hf(cls, model, **kw):
        cfg, W = weights_from_hf(model)
        kw.setdefault("dtype", next(model.parameters()).dtype)
        return cls(cfg, W, **kw)

    def release(self):
        self._arena = Arena(self.device, self.dtype)
        self._graphs.clear()

    def _window(self, li):
        return self.cfg["window"] if self.cfg["layer_types"][li] == "sliding_attention" else 0

    def _attn_mask(self, li, row_iv):
        """-> (causal, window, row intervals) of layer li.  row_iv is None / a (lo, hi) pair (left-padded text batches: causal + window stay
        structural) or a dict {"global": (lo, hi), "local": (lo, hi)} of COMPLETE per-row key intervals (image + text prompts: tokens of one
        image attend to each other in both directions, HF `create_masks_for_vision_model`; the intervals then carry causality and the
        sliding window themselves, see engine_gemma3_mm.mm_row_intervals)"""
        if isinstance(row_iv, dict):
            return False, 0, row_iv["local" if self.cfg["layer_types"][li] == "sliding_attention" else "global"]
        return True, self._window(li), row_iv

    # ---------------------------------------------------------------------------------------------
    def forward(self, emb, B, S, row_iv=None, keep_h=False, keep_m=False, rows=None):
        """keep_h / keep_m: every layer's input h / down-projection input m gets a buffer of its own (the read-outs of the backward need
        them); otherwise h lives in a two-buffer ping-pong and m in one shared buffer, and neither survives its layer.  rows int64 [R]
        (explain(positions=...)): the explained rows of the [B S, .] activations in place of each prompt's last one; the top layer then
        runs dense like every other layer, whatever self.sparse_top says"""
        c = self.cfg
        H, I, d, nq, nk = c["hidden"], c["inter"], c["head_dim"], c["n_heads"], c["n_kv"]
        M, dt, dev = B * S, self.dtype, self.device
        nqd, nkd, nqkv = nq * d, nk * d, (nq + 2 * nk) * d
        ar = self._arena
        eps = c["rms_eps"]
        stash = []
        h_prev, branch, nxt = emb, None, None
        last = torch.arange(B, device=dev) * S + (S - 1) if rows is None else rows
        site = ops.sandwich_norm_ok(emb)      # Gemma-3's norms / q-k norm / RoPE fused per site (ops.SITE_FUSION; results bit-identical)
        h_tag = (lambda li: ("h_keep", li)) if keep_h else (lambda li: ("h", li & 1))
        m_buf = (lambda li: ar.get(("m_keep", li), (M, I), dt, pad=pitch_pad(I, dt.itemsize))) if keep_m else (lambda li: ar.wide("m", M, I))
        for li, Lw in enumerate(self.layers):
            st = {}
            cos, sin = self.rope[c["layer_types"][li]]
            # input norm (fused with the previous layer's residual add: h = h1_prev + post_ff_norm(dn_prev); with the site kernels the previous
            # layer's tail has produced h, x and rstd1 already)
            if nxt is not None:
                h, x, st["rstd1"] = nxt
            else:
                x, st["rstd1"] = ar.new("x", M, H), ar.f32(("rstd1", li), M)
                if branch is None:
                    h = h_prev
                    ops.add_rmsnorm_fwd(h_prev, None, Lw["ln_in"], eps, 1.0, y=x, rstd=st["rstd1"])
                else:
                    h = ar.new(h_tag(li), M, H)
                    ops.add_rmsnorm_fwd(h_prev, branch, Lw["ln_in"], eps, 1.0, hsum_out=h, y=x, rstd=st["rstd1"])
            st["h"] = h
            qkv = ops.linear_fwd(x, Lw["wqkv"], out=ar.new(("qkv", li), M, nqkv))
            # per-head q / k norm straight out of the fused projection output (strided rows), then RoPE with this layer type's table
            st["rstd_q"], st["rstd_k"] = ar.f32(("rstd_q", li), M * nq), ar.f32(("rstd_k", li), M * nk)
            if site:      # one pass: q / k norm + RoPE (bit-identical to the four launches below)
                qr, kr = ops.qk_norm_rope_fwd(qkv, Lw["qn"], Lw["kn"], ar.new(("qr", li), M, nqd), ar.new(("kr", li), M, nkd), st["rstd_q"],
                                              st["rstd_k"], cos, sin, S, nq, nk, d, eps, 1.0)
            else:
                qn, kn = ar.new("qn", M, nqd), ar.new("kn", M, nkd)
                ops.head_rmsnorm_fwd(qkv[:, :nqd], Lw["qn"], qn, st["rstd_q"], nq, d, eps, 1.0)
                ops.head_rmsnorm_fwd(qkv[:, nqd: nqd + nkd], Lw["kn"], kn, st["rstd_k"], nk, d, eps, 1.0)
                qr = ops.rope_fwd(qn, ar.new(("qr", li), M, nqd), cos, sin, S, nq, d)
                kr = ops.rope_fwd(kn, ar.new(("kr", li), M, nkd), cos, sin, S, nk, d)
            v = qkv[:, nqd + nkd:]
            v_t = ops.transpose_heads(v, B, S, nk, d) if self.attn_t else None
            o, lse = ar.new(("o", li), M, nqd), ar.f32(("lse", li), B, nq, S)
            causal, win, iv = self._attn_mask(li, row_iv)
            if self.sparse_top and rows is None and li == len(self.layers) - 1:
                # ---- the top layer above its attention: one row per prompt
                ops.attn_fwd(qr, kr, v, v_t, o, lse, B, S, nq, nk, d, c["scale"], causal, win, q_begin=S - 1, row_iv=iv)
                o_l, h_l = o.index_select(0, last), h.index_select(0, last)
                a_l = ops.linear_fwd(o_l, Lw["wo"], out=ar.new("a_l", B, H))
                pa_l, rstd_pa_l = ops.add_rmsnorm_fwd(a_l, None, Lw["ln_pa"], eps, 1.0)
                h1_l = ar.new("h1_l", B, H)
                x2_l, rstd2_l = ops.add_rmsnorm_fwd(h_l, pa_l, Lw["ln_pf"], eps, 1.0, hsum_out=h1_l)
                gu_l, m_l = ops.gemm_gated_fwd(x2_l, Lw["wgu"], ar.new("gu_l", B, 2 * I), ar.new("m_l", B, I), self.act)
                dn_l = ops.linear_fwd(m_l, Lw["wd"], out=ar.new("dn_l", B, H))
                pff_l, rstd_pff_l = ops.add_rmsnorm_fwd(dn_l, None, Lw["ln_pff"], eps, 1.0)
                st.update(top=True, qkv=qkv, qr=qr, kr=kr, lse=lse, o_l=o_l, gu_l=gu_l, m_l=m_l, rstd_pa_l=rstd_pa_l, rstd2_l=rstd2_l,
                          rstd_pff_l=rstd_pff_l)
                stash.append(st)
                h_prev, branch = h1_l, pff_l
                break
            ops.attn_fwd(qr, kr, v, v_t, o, lse, B, S, nq, nk, d, c["scale"], causal, win, row_iv=iv)
            a = ops.linear_fwd(o, Lw["wo"], out=ar.new("a", M, H))
            # post-attention norm, residual add, pre-feed-forward norm
            st["rstd_pa"] = ar.f32(("rstd_pa", li), M)
            h1, x2, st["rstd2"] = ar.new(("h1", li & 1), M, H), ar.new("x2", M, H), ar.f32(("rstd2", li), M)
            if site:      # one pass (the normed branch never goes to memory)
                ops.sandwich_norm_fwd(a, h, Lw["ln_pa"], Lw["ln_pf"], eps, 1.0, h1, x2, st["rstd_pa"], st["rstd2"])
            else:
                pa = ar.new("pa", M, H)
                ops.add_rmsnorm_fwd(a, None, Lw["ln_pa"], eps, 1.0, y=pa, rstd=st["rstd_pa"])
                ops.add_rmsnorm_fwd(h, pa, Lw["ln_pf"], eps, 1.0, hsum_out=h1, y=x2, rstd=st["rstd2"])
            coef = ops.gated_coef_ok(M, I, H, H, Lw["wgu"].stride(0), H, Lw["wd"].stride(0), self.act, dt)
            if coef:      # gated rules inside the two GEMMs: the backward's coefficients are stashed in gu's place (ops.gemm_gated_fwd_coef)
                gu, m = ops.gemm_gated_fwd_coef(x2, Lw["wgu"], ar.new(("gu", li), M, 2 * I), m_buf(li), self.eps_g, self.eps["lin"], self.act)
            else:
                gu, m = ops.gemm_gated_fwd(x2, Lw["wgu"], ar.new(("gu", li), M, 2 * I), m_buf(li), self.act)
            dn = ops.linear_fwd(m, Lw["wd"], out=ar.new("dn", M, H))
            st["rstd_pff"] = ar.f32(("rstd_pff", li), M)
            st.update(qkv=qkv, qr=qr, kr=kr, o=o, lse=lse, gu=gu, coef=coef, m=m)
            stash.append(st)
            if site and li + 1 < len(self.layers):
                # post-feed-forward norm, residual add and the NEXT layer's input norm in one pass
                nxt = (ar.new(h_tag(li + 1), M, H), ar.new("x", M, H), ar.f32(("rstd1", li + 1), M))
                ops.sandwich_norm_fwd(dn, h1, Lw["ln_pff"], self.layers[li + 1]["ln_in"], eps, 1.0, nxt[0], nxt[1], st["rstd_pff"], nxt[2])
                continue
            nxt = None
            pff = ar.new("pff", M, H)
            ops.add_rmsnorm_fwd(dn, None, Lw["ln_pff"], eps, 1.0, y=pff, rstd=st["rstd_pff"])
            h_prev, branch = h1, pff
        top = bool(stash) and stash[-1].get("top", False)         # (the sparse top layer left one row per prompt already)
        return dict(stash=stash, last=last, row_iv=row_iv, site=site, **head_fwd(ar, h_prev, branch, top, last, self.norm, self.lm_head, eps, 1.0))

    # ---------------------------------------------------------------------------------------------
    def _map_mask(self, cache, li, row_iv, B, S):
        """-> (causal, row intervals) of layer li's token-to-token map.  lrp_attn_relmap has no window argument: a sliding layer of a text
        prompt gets per-row intervals with the window folded in, lo = max(first, i - w + 1), built on the device once per call and window
        size (cache); image + text prompts hand over complete intervals per layer type and the call is not causal (_attn_mask)"""
        causal, win, iv = self._attn_mask(li, row_iv)
        if not win:
            return causal, iv
        if win not in cache:
            i = torch.arange(S, device=self.device, dtype=torch.int32)
            lo = (i - (win - 1)).clamp_min(0)[None].expand(B, S)
            if iv is None:
                cache[win] = (lo.contiguous(), (i + 1)[None].expand(B, S).contiguous())
            else:
                cache[win] = (torch.maximum(iv[0], lo).contiguous(), iv[1])
        return causal, cache[win]

    def backward(self, fw, idx, B, S, layer_relevance=False, latent=frozenset(), heads=None, attn_map=None):
        """-> (G at the embedding, layer_R rows or None, dict of the token-summed latent read-outs), as LlamaLRP.backward.  layer_relevance /
        "resid" need forward(keep_h=True), "mlp" forward(keep_m=True); heads: a HeadSink, attn_map: an AttnMapSink (None: nothing is launched)"""
        c, E = self.cfg, self.eps
        H, I, d, nq, nk = c["hidden"], c["inter"], c["head_dim"], c["n_heads"], c["n_kv"]
        M, rep = B * S, nq // nk
        nqd, nkd, nqkv = nq * d, nk * d, (nq + 2 * nk) * d
        ar = self._arena
        nL, dev = len(self.layers), self.device
        lat, layer_R, iv_cache = {}, None, {}
        # LM head (gradient of the explained logit) + final (1 + w) norm on the explained rows (one per prompt, or a span's R = B T: shared with
        # LlamaLRP, engine.head_seed_bwd), scattered into [M, H]
        R = fw["last"].shape[0]
        Gh_last = head_seed_bwd(ar, fw, idx, self.norm, self.lm_head, E["lin"], 1.0)
        top = bool(fw["stash"]) and fw["stash"][-1].get("top", False)
        Gs = None if top else ar.zeros(("Gs", len(self.layers) & 1), M, H).index_copy_(0, fw["last"], Gh_last)       # gradient w.r.t. h_L = h1 + pff
        if layer_relevance:          # index L: the head's explained rows (S = 1)
            layer_R = [ops.readout(fw["hL_last"], Gh_last, out=ar.f32("rel_last", R))]
        if "resid" in latent:
            lat["R_resid"] = torch.empty(nL + 1, B, H, device=dev, dtype=torch.float32)
            ops.colsum_dot(fw["hL_last"], Gh_last, B, R // B, out=lat["R_resid"][nL])          # (a prompt's explained rows, in slot order)
        if "mlp" in latent:
            lat["R_mlp"] = torch.empty(nL, B, I, device=dev, dtype=torch.float32)
        site, Gdn = fw["site"], None
        for li in range(len(self.layers) - 1, -1, -1):
            Lw, st = self.layers[li], fw["stash"][li]
            hs = None if heads is None else heads.layer(li)
            am = None if attn_map is None else attn_map.layer(li)
            cos, sin = self.rope[c["layer_types"][li]]
            causal, win, iv = self._attn_mask(li, fw["row_iv"])
            q_begin = 0
            if st.get("top", False):
                # ---- one row per prompt through the post-feed-forward norm, the MLP, the two norms around the residual add and the o-projection; then
                # scatter into the dense operands of the attention backward (zero fill + row scatter; D's live column S - 1 is a strided scatter)
                Gdn_l, Gs1_l, Ga_l = ar.new("Gdn_l", B, H), ar.new("Gs1_l", B, H), ar.new("Ga_l", B, H)
                ops.rmsnorm_bwd_add2(None, Gh_last, Lw["ln_pff"], st["rstd_pff_l"], None, None, Gdn_l, None, None, 1.0, 0.0, 0.0)
                Agu_l = ops.gemm_gated_bwd(Gdn_l, Lw["wd"], st["gu_l"], ar.new("Agu_l", B, 2 * I), self.eps_g, E["lin"], self.act)
                Gx2_l = ops.linear_dgrad(Agu_l, Lw["wgu"], out=ar.new("Gx2_l", B, H))
                ops.rmsnorm_bwd_add2(Gh_last, Gx2_l, Lw["ln_pf"], st["rstd2_l"], None, None, Gs1_l, None, None, 1.0, 0.0, 0.0)
                ops.rmsnorm_bwd_add2(None, Gs1_l, Lw["ln_pa"], st["rstd_pa_l"], None, None, Ga_l, None, None, 1.0, 0.0, 0.0)
                Gof_l = ops.linear_dgrad(Ga_l, Lw["wo"], out=ar.new("Gof_l", B, nqd))
                Gho, D, Gs1 = top_attn_operands(ar, Gof_l, st["o_l"], Gs1_l, fw["last"], S, nq, d, E["pv"])
                if "mlp" in latent:      # G_m = Gdn Wd, one dgrad the backward otherwise folds into Agu; one row per prompt, the others' neurons are 0
                    ops.colsum_dot(st["m_l"], ops.linear_dgrad(Gdn_l, Lw["wd"], out=ar.new("Gm_l", B, I)), B, 1, out=lat["R_mlp"][li])
                if hs is not None:
                    hs.last("out", st["o_l"], Gof_l)
                q_begin = S - 1
            else:
                # ---- post-feed-forward norm, gated MLP, pre-feed-forward norm + residual
                if Gdn is None:      # (with the site kernels the layer above has produced Gdn together with Gs)
                    Gdn = ar.new("Gdn", M, H)
                    ops.rmsnorm_bwd_add2(None, Gs, Lw["ln_pff"], st["rstd_pff"], None, None, Gdn, None, None, 1.0, 0.0, 0.0)
                if "mlp" in latent:
                    ops.colsum_dot(st["m"], ops.linear_dgrad(Gdn, Lw["wd"], out=ar.new("Gm", M, I)), B, S, out=lat["R_mlp"][li])
                if st["coef"]:
                    Agu = ops.gemm_gated_bwd_coef(Gdn, Lw["wd"], st["gu"], ar.wide("Agu", M, 2 * I))
                else:
                    Agu = ops.gemm_gated_bwd(Gdn, Lw["wd"], st["gu"], ar.wide("Agu", M, 2 * I), self.eps_g, E["lin"], self.act)
                Gx2 = ops.linear_dgrad(Agu, Lw["wgu"], out=ar.new("Gx2", M, H))
                Gs1, Ga = ar.new("Gs1", M, H), ar.new("Ga", M, H)
                if site:      # pre-feed-forward norm + residual (gradient w.r.t. h1) and the post-attention norm in one pass
                    ops.sandwich_norm_bwd(Gs, Gx2, Lw["ln_pf"], st["rstd2"], Lw["ln_pa"], st["rstd_pa"], Gs1, Ga, 1.0)
                else:
                    ops.rmsnorm_bwd_add2(Gs, Gx2, Lw["ln_pf"], st["rstd2"], None, None, Gs1, None, None, 1.0, 0.0, 0.0)     # w.r.t. h1
                    # ---- post-attention norm, o-proj, attention
                    ops.rmsnorm_bwd_add2(None, Gs1, Lw["ln_pa"], st["rstd_pa"], None, None, Ga, None, None, 1.0, 0.0, 0.0)
                Gof = ops.linear_dgrad(Ga, Lw["wo"], out=ar.new("Gof", M, nqd))
                Gho, D = ar.new("Gho", M, nqd), ar.f32("D", B, nq, S)
                ops.attn_bwd_prep(Gof, st["o"], Gho, D, B, S, nq, d, E["pv"], 0.5)
                if hs is not None:
                    hs("out", st["o"], Gof)
            q, k, v = st["qr"], st["kr"], st["qkv"][:, nqd + nkd:]
            if am is not None:          # (Gho = 1/2 G_o: attn_bwd_prep's factor)
                m_causal, m_iv = self._map_mask(iv_cache, li, fw["row_iv"], B, S)
                if q_begin == 0:
                    am(q, k, v, Gho, st["lse"], 2.0, m_iv, m_causal)
                else:
                    am.top(ar, q, k, v, Gho, st["lse"], 2.0, fw["last"], m_iv, m_causal)
            k_t = q_t = Gho_t = None
            if self.attn_t:
                k_t = ops.transpose_heads(k, B, S, nk, d)
                q_t = ops.transpose_heads(q, B, S, nq, d)
                Gho_t = ops.transpose_heads(Gho, B, S, nq, d)
            dq = ar.new("dq", M, nqd) if q_begin == 0 else ar.zeros("dq", M, nqd)          # (queries below q_begin carry no relevance: rows stay zero)
            dk_h, dv_h = ar.new("dk_h", M, nqd), ar.new("dv_h", M, nqd)
            ops.attn_bwd_dq(q, k, v, k_t, Gho, st["lse"], D, dq, B, S, nq, nk, d, c["scale"], E["mask"], E["qk"], causal, win, q_begin=q_begin,
                            row_iv=iv)
            ops.attn_bwd_dkv(q, k, v, q_t, Gho, Gho_t, st["lse"], D, dk_h, dv_h, B, S, nq, nk, d, c["scale"], E["mask"], E["qk"], causal, win,
                             q_begin=q_begin, row_iv=iv)
            if hs is not None:          # after the q / k norm and RoPE, k and v per QUERY head (before the group sums): no rotary table needed
                if q_begin == 0:
                    hs("q", q, dq)
                else:          # (the sparse top layer: dq's only live rows)
                    hs.last("q", q.index_select(0, fw["last"]), dq.index_select(0, fw["last"]))
                hs("k", k, dk_h, rep)
                hs("v", v, dv_h, rep)
            Aqkv = ar.new("Aqkv", M, nqkv)
            if site:      # the group sums, RoPE's backward and the q / k norms' scale in one pass over dq / dk_h / dv_h
                ops.qkv_bwd_pack(dq, dk_h, dv_h, Lw["qn"], Lw["kn"], st["rstd_q"], st["rstd_k"], cos, sin, Aqkv, S, nq, nk, d, 1.0)
            else:
                dk = ops.gqa_reduce(dk_h, ar.new("dk", M, nkd), M, nk, rep, d)
                ops.gqa_reduce(dv_h, Aqkv[:, nqd + nkd:], M, nk, rep, d)
                # RoPE backward (a rotation: plain gradient), then the q / k norms' row-constant scale, written into the fused [q | k | v] operand
                Gqn = ops.rope_bwd(dq, None, None, ar.new("Gqn", M, nqd), cos, sin, S, nq, d, 0.0, 0.0)
                Gkn = ops.rope_bwd(dk, None, None, ar.new("Gkn", M, nkd), cos, sin, S, nk, d, 0.0, 0.0)
                ops.head_rmsnorm_bwd(Gqn, Lw["qn"], st["rstd_q"], Aqkv[:, :nqd], nq, d, 1.0)
                ops.head_rmsnorm_bwd(Gkn, Lw["kn"], st["rstd_k"], Aqkv[:, nqd: nqd + nkd], nk, d, 1.0)
            Gx = ops.linear_dgrad(Aqkv, Lw["wqkv"], out=ar.new("Gx", M, H))
            # ---- input norm + residual (and, with the site kernels, the post-feed-forward norm of the layer below)
            Gs = ar.new(("Gs", li & 1), M, H)
            if site and li > 0:
                below = fw["stash"][li - 1]
                Gdn = ar.new("Gdn", M, H)
                ops.sandwich_norm_bwd(Gs1, Gx, Lw["ln_in"], st["rstd1"], self.layers[li - 1]["ln_pff"], below["rstd_pff"], Gs, Gdn, 1.0)
            else:
                Gdn = None
                ops.rmsnorm_bwd_add2(Gs1, Gx, Lw["ln_in"], st["rstd1"], None, None, Gs, None, None, 1.0, 0.0, 0.0)
            # ---- the boundary read-outs: one pass over the stored gradient and the layer's kept input
            if layer_relevance:
                layer_R.append(ops.readout(st["h"], Gs, out=ar.f32(("rel", li), M)))
            if "resid" in latent:
                ops.colsum_dot(st["h"], Gs, B, S, out=lat["R_resid"][li])
        return Gs, layer_R, lat

    # ---------------------------------------------------------------------------------------------
    @torch.no_grad()
    def readout_requests(self, latent, heads, attn_map):
        """-> (latent, heads, attn_map) requests, checked: every ValueError is raised before a kernel of the model runs"""
        c = self.cfg
        am = gemma_attn_map_request(attn_map, len(getattr(self, "layers", ())), c.get("n_heads", 0), c.get("head_dim"), self.dtype)
        return latent_request(latent, c["hidden"], c["inter"], self.dtype), head_request(heads, c.get("head_dim"), self.dtype), am

    def explain_emb(self, emb, B, S, row_iv, idx, return_G=False, layer_relevance=False, lat=frozenset(), hd=frozenset(), am=(False, ()),
                    span=None):
        """forward + backward + read-outs on prepared embeddings and CHECKED requests (readout_requests) -> (explain()'s dict, G at the embedding);
        with no request the buffers, the launches and every output are those of the plain call.  span: a SpanRequest
        (engine.position_request, explain(positions=...)); None: nothing of it is touched"""
        keep_h = layer_relevance or "trace" in lat or "resid" in lat
        return explain_pipeline(self, lambda **rows: self.forward(emb, B, S, row_iv, keep_h=keep_h, keep_m="mlp" in lat, **rows),
                                lambda fw, i, *readouts: self.backward(fw, i, B, S, *readouts), emb, B, S, idx, self.cfg["scale"],
                                return_G=return_G, layer_relevance=layer_relevance, latent=lat, heads=hd, attn_map=am, span=span)

    @torch.no_grad()
    def explain(self, input_ids=None, inputs_embeds=None, target=None, return_G=False, lengths=None, layer_relevance=False, latent=None,
                heads=None, attn_map=None, positions=None, position_weights=None, objective="logit", per_position=False):
        """input_ids [B, S] (or inputs_embeds [B, S, H] = HF's scaled embeddings); target: None (arg-max of the last position) or [B]
        vocabulary indices.  Returns dict(idx [B], logit [B], R_tok [B, S] fp32 = sum_h e (*) dlogit/de, logits [B, V]).
        lengths [B] (optional): prompts of different lengths in one call, LEFT-padded to S (as LlamaLRP.explain: pad keys are masked through
        the attention kernels' per-row key intervals, RoPE is relative, R_tok is exactly 0 at pad positions).
        layer_relevance, latent, heads, attn_map (optional): the read-outs of LlamaLRP.explain under the same names, shapes and meaning --
        layer_R [L+1, B];  latent from {"trace", "resid", "mlp"}: R_trace [L+1, B, S], R_resid [L+1, B, H], R_mlp [L, B, I];  heads from
        {"out", "q", "k", "v"}: R_head_out / _q / _k / _v [L, B, n_heads, S] and R_head [L, B, n_heads] (q / k after the head norms and RoPE,
        k / v per QUERY head at the source position);  attn_map "sum" and / or (layer, head) pairs: R_attn [L, B, S, S], R_attn_heads
        [n, B, S, S] and attn_map_heads (bf16 at head dim 256 runs lrp_attn_relmap_d256).  Entries outside a sliding layer's window, above
        the diagonal and at pad positions are exactly 0.  Requests are checked before a kernel of the model runs; R_tok, logit, idx and logits
        do not change with them, and a call without them allocates and launches what it always did.
        positions int [B, T] (optional), with position_weights, objective and per_position: answer-span attribution with the semantics, shapes
        and refusals of LlamaLRP.explain (DESIGN.md sections 20 and 23) -- T explained rows per prompt in one forward and one backward, target
        then [B, T] (default: the next token, the arg-max at column S - 1); returns idx, logit, logprob [B, T] and R_tok [B, S] (no logits),
        exactly 0 at pads and above the highest explained column; per_position=True adds R_tok_each [B, T, S] from T backwards.  Every
        read-out keyword keeps working.  Such a call runs the top layer dense; self.sparse_top stays as it is."""
        lat, hd, am = self.readout_requests(latent, heads, attn_map)
        nb, ns = (input_ids.shape if inputs_embeds is None else inputs_embeds.shape[:2]) if positions is not None else (0, 0)
        span = position_request(positions, position_weights, objective, per_position, nb, ns, self.cfg["vocab"], getattr(self, "device", None),
                                input_ids if inputs_embeds is None else None, target, lengths,
                                readouts=bool(layer_relevance or return_G or latent or heads or attn_map))
        if span is not None:
            target = None          # (checked and converted above; explain_inputs sees the plain form)
        B, S, emb, row_iv, idx = explain_inputs(input_ids, inputs_embeds, lengths, target, self.cfg["vocab"], self.max_seq, self.dtype,
                                                self.device)
        if emb is None:
            emb = self._embed(input_ids.to(self.device).reshape(-1))
        return self.explain_emb(emb, B, S, row_iv, idx, return_G, layer_relevance, lat, hd, am, span)[0]

    # --------------------------------------------------------------------------------------------- generation
    def _embed(self, ids):
        """the embedding rows [n, H] of token ids [n] on the device, times embed_scale (HF's scaled embeddings)"""
        return self.embed.index_select(0, ids) * self.embed_scale.to(self.device)

    def _prefill_kv(self, st):
        """(normed, rotated K rows, V rows) [B S, nk d] of one layer's forward stash: what generate() copies into the caches"""
        return st["kr"], st["qkv"][:, (self.cfg["n_heads"] + self.cfg["n_kv"]) * self.cfg["head_dim"]:]

    def _decode_step(self, tok, pos, lo, kc, vc, ws):
        """one new token per prompt through every layer on B rows (LlamaLRP._decode_step for Gemma-3): embedding rows times embed_scale, then
        per layer the input norm, the QKV Linear, lrp_decode_qknorm_rope_append (both head norms, RoPE with the layer type's table and the
        cache append in one launch), lrp_attn_decode, the o projection, the post-attention / pre-feed-forward norm pair, the gated MLP, the
        down projection, and the post-feed-forward norm with the next layer's input norm.  A sliding layer's first live key is
        max(lo[b], p - window + 1), formed on the device once per step.  tok int64 [B] and pos int32 [1] are device INPUTS of the step,
        nothing is incremented inside it.  kc, vc [L, B, cap, nk d];  lo int32 [B].  -> (logits [B, V] fp32, idx int32 [B]); launches only,
        capturable"""
        c = self.cfg
        H, I, d, nq, nk, eps = c["hidden"], c["inter"], c["head_dim"], c["n_heads"], c["n_kv"], c["rms_eps"]
        B, ar, nqk, nL = tok.shape[0], self._arena, (nq + nk) * d, len(self.layers)
        h = torch.mul(self.embed.index_select(0, tok), self._embed_scale_dev, out=ar.new("dec_emb", B, H))
        lo_win = None
        if "sliding_attention" in c["layer_types"]:
            first = torch.sub(pos, c["window"] - 1, out=ar.get("dec_first", (1,), torch.int32))
            lo_win = torch.maximum(lo, first, out=ar.get("dec_lo_win", (B,), torch.int32))
        site = ops.sandwich_norm_ok(h)
        x, r1, r2 = ar.new("dec_x", B, H), ar.f32("dec_rstd_a", B), ar.f32("dec_rstd_b", B)
        ops.add_rmsnorm_fwd(h, None, self.layers[0]["ln_in"], eps, 1.0, y=x, rstd=r1)
        for li, Lw in enumerate(self.layers):
            cos, sin = self.rope[c["layer_types"][li]]
            qkv = ops.linear_fwd(x, Lw["wqkv"], out=ar.new("dec_qkv", B, nqk + nk * d))
            q = ops.decode_qknorm_rope_append(qkv[:, :nqk], qkv[:, nqk:], Lw["qn"], Lw["kn"], eps, cos, sin, pos, ar.new("dec_q", B, nq * d),
                                              kc[li], vc[li], nq, nk, d, 1.0)
            o = ops.attn_decode(q, kc[li], vc[li], lo_win if self._window(li) else lo, pos, nq, nk, d, c["scale"],
                                out=ar.new("dec_o", B, nq * d), ws=ws)
            a = ops.linear_fwd(o, Lw["wo"], out=ar.new("dec_a", B, H))
            h1, x2 = ar.new("dec_h1", B, H), ar.new("dec_x2", B, H)
            if site:
                ops.sandwich_norm_fwd(a, h, Lw["ln_pa"], Lw["ln_pf"], eps, 1.0, h1, x2, r1, r2)
            else:
                pa = ar.new("dec_pa", B, H)
                ops.add_rmsnorm_fwd(a, None, Lw["ln_pa"], eps, 1.0, y=pa, rstd=r1)
                ops.add_rmsnorm_fwd(h, pa, Lw["ln_pf"], eps, 1.0, hsum_out=h1, y=x2, rstd=r2)
            gu, m = ops.gemm_gated_fwd(x2, Lw["wgu"], ar.new("dec_gu", B, 2 * I), ar.new("dec_m", B, I), self.act)
            dn = ops.linear_fwd(m, Lw["wd"], out=ar.new("dec_dn", B, H))
            if li + 1 == nL:
                pff = ar.new("dec_pff", B, H)
                ops.add_rmsnorm_fwd(dn, None, Lw["ln_pff"], eps, 1.0, y=pff, rstd=r1)
                break
            h = ar.new(("dec_h", li & 1), B, H)          # (the next layer's input: not h1, which this very step reads)
            if site:
                ops.sandwich_norm_fwd(dn, h1, Lw["ln_pff"], self.layers[li + 1]["ln_in"], eps, 1.0, h, x, r1, r2)
            else:
                pff = ar.new("dec_pff", B, H)
                ops.add_rmsnorm_fwd(dn, None, Lw["ln_pff"], eps, 1.0, y=pff, rstd=r1)
                ops.add_rmsnorm_fwd(h1, pff, self.layers[li + 1]["ln_in"], eps, 1.0, hsum_out=h, y=x, rstd=r2)
        logits = head_fwd(ar, h1, pff, True, tok, self.norm, self.lm_head, eps, 1.0)["logits"]      # (top form: one row per prompt already)
        return logits, ops.argmax_rows(logits)[0]

    @torch.no_grad()
    def generate(self, input_ids=None, max_new_tokens=1, lengths=None, eos_token_id=None, pad_token_id=None, graph=False, return_logits=False,
                 inputs_embeds=None, force_tokens=None, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, seed=None, repetition_penalty=1.0,
                 presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None):
        """Continuation of input_ids [B, S] on the resident weights, forward only, with a KV cache, greedy by default: LlamaLRP.generate's signature,
        returned dict (sequences, new_tokens, n_new, logit, logprob, lengths[, logits]) and EOS / pad / force_tokens / lengths behaviour
        (DESIGN.md sections 21 and 23).  The prefill is the forward explain() runs; every layer's normed, rotated K and its V are copied into
        caches [L, B, cap, nk d] of the arena, cap = S + max_new_tokens <= max_seq (sliding layers keep all cap rows: no ring buffer); the
        first new token is the lrp_argmax_rows of the prefill's logits, each further one costs one _decode_step.  graph=True: the step is
        captured once per (B, cap) and replayed, bitwise the eager result.  do_sample=True with temperature / top_k / top_p / min_p / seed: the
        seeded sampling of LlamaLRP.generate (the dict gains sample_logprob).  repetition_penalty / presence_penalty / frequency_penalty /
        logit_bias: the penalties of LlamaLRP.generate, applied by lrp_logit_penalty before the arg-max or the draw.
        ValueError before any kernel runs:
        inputs_embeds, max_new_tokens < 1, S + max_new_tokens > max_seq, bad lengths, an eos_token_id, pad_token_id or forced token outside
        [0, vocab), and what sample_request and penalty_request refuse."""
        return generate_cached(self, self._embed, self._prefill_kv, lambda B, cap: ("decode", B, cap), input_ids, max_new_tokens, lengths,
                               eos_token_id, pad_token_id, graph, return_logits, inputs_embeds, force_tokens, do_sample, temperature, top_k, top_p,
                               min_p, seed, repetition_penalty, presence_penalty, frequency_penalty, logit_bias)

    @torch.no_grad()
    def explain_generated(self, input_ids=None, max_new_tokens=1, lengths=None, eos_token_id=None, pad_token_id=None, graph=False,
                          objective="logprob", position_weights=None, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0,
                          seed=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None,
                          **readout_kw):
        """generate() (greedy, or sampled with do_sample=True and generate()'s sampling keywords; generate()'s penalties apply), then explain(sequences, lengths=out["lengths"], positions=[S - 1 .. S + T' - 2], position_weights=w,
        objective=objective, **readout_kw) with the weight rules of LlamaLRP.explain_generated (1 for t < n_new[b] else 0; "mean";
        or explicit) -> explain's dict plus sequences, new_tokens, n_new.  The last column is no explained row: R_tok is exactly 0 there"""
        return explain_answer(self, input_ids, max_new_tokens, lengths, eos_token_id, pad_token_id, graph, objective, position_weights,
                              do_sample, temperature, top_k, top_p, min_p, seed, readout_kw, repetition_penalty, presence_penalty,
                              frequency_penalty, logit_bias)
