"""Whole-model AttnLRP engine for the dense Qwen decoders (Qwen2 / Qwen2.5 and the distillations built on them; Qwen3), efficient placement
(ref wiring: lxt/efficient/models/qwen2.py, qwen3.py; examples/quantized_qwen2.py, quantized_qwen3.py).

Both families are a Llama layer plus one thing, and QwenLRP is LlamaLRP plus those two things -- the same scaffold, the same fused layer
(engine.fused_qkv_fwd / fused_layer_fwd / fused_layer_bwd), the same explain():
  * Qwen2: a bias on q / k / v.  bf16, M = B S rows: added in the fused QKV GEMM's epilogue ahead of the rotation (lrp_gemm_nt_rs_bias[_rope]);
    the backward does not change (the bias receives relevance and passes none on).  The norm-weight fold scales columns of W only.
  * Qwen3: a per-head RMSNorm on q and k in front of RoPE (ops.qk_norm_rope_fwd / ops.qkv_bwd_pack, the site kernels Gemma-3 uses, w_offset 0).
fp32 (the parity engine) runs the per-kernel path: the bias through ops.linear_fwd, the head norms through ops.head_rmsnorm_fwd / _bwd.
Tied embeddings (the small checkpoints): one stored copy serves the embedding and the LM head.
"""
import torch

from . import engine as E

_FAMILIES = ("qwen2", "qwen3")


def config_from_hf(hf_cfg):
    """HF Qwen2Config / Qwen3Config -> engine cfg.  What the driver does not implement is refused here, before any kernel runs."""
    mt = getattr(hf_cfg, "model_type", None)
    if mt not in _FAMILIES:
        raise NotImplementedError(f"QwenLRP drives dense Qwen2 / Qwen3 decoders only (model_type={mt!r}); Llama runs on lxt_amd.engine.LlamaLRP, "
                                  "Qwen3-MoE and other families through lxt_amd.efficient.monkey_patch")
    nL = hf_cfg.num_hidden_layers
    types = getattr(hf_cfg, "layer_types", None)
    if getattr(hf_cfg, "use_sliding_window", False) or (types is not None and any(t != "full_attention" for t in list(types)[:nL])):
        raise NotImplementedError("QwenLRP: sliding-window layers (use_sliding_window=True / layer_types other than 'full_attention') are not "
                                  "supported by the fused driver (use the monkey_patch drop-in path)")
    if getattr(hf_cfg, "mlp_bias", False):
        raise NotImplementedError("QwenLRP: mlp_bias=True is not supported by the fused driver (use the monkey_patch drop-in path)")
    if mt == "qwen3" and getattr(hf_cfg, "attention_bias", False):
        raise NotImplementedError("QwenLRP: Qwen3 with attention_bias=True puts a bias on the o projection, which the fused driver does not "
                                  "support (use the monkey_patch drop-in path)")
    kind = E.rope_kind(hf_cfg)
    if kind not in E._STATIC_ROPE:
        raise NotImplementedError(f"QwenLRP: rope_type {kind!r} (sequence-length dependent frequencies) is not supported")
    hd = getattr(hf_cfg, "head_dim", None) or hf_cfg.hidden_size // hf_cfg.num_attention_heads
    rp = getattr(hf_cfg, "rope_parameters", None)
    theta = rp.get("rope_theta") if isinstance(rp, dict) else None
    if theta is None:
        theta = getattr(hf_cfg, "rope_theta", 10000.0)
    cfg = dict(hidden=hf_cfg.hidden_size, inter=hf_cfg.intermediate_size, n_layers=nL, n_heads=hf_cfg.num_attention_heads,
               n_kv=hf_cfg.num_key_value_heads, head_dim=hd, vocab=hf_cfg.vocab_size, rope_theta=float(theta),
               rms_eps=float(hf_cfg.rms_norm_eps), act=getattr(hf_cfg, "hidden_act", "silu"), family=mt,
               qkv_bias=mt == "qwen2", qk_norm=mt == "qwen3", tied=bool(getattr(hf_cfg, "tie_word_embeddings", False)))
    if kind != "default":
        from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS
        inv_freq, att = ROPE_INIT_FUNCTIONS[kind](hf_cfg, "cpu")
        cfg["inv_freq"], cfg["attention_scaling"] = inv_freq.float().cpu(), float(att)
    return cfg


def weights_from_hf(model):
    """plain (cfg, W) view of a HF Qwen2ForCausalLM / Qwen3ForCausalLM (no copies).  A bias on o or in the MLP is refused."""
    cfg = config_from_hf(model.config)
    m = model.model
    W = dict(embed=m.embed_tokens.weight.detach(), norm=m.norm.weight.detach(), layers=[])
    if model.lm_head.weight.data_ptr() != m.embed_tokens.weight.data_ptr():
        W["lm_head"], cfg["tied"] = model.lm_head.weight.detach(), False
    else:
        cfg["tied"] = True
    for L in m.layers:
        a, mlp = L.self_attn, L.mlp
        if any(t.bias is not None for t in (a.o_proj, mlp.gate_proj, mlp.up_proj, mlp.down_proj)):
            raise NotImplementedError("QwenLRP: a bias on o_proj or in the MLP is not supported by the fused driver")
        Lw = dict(ln1=L.input_layernorm.weight.detach(), ln2=L.post_attention_layernorm.weight.detach(), wq=a.q_proj.weight.detach(),
                  wk=a.k_proj.weight.detach(), wv=a.v_proj.weight.detach(), wo=a.o_proj.weight.detach(), wg=mlp.gate_proj.weight.detach(),
                  wu=mlp.up_proj.weight.detach(), wd=mlp.down_proj.weight.detach())
        if cfg["qkv_bias"]:
            Lw.update(bq=a.q_proj.bias.detach(), bk=a.k_proj.bias.detach(), bv=a.v_proj.bias.detach())
        if cfg["qk_norm"]:
            Lw.update(qn=a.q_norm.weight.detach(), kn=a.k_norm.weight.detach())
        W["layers"].append(Lw)
    return cfg, W


class QwenLRP(E.LlamaLRP):
    """LlamaLRP for dense Qwen2 / Qwen3: cfg carries qkv_bias / qk_norm / tied (config_from_hf); W["layers"][i] additionally holds bq, bk, bv
    (Qwen2) or qn, kn (Qwen3), and W has no "lm_head" when the embeddings are tied.  explain() is LlamaLRP.explain."""

    def __init__(self, cfg, W, dtype=torch.bfloat16, device="cuda", mode="efficient", max_seq=4096, sparse_top=True, fold_norm=None,
                 weight_format=None, rule="attnlrp"):
        cfg = dict(cfg, tied=bool(cfg.get("tied", "lm_head" not in W)))
        super().__init__(cfg, W, dtype=dtype, device=device, mode=mode, max_seq=max_seq, sparse_top=sparse_top, fold_norm=fold_norm,
                         weight_format=weight_format, rule=rule)

    def set_mode(self, mode):
        if mode == "explicit":
            raise NotImplementedError("QwenLRP: mode='explicit' is not implemented -- the explicit eps-rule of a biased Linear divides by "
                                      "z = x W^T + b and is a different piece of work; the dense Qwen driver runs the efficient placement only")
        super().set_mode(mode)

    @classmethod
    def from_hf(cls, model, **kw):
        cfg, W = weights_from_hf(model)
        kw.setdefault("dtype", next(model.parameters()).dtype)
        return cls(cfg, W, **kw)
