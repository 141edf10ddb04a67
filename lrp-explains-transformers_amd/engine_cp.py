"""CP-LRP on the fused Llama / Qwen drivers (ref: the `cp_LRP` composites of lxt/efficient/models/llama.py, qwen2.py, qwen3.py;
lxt/efficient/patches.py:228-280).  Against the efficient AttnLRP placement:
  attention : query and key are detached and value takes the whole gradient, factor 1 -- no dQ, no dK, no RoPE / head-norm backward, no D;
  gated MLP : gate_proj(x) is detached, the activation is plain, no divide_gradient -- G_u = act(g) (*) G_m, G_g = 0;
  unchanged : RMSNorm (identity rule), the residual adds, the Linears (plain gradient), the head and the read-out.
The forward is the model's forward with the pre-activations gu stored (no coefficient stash); this module is the backward of one layer
(DESIGN.md section 25)."""
from . import ops

RULES = ("attnlrp", "cp")


def cp_request(rule, mode="efficient", heads=None, attn_map=None, weights=None, dtype=None, head_dim=None):
    """the `rule` keyword of LlamaLRP / QwenLRP and what rule="cp" does not serve, refused before a device is looked at and before any kernel
    runs: the explicit placement (CP-LRP is defined on the efficient one); the three read-outs that are formed inside the AttnLRP attention /
    Linear backward -- per-head relevance (heads=), attention maps (attn_map=), per-weight relevance (weights=); and a (dtype, head dim) that
    lrp_attn_bwd_dv has no kernel for"""
    if rule not in RULES:
        raise ValueError(f"rule must be one of {RULES}, got {rule!r}")
    if rule != "cp":
        return rule
    if mode != "efficient":
        raise ValueError('rule="cp" is defined on the efficient placement: mode="explicit" is not served')
    for name, v in (("heads", heads), ("attn_map", attn_map), ("weights", weights)):
        if v is not None and not (isinstance(v, (tuple, list, set, frozenset, dict)) and len(v) == 0):
            raise ValueError(f'{name}= is not served under rule="cp"')
    if dtype is not None and not ops.attn_bwd_dv_ok(dtype, head_dim):
        raise ValueError(f'rule="cp": no dV attention kernel for {dtype} at head_dim {head_dim}')
    return rule


def cp_layer_bwd(eng, li, st, Lw, Gs, B, S, row_iv=None, top=None, Gm=None, rel=None):
    """one decoder layer's CP-LRP backward: G [M, H] at the layer's output -> G' [M, H] at its input (buffer ("Gs", li & 1) of the arena).
         G_m = G Wd;  A_u = act(g) (*) G_m;  Gx2 = A_u W_up;  Gs1 = G + ln2 rstd2 (*) Gx2;  Gof = Gs1 Wo;
         dV = P^T Gof summed over the query heads of a kv group;  Gx = dV Wv;  G' = Gs1 + ln1 rstd1 (*) Gx
    top = (Gs_last, A_last, last): the sparse top layer -- everything above the attention runs on one row per prompt (rows `last` of the
    [M, .] operands; Gs is then not read) and the attention takes q_begin = S - 1.  Gm: G_m where the caller formed it already (latent
    "mlp").  rel: fp32 [M], the layer relevance sum_h h (*) G' (layer_relevance / latent "trace"), or None."""
    c, ar = eng.cfg, eng._arena
    H, I, d, nq, nk = c["hidden"], c["inter"], c["head_dim"], c["n_heads"], c["n_kv"]
    M, nqk = B * S, (nq + nk) * d
    lin = eng._lin_bwd
    if top is not None:
        Gs_last, A_last, last = top
        Gm = lin(A_last, Lw["wd"], ar.new("Gm_l", B, I)) if Gm is None else Gm
        Agu = ops.gated_cp_bwd_il(Gm, st["gu_l"], ar.new("Agu_l", B, 2 * I), eng.act)
        Gx2 = lin(Agu, Lw["wgu"], ar.new("Gx2_l", B, H))
        Gs1_l = ar.new("Gs1_l", B, H)
        ops.rmsnorm_bwd_add2(Gs_last, Gx2, Lw["ln2"], st["rstd2_l"], None, None, Gs1_l, None, None, 0.0, 0.0, 0.0)
        Gof_l = lin(Gs1_l, Lw["wo"], ar.new("Gof_l", B, nq * d))
        Gof = ar.zeros("Gof", M, nq * d).index_copy_(0, last, Gof_l)
        Gs1 = ar.zeros("Gs1", M, H).index_copy_(0, last, Gs1_l)
        q_begin = S - 1
    else:
        Gm = lin(Gs, Lw["wd"], ar.wide("Gm", M, I)) if Gm is None else Gm
        Agu = ops.gated_cp_bwd_il(Gm, st["gu"], ar.wide("Agu", M, 2 * I), eng.act)
        Gs1 = ar.new("Gs1", M, H)
        if (eng._norm_fused(M) and ops.norm_fusion_part("bwd_gu")
                and ops.norm_fused_ok(M, H, 2 * I, Agu.stride(0), Lw["wgu"].stride(0), True, eng.dtype)):
            ops.gemm_nn_rs_res(Agu, Lw["wgu"], st["rstd2"], Gs, Gs1)          # K1n: the norm's row scale and the residual in the dgrad's epilogue
        else:
            Gx2 = lin(Agu, Lw["wgu"], ar.new("Gx2", M, H))
            ops.rmsnorm_bwd_add2(Gs, Gx2, Lw["ln2"], st["rstd2"], None, None, Gs1, None, None, 0.0, 0.0, 0.0)
        Gof = lin(Gs1, Lw["wo"], ar.new("Gof", M, nq * d))
        q_begin = 0
    qkr = st["qkr"]
    Gof_t = ops.transpose_heads(Gof, B, S, nq, d) if eng.attn_t else None
    dv = ar.new("dv", M, nk * d)
    ops.attn_bwd_dv(qkr[:, : nq * d], qkr[:, nq * d:], Gof, st["lse"], dv, B, S, nq, nk, d, d ** -0.5, q_begin=q_begin, row_iv=row_iv, G_t=Gof_t)
    Gx = lin(dv, Lw["wqkv"][nqk:], ar.new("Gx", M, H))          # the V rows of the fused weight: a row slice at the same pitch
    Gout = ar.new(("Gs", li & 1), M, H)
    ops.rmsnorm_bwd_add2(Gs1, Gx, Lw["ln1"], st["rstd1"], st["h"] if rel is not None else None, None, Gout, None, rel, 0.0, 0.0, 0.0)
    return Gout
