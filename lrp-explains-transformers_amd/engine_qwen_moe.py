"""Whole-model AttnLRP engine for Qwen3-MoE (Qwen3MoeForCausalLM; Qwen3-30B-A3B and the like), efficient placement
(ref wiring: lxt/efficient/models/qwen3_moe.py; the router is left to plain autograd there).

A layer is QwenLRP's Qwen3 attention half -- per-head q / k RMSNorm, on the fused launch sequence where its GEMMs take the shape (bf16, M = B S
rows: engine.fused_qkv_fwd / fused_attn_fwd / fused_attn_bwd), else kernel by kernel (fp32, the parity engine, and small row counts) -- and
then either the dense gated MLP (mlp_only_layers / decoder_sparse_step) or the sparse block:
    forward   xn = rstd2 (.) ln2 (.) h1 (row kernel; ln2 is NOT folded into the expert weights -- they are read as stored, no copy),
              logits = xn Wr^T, ops.moe_router_fwd -> (idx, w, lse), ops.MoePlan, moe_gate_up_fwd, moe_down_fwd, moe_combine(y, plan, w), h1 + out
    backward  moe_down_dgrad -> (Agu, G_w);  G_xn = moe_combine(moe_gate_up_dgrad(Agu)) + moe_router_bwd(G_w) Wr;  the norm's identity rule
              (rstd held constant) and the residual: Gs1 = G + ln2 (.) rstd2 (.) G_xn
Stash per MoE layer: the coefficients [T k, 2 I] and m [T k, I], the int32 plan, and the router's logits, lse, idx, w.
explain(experts=True) adds R_expert [L, B, E] (ops.moe_expert_relevance: `routing_weights * routing_weights.grad` scattered by expert and
summed over a prompt's tokens; = 1/2 of the block-output relevance when summed over the experts) and expert_index [L, B, S, k].
weight_format="mxfp4": the routed experts -- almost all of the parameters -- are resident ONLY as MXFP4 codes + scales (views of the uint8
buffer flat_q) and the four grouped GEMMs decode them in their staging loads (ops.MoeQuantWeight): no scratch copy, no
dequant launch, forward / backward below unchanged.
explain(moe_weights=...) adds R_W, the per-weight relevance `weight * weight.grad` of the attention Linears, the router and the routed
experts' gate_up_proj / down_proj (moe_weight_request, MoeWeightSink; ops.moe_wgrad_rel)."""
import operator

import torch

from . import engine as E
from . import engine_qwen as Q
from . import ops
from .efficient.moe import _ACTS


def config_from_hf(hf_cfg):
    """HF Qwen3MoeConfig -> engine cfg.  What the driver does not implement is refused here, before any kernel runs."""
    mt = getattr(hf_cfg, "model_type", None)
    if mt != "qwen3_moe":
        raise NotImplementedError(f"Qwen3MoeLRP drives Qwen3-MoE decoders only (model_type={mt!r}); dense Qwen2 / Qwen3 run on "
                                  "lxt_amd.engine_qwen.QwenLRP, Llama on lxt_amd.engine.LlamaLRP, other families through "
                                  "lxt_amd.efficient.monkey_patch")
    nL = hf_cfg.num_hidden_layers
    types = getattr(hf_cfg, "layer_types", None)
    if getattr(hf_cfg, "use_sliding_window", False) or (types is not None and any(t != "full_attention" for t in list(types)[:nL])):
        raise NotImplementedError("Qwen3MoeLRP: sliding-window layers (use_sliding_window=True / layer_types other than 'full_attention') are "
                                  "not supported by the fused driver (use the monkey_patch drop-in path)")
    if getattr(hf_cfg, "attention_bias", False) or getattr(hf_cfg, "mlp_bias", False):
        raise NotImplementedError("Qwen3MoeLRP: attention_bias / mlp_bias = True are not supported by the fused driver (use the monkey_patch "
                                  "drop-in path)")
    act = getattr(hf_cfg, "hidden_act", "silu")
    act = "gelu_tanh" if act == "gelu_pytorch_tanh" else act
    if act not in _ACTS:
        raise NotImplementedError(f"Qwen3MoeLRP: activation {act!r} is not served (the grouped expert kernels implement {', '.join(_ACTS)})")
    H, Im, Ne, k = hf_cfg.hidden_size, hf_cfg.moe_intermediate_size, hf_cfg.num_experts, hf_cfg.num_experts_per_tok
    if H % 128 or Im % 128:
        raise NotImplementedError(f"Qwen3MoeLRP: hidden size {H} and moe_intermediate_size {Im} must be multiples of 128 (the grouped GEMMs' "
                                  "128 x 128 tiles)")
    if Ne > ops.ROUTER_EMAX or k > ops.ROUTER_KMAX or not 1 <= k <= Ne:
        raise NotImplementedError(f"Qwen3MoeLRP: top-{k} of {Ne} experts; the routing plan serves at most {ops.ROUTER_EMAX} experts and the "
                                  f"router kernel at most {ops.ROUTER_KMAX} per token")
    kind = E.rope_kind(hf_cfg)
    if kind not in E._STATIC_ROPE:
        raise NotImplementedError(f"Qwen3MoeLRP: rope_type {kind!r} (sequence-length dependent frequencies) is not supported")
    hd = getattr(hf_cfg, "head_dim", None) or H // hf_cfg.num_attention_heads
    rp = getattr(hf_cfg, "rope_parameters", None)
    theta = rp.get("rope_theta") if isinstance(rp, dict) else None
    if theta is None:
        theta = getattr(hf_cfg, "rope_theta", 10000.0)
    only, step = set(getattr(hf_cfg, "mlp_only_layers", None) or ()), int(getattr(hf_cfg, "decoder_sparse_step", 1))
    cfg = dict(hidden=H, inter=hf_cfg.intermediate_size, n_layers=nL, n_heads=hf_cfg.num_attention_heads, n_kv=hf_cfg.num_key_value_heads,
               head_dim=hd, vocab=hf_cfg.vocab_size, rope_theta=float(theta), rms_eps=float(hf_cfg.rms_norm_eps), act=act, family=mt,
               qkv_bias=False, qk_norm=True, tied=bool(getattr(hf_cfg, "tie_word_embeddings", False)), moe_inter=Im, n_experts=Ne, top_k=k,
               norm_topk=bool(getattr(hf_cfg, "norm_topk_prob", False)),
               moe_layers=tuple(li not in only and Ne > 0 and (li + 1) % step == 0 for li in range(nL)))      # (HF Qwen3MoeDecoderLayer.__init__)
    if kind != "default":
        from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS
        inv_freq, att = ROPE_INIT_FUNCTIONS[kind](hf_cfg, "cpu")
        cfg["inv_freq"], cfg["attention_scaling"] = inv_freq.float().cpu(), float(att)
    return cfg


def weights_from_hf(model):
    """plain (cfg, W) view of a HF Qwen3MoeForCausalLM (no copies).  A MoE layer holds wr (the router), wgu_e [E, 2 I, H] and wd_e [E, H, I]
    (HF's gate_up_proj / down_proj) in place of wg / wu / wd"""
    cfg = config_from_hf(model.config)
    m = model.model
    W = dict(embed=m.embed_tokens.weight.detach(), norm=m.norm.weight.detach(), layers=[])
    if model.lm_head.weight.data_ptr() != m.embed_tokens.weight.data_ptr():
        W["lm_head"], cfg["tied"] = model.lm_head.weight.detach(), False
    else:
        cfg["tied"] = True
    for li, L in enumerate(m.layers):
        a, mlp = L.self_attn, L.mlp
        if a.o_proj.bias is not None or a.q_proj.bias is not None:
            raise NotImplementedError("Qwen3MoeLRP: a bias on the attention projections is not supported by the fused driver")
        Lw = dict(ln1=L.input_layernorm.weight.detach(), ln2=L.post_attention_layernorm.weight.detach(), wq=a.q_proj.weight.detach(),
                  wk=a.k_proj.weight.detach(), wv=a.v_proj.weight.detach(), wo=a.o_proj.weight.detach(), qn=a.q_norm.weight.detach(),
                  kn=a.k_norm.weight.detach())
        if cfg["moe_layers"][li]:
            Lw.update(wr=mlp.gate.weight.detach(), wgu_e=mlp.experts.gate_up_proj.detach(), wd_e=mlp.experts.down_proj.detach())
        else:
            if any(t.bias is not None for t in (mlp.gate_proj, mlp.up_proj, mlp.down_proj)):
                raise NotImplementedError("Qwen3MoeLRP: a bias in the dense MLP is not supported by the fused driver")
            Lw.update(wg=mlp.gate_proj.weight.detach(), wu=mlp.up_proj.weight.detach(), wd=mlp.down_proj.weight.detach())
        W["layers"].append(Lw)
    return cfg, W


EXPERT_FORMATS = (None, "mxfp4")
EXPERT_TENSORS = ("wgu_e", "wd_e")


def expert_format_request(weight_format):
    """Qwen3MoeLRP(weight_format=...) -> the format; an unknown name raises ValueError before any device work.  (No grid check: config_from_hf
    already holds hidden and moe_intermediate_size, the two block directions, to multiples of 128.)"""
    if not any(weight_format is f or (isinstance(weight_format, str) and weight_format == f) for f in EXPERT_FORMATS):
        raise ValueError(f"weight_format must be one of {EXPERT_FORMATS}, got {weight_format!r}")
    return weight_format


def expert_bytes(n_sparse, n_experts, hidden, moe_inter, weight_format, dtype):
    """exact bytes of the routed experts of n_sparse layers as held: 3 H I parameters per expert, 4 + 8 / 32 bits each as MXFP4"""
    n = n_sparse * n_experts * 3 * hidden * moe_inter
    return n // 2 + n // ops.MX_BLOCK if weight_format == "mxfp4" else n * torch.empty((), dtype=dtype).element_size()


def expert_quant_layout(cfg):
    """one uint8 spec per layer for E.pack_flat: a sparse layer's codes [E, N, K / 2] and scales [E, N, K / 32] of gate_up_proj [E, 2 I, H] and
    down_proj [E, H, I]; a dense layer holds nothing there"""
    Ne, H, Im = cfg["n_experts"], cfg["hidden"], cfg["moe_inter"]
    spec = {}
    for k, (N, K) in zip(EXPERT_TENSORS, ((2 * Im, H), (H, Im))):
        spec[k + "_c"] = ((Ne, N, K // 2), None)
        spec[k + "_s"] = ((Ne, N, K // ops.MX_BLOCK), None)
    return [spec if moe else {} for moe in cfg["moe_layers"]]


MOE_WEIGHTS = ("qkv", "o", "router", "gate_up", "down")
MOE_WEIGHTS_SPARSE = ("router", "gate_up", "down")          # one row per requested SPARSE layer; qkv / o: one per requested layer


def moe_weight_shapes(cfg):
    """{name: shape of one layer's matrix}: qkv / o in HF row order (q | k | v rows), router = gate.weight [E, H], gate_up =
    experts.gate_up_proj [E, 2 I, H] ([gate | up] rows), down = experts.down_proj [E, H, I]"""
    H, Im, Ne, nq, nk, d = cfg["hidden"], cfg["moe_inter"], cfg["n_experts"], cfg["n_heads"], cfg["n_kv"], cfg["head_dim"]
    return dict(qkv=((nq + 2 * nk) * d, H), o=(H, nq * d), router=(Ne, H), gate_up=(Ne, 2 * Im, H), down=(Ne, H, Im))


def moe_weight_request(moe_weights, weight_layers, weights_out, cfg, dtype, mode="efficient", graph=False):
    """explain(moe_weights=..., weight_layers=..., weights_out=...) -> (names, layers, moe): the requested matrices in MOE_WEIGHTS order, the
    ascending layer indices (default: every layer) and the sparse ones among them; moe_weights=None -> ((), (), ()).  Raises ValueError before
    a kernel of the model runs: an unknown name, a non-iterable, layer indices that are not ascending integers in [0, L) (negative indices
    are not wrapped), weight_layers / weights_out without names, a placement other than the efficient one, graph=True, router / gate_up /
    down when no requested layer is sparse, a bf16 qkv / o / router matrix off lrp_wgrad_rel's grid of 8 (the expert tensors are on it:
    config_from_hf), or a weights_out that is not a previous call's R_W for the same names and layers"""
    nL = len(cfg["moe_layers"])
    if moe_weights is None:
        if weight_layers is not None or weights_out is not None:
            raise ValueError("weight_layers / weights_out need moe_weights=...")
        return (), (), ()
    try:
        names = (moe_weights,) if isinstance(moe_weights, str) else tuple(moe_weights)
    except TypeError:
        raise ValueError(f"moe_weights must be an iterable of names from {MOE_WEIGHTS}, got {moe_weights!r}") from None
    bad = [n for n in names if n not in MOE_WEIGHTS]
    if bad:
        raise ValueError(f"moe_weights: unknown matrix name(s) {bad}; choose from {MOE_WEIGHTS}")
    names = tuple(n for n in MOE_WEIGHTS if n in names)
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
        return (), (), ()
    if mode != "efficient":
        raise ValueError(f"moe_weights: the per-weight relevance is defined for the efficient placement only, not mode={mode!r}")
    if graph:
        raise ValueError("moe_weights: graph=True is not supported (R_W is allocated, or accumulated into the caller's tensors, per call)")
    moe = tuple(l for l in layers if cfg["moe_layers"][l])
    sparse = [n for n in names if n in MOE_WEIGHTS_SPARSE]
    if sparse and not moe:
        raise ValueError(f"moe_weights: {sparse} belong to sparse layers and none of the requested layers {list(layers)} is sparse")
    shapes = moe_weight_shapes(cfg)
    if dtype == torch.bfloat16:
        for n in names:
            if len(shapes[n]) == 2 and (shapes[n][0] % 8 or shapes[n][1] % 8):
                raise ValueError(f"moe_weights: the bf16 kernel needs both sizes of {n!r} {shapes[n]} to be multiples of 8")
    if weights_out is not None:
        if not isinstance(weights_out, dict) or set(weights_out) != set(names):
            raise ValueError(f"weights_out must be a previous call's R_W with exactly the matrices {list(names)}")
        for n in names:
            t, want = weights_out[n], (len(moe) if n in MOE_WEIGHTS_SPARSE else len(layers), *shapes[n])
            if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != want or not t.is_contiguous():
                raise ValueError(f"weights_out[{n!r}] must be a contiguous float32 {list(want)} tensor")
    return names, layers, moe


class MoeWeightSink:
    """the per-weight relevance of one Qwen3-MoE explanation, built like engine.WeightSink: out[name] fp32, qkv / o [len(layers), N, K] and
    router / gate_up / down [len(moe), E, ...] in HF order, one launch per requested matrix and layer on the buffers the backward has just
    left -- ops.wgrad_rel for the dense matrices (called as a WeightSink: engine.fused_attn_bwd takes it in that place), ops.moe_wgrad_rel
    for the expert tensors.  A layer or a name that was not requested launches nothing.  prev: a previous call's R_W -- this call's values
    are ADDED to it in place.  Operands:
        qkv      G = Aqkv (the gradient at the fused QKV Linear's output), X = the normed input rows (folded ln1: h with rs = rstd1)
        o        G = Gs1 (the gradient at h1; no stabiliser on the residual add), X = o (the attention's output)
        router   G = Glogits (moe_router_bwd), X = x2 = rstd2 (.) ln2 (.) h1
        gate_up  G = Agu in plan rows (moe_down_dgrad), X = x2 gathered by token
        down     G = Gs (the gradient at the layer's output) gathered by token, scaled by 1/2 w; X = m in plan rows"""

    def __init__(self, req, cfg, device, prev=None):
        names, self.layers, self.moe = req
        shapes = moe_weight_shapes(cfg)
        self.slot, self.mslot = {l: i for i, l in enumerate(self.layers)}, {l: i for i, l in enumerate(self.moe)}
        self.accumulate, self.li = prev is not None, None
        if prev is not None and any(t.device != torch.empty(0, device=device).device for t in prev.values()):          # ("cuda" -> "cuda:N")
            raise ValueError(f"weights_out must live on {device}")
        rows = lambda n: len(self.moe) if n in MOE_WEIGHTS_SPARSE else len(self.layers)      # noqa: E731
        self.out = {n: torch.empty(rows(n), *shapes[n], device=device, dtype=torch.float32) for n in names} if prev is None else prev

    def layer(self, li):
        """-> the sink positioned at layer li, or None when nothing of that layer was requested"""
        self.li = li
        return self if li in self.slot else None

    def wants(self, *names):
        return any(n in self.out for n in names)

    def __call__(self, name, G, X, W, rs=None):
        """a dense matrix: G the gradient at the Linear's output, X its input (with rs = 1 / rms when X is un-normed)"""
        if name in self.out:
            slot = self.mslot[self.li] if name in MOE_WEIGHTS_SPARSE else self.slot[self.li]
            ops.wgrad_rel(G, X, W, out=self.out[name][slot], rs=rs, accumulate=self.accumulate)

    def experts(self, name, G, X, W, plan, w=None):
        """an expert tensor of the sparse layer the sink is positioned at (ops.moe_wgrad_rel's operands)"""
        if name in self.out:
            ops.moe_wgrad_rel(G, X, W, plan, name, w=w, out=self.out[name][self.mslot[self.li]], accumulate=self.accumulate)


class Qwen3MoeLRP(Q.QwenLRP):
    """QwenLRP for Qwen3-MoE: cfg carries moe_layers (which layers are sparse), n_experts, top_k, norm_topk, moe_inter (config_from_hf);
    W["layers"][i] of a sparse layer holds wr, wgu_e, wd_e.  The expert weights stay the caller's tensors (moved to the engine's device and
    dtype only if they are elsewhere); everything else lives in the flat buffer.  explain() is LlamaLRP.explain plus `experts`.
    weight_format="mxfp4": wgu_e / wd_e of every sparse layer are ops.MoeQuantWeight views of ONE uint8 buffer flat_q (128-byte aligned views)
    and nothing else of them is kept -- a multi-GPU start-up is dist.broadcast_weights([eng.flat, eng.flat_q]).  Attention, router, dense
    layers' MLPs, norms, embedding and head stay in `flat` in the model dtype: the base classes see weight_format=None."""

    def __init__(self, cfg, W, dtype=torch.bfloat16, device="cuda", mode="efficient", max_seq=4096, sparse_top=False, fold_norm=None, **storage):
        """storage: weight_format=None | "mxfp4", the format of the ROUTED EXPERTS alone.  It is keyword-only and not a named parameter: the
        dense drivers' weight_format (all four Linears of a layer through a scratch, engine.weight_format_request) is a different contract,
        which this driver does not take -- tests/test_mxfp4_cpu.py holds its signature to that"""
        unknown = set(storage) - {"weight_format"}
        if unknown:
            raise TypeError(f"Qwen3MoeLRP() got unexpected keyword argument(s) {sorted(unknown)}")
        self.expert_format = expert_format_request(storage.get("weight_format"))
        self._af_cache = {}
        self._eq_flat = self._eq_layers = None      # the experts' uint8 buffer while the layers load (the base constructor owns the name flat_q)
        super().__init__(cfg, W, dtype=dtype, device=device, mode=mode, max_seq=max_seq, sparse_top=False, fold_norm=fold_norm)
        self.flat_q = self._eq_flat

    @staticmethod
    def flat_layout(cfg, dtype):
        """one spec per layer: a sparse layer keeps the attention half's weights and the router [E, H]; a dense one is QwenLRP's layer"""
        top, dense = E.LlamaLRP.flat_layout(cfg, dtype)
        sparse = {k: v for k, v in dense.items() if k not in ("wgu", "wd")}
        sparse["wr"] = ((cfg["n_experts"], cfg["hidden"]), None)
        return top, [sparse if moe else dense for moe in cfg["moe_layers"]]

    def _put_layer(self, Lw, L):
        if "wr" not in L:
            return super()._put_layer(Lw, L)
        for k in ("ln1", "ln2", "wo", "qn", "kn", "wr"):
            E.put_rows(Lw[k], L[k])
        E.put_rows(Lw["wqkv"], L["wq"], L["wk"], L["wv"])
        if self.folded:          # (ln1 into the QKV columns as in the dense layers; ln2 stays a vector: the expert weights are read as stored)
            E.fold_rows(Lw["wqkv"], (Lw["wqkv"],), L["ln1"])
            Lw["ln1"].fill_(1.0)
        li = next(i for i, x in enumerate(self.layers) if x is Lw)
        if self.expert_format is not None and self._eq_flat is None:
            self._eq_flat, _, self._eq_layers = E.pack_flat({}, expert_quant_layout(self.cfg), len(self.layers), torch.uint8, self.device, align=128)
        for k in EXPERT_TENSORS:
            # one expert tensor at a time: on the device in the engine dtype, quantised into its views, and dropped -- the peak at load is
            # what is resident plus one tensor (a CPU-resident model loads even when its bf16 experts would not fit the device)
            w = L[k].detach().to(device=self.device, dtype=self.dtype)
            if not w.is_contiguous():
                raise NotImplementedError("Qwen3MoeLRP: gate_up_proj / down_proj must be contiguous (the grouped kernels read them as stored)")
            if self.expert_format is None:
                Lw[k] = w
                continue
            if not bool(torch.isfinite(w).all()):
                raise ValueError(f"weight_format={self.expert_format!r}: layer {li} holds non-finite expert weights ({k})")
            Lw[k] = ops.MoeQuantWeight(w, self._eq_layers[li][k + "_c"], self._eq_layers[li][k + "_s"])
            del w

    def _load_layer(self, li, only=()):
        """nothing to load: the quantised experts are read in place by the grouped GEMMs"""

    def weight_bytes(self):
        """LlamaLRP.weight_bytes (resident: `flat` + `flat_q`, scratch: 0 -- there is none) plus experts: the exact bytes of the routed
        experts as held -- codes + scales, or the tensors in the model dtype (weight_format=None: those are not part of `flat`)"""
        out = super().weight_bytes()
        held = [Lw[k] for Lw in self.layers if "wr" in Lw for k in EXPERT_TENSORS]
        out["experts"] = sum(t.nbytes() if isinstance(t, ops.MoeQuantWeight) else t.numel() * t.element_size() for t in held)
        return out

    def dequantized_weights(self):
        """-> (cfg, W) in the form weights_from_hf gives and Qwen3MoeLRP(cfg, W) takes, holding what this engine computes with: the experts
        dequantised exactly in the engine dtype, everything else as stored (q / k / v split, a dense layer's gate / up de-interleaved, folded
        norm vectors as ones: an engine built from it folds by exactly 1.0 and ends up with the same bits).  Whole-model copies: for checks"""
        c = self.cfg
        nq, nk, d, I = c["n_heads"], c["n_kv"], c["head_dim"], c["inter"]
        W = dict(embed=self.embed.clone(), norm=self.norm.clone(), layers=[])
        if self.lm_head is not self.embed:
            W["lm_head"] = self.lm_head.clone()
        for Lw in self.layers:
            wq, wk, wv = (t.clone() for t in Lw["wqkv"].split((nq * d, nk * d, nk * d), 0))
            L = dict(ln1=Lw["ln1"].clone(), ln2=Lw["ln2"].clone(), wq=wq, wk=wk, wv=wv, wo=Lw["wo"].clone(), qn=Lw["qn"].clone(),
                     kn=Lw["kn"].clone())
            if "wr" in Lw:
                L["wr"] = Lw["wr"].clone()
                for k in EXPERT_TENSORS:
                    L[k] = Lw[k].dequant(self.dtype) if isinstance(Lw[k], ops.MoeQuantWeight) else Lw[k].clone()
            else:
                gu = Lw["wgu"].unflatten(0, (I // ops.GATED_IL, 2, ops.GATED_IL))
                L.update(wg=gu[:, 0].reshape(I, -1).clone(), wu=gu[:, 1].reshape(I, -1).clone(), wd=Lw["wd"].clone())
            W["layers"].append(L)
        torch.cuda.synchronize(self.device)
        return dict(c), W

    def set_mode(self, mode):
        if mode == "explicit":
            raise NotImplementedError("Qwen3MoeLRP: mode='explicit' is not implemented -- the reference defines no explicit composite for "
                                      "Qwen3-MoE; the driver runs the efficient placement only")
        super().set_mode(mode)

    def build_transposes(self):
        for L in self.layers:
            ops.clear_weight_cache(*(L[k] for k in ("wqkv", "wo", "wgu", "wd", "wr") if k in L))
        self.lm_head_t = None

    def _fused(self, M):
        """fused_layer_ok of the DENSE layers' shapes (the sparse layers have no wgu / wd); without a dense layer nothing of it applies"""
        dense = next((Lw for Lw in self.layers if "wgu" in Lw), None)
        if dense is None:
            return E.FusedOk(False, False, False, False)
        return E.fused_layer_ok(M, dense, self.meta, self.dtype, self._nf_cache)

    def _attn_fused(self, M):
        """the attention half of every layer runs on the fused launch sequence at M rows: folded norm weights, and each of its four GEMMs is
        a problem the ping-pong kernel's fused epilogues take (bf16, >= 190 tiles), the dQ kernel forms D, head dim 64 or 128"""
        key = (M, E.PITCH_PAD, repr(ops.NORM_FUSION), ops.PREP_FUSION)
        hit = self._af_cache.get(key)
        if hit is None:
            nq, nk, d = self.meta[:3]
            H, nqkv, dt, Lw = self.cfg["hidden"], (nq + 2 * nk) * d, self.dtype, self.layers[0]
            ldo, ldqkv = Lw["wo"].stride(0), Lw["wqkv"].stride(0)
            hit = self._af_cache[key] = bool(
                self.folded and ops.NORM_FUSION is True and self.mode == "efficient" and not self.attn_t and d in (64, 128)
                and ops.attn_dq_d_ok(dt, d)
                and ops.norm_fused_ok(M, H, nq * d, nq * d, ldo, False, dt)                                        # h1 = h + o Wo^T
                and ops.norm_fused_ok(M, nqkv, H, H, ldqkv, False, dt)                                             # qkv = rstd (h W'qkv^T)
                and ops.norm_fused_ok(M, nq * d, H, H, ldo, True, dt)                                              # Gho = 1/2 (Gs1 Wo)
                and ops.norm_fused_ok(M, H, nqkv, E.fused_layout(H, 0, nq, nk, d, dt)["Aqkv"], ldqkv, True, dt))   # G_h = rstd (Aqkv W'qkv) + Gs1
        return hit

    # ---------------------------------------------------------------------------------------------
    def forward(self, emb, B, S, row_iv=None, keep_m=False, experts=False, rows=None):
        """experts: every sparse block's output is kept for the R_block read-out of the backward; rows: LlamaLRP.forward's"""
        c, ar = self.cfg, self._arena
        H, I, d, nq, nk, eps = c["hidden"], c["inter"], c["head_dim"], c["n_heads"], c["n_kv"], c["rms_eps"]
        M, nqk, nqkv, scale = B * S, (nq + nk) * d, (nq + 2 * nk) * d, d ** -0.5
        last = torch.arange(B, device=self.device) * S + (S - 1) if rows is None else rows
        fa, coef = self._attn_fused(M), self._gated_coef(M)
        stash, h_prev, branch = [], emb, None
        for li, Lw in enumerate(self.layers):
            st = dict(rstd1=ar.f32(("rstd1", li), M), moe="wr" in Lw)
            x = None if fa else ar.new("x", M, H)          # (fused: the QKV GEMM's epilogue applies the norm; only the sum and rstd1 are formed)
            if branch is None:
                st["h"] = h_prev
                ops.add_rmsnorm_fwd(h_prev, None, Lw["ln1"], eps, y=x, rstd=st["rstd1"], norm_out=not fa)
            else:
                st["h"] = ar.new(("h", li), M, H)
                ops.add_rmsnorm_fwd(h_prev, branch, Lw["ln1"], eps, hsum_out=st["h"], y=x, rstd=st["rstd1"], norm_out=not fa)
            qkn = self._qk_norm(Lw)
            # ---- attention half -> h1, rstd2 and x2 = rstd2 (.) ln2 (.) h1
            x2 = ar.new("x2", M, H)
            if fa:
                qkv, qkr, st["rstd_q"], st["rstd_k"] = E.fused_qkv_fwd(st["h"], st["rstd1"], Lw["wqkv"], self.cos, self.sin, S, self.meta,
                                                                      self._alloc(li), qk_norm=qkn)
                st.update(E.fused_attn_fwd(st["h"], qkv, qkr, Lw, B, S, self.meta, self._alloc(li), row_iv)[0], qkv=qkv, qkr=qkr)
                ops.rmsnorm_bwd_add2(None, st["h1"], Lw["ln2"], st["rstd2"], None, None, x2, None)      # (the row-scale kernel: x w rstd)
            else:
                qkv, qn = ops.linear_fwd(x, Lw["wqkv"], out=ar.new(("qkv", li), M, nqkv)), ar.new("qkn", M, nqk)
                st["rstd_q"], st["rstd_k"] = ar.f32(("rstd_q", li), M * nq), ar.f32(("rstd_k", li), M * nk)
                ops.head_rmsnorm_fwd(qkv[:, : nq * d], qkn[0], qn[:, : nq * d], st["rstd_q"], nq, d, eps)
                ops.head_rmsnorm_fwd(qkv[:, nq * d: nqk], qkn[1], qn[:, nq * d:], st["rstd_k"], nk, d, eps)
                qkr = ops.rope_fwd(qn, ar.new(("qkr", li), M, nqk), self.cos, self.sin, S, nq + nk, d)
                v = qkv[:, nqk:]
                v_t = ops.transpose_heads(v, B, S, nk, d) if self.attn_t else None
                o, lse = ar.new(("o", li), M, nq * d), ar.f32(("lse", li), B, nq, S)
                ops.attn_fwd(qkr[:, : nq * d], qkr[:, nq * d:], v, v_t, o, lse, B, S, nq, nk, d, scale, True, 0, row_iv=row_iv)
                a = self._lin_fwd(o, Lw["wo"], ar.new("a", M, H))
                st.update(qkv=qkv, qkr=qkr, o=o, lse=lse, h1=ar.new(("h1", li), M, H), rstd2=ar.f32(("rstd2", li), M))
                ops.add_rmsnorm_fwd(st["h"], a, Lw["ln2"], eps, hsum_out=st["h1"], y=x2, rstd=st["rstd2"])
            # ---- MLP half
            if st["moe"]:
                logits = ops.linear_fwd(x2, Lw["wr"], out=ar.new(("logits", li), M, c["n_experts"]))
                idx, w, lse_r = ops.moe_router_fwd(logits, c["top_k"], c["norm_topk"])
                plan = ops.MoePlan(idx, c["n_experts"])
                st["coef"], st["m"] = ops.moe_gate_up_fwd(x2, Lw["wgu_e"], plan, self.act)
                branch = ops.moe_combine(ops.moe_down_fwd(st["m"], Lw["wd_e"], plan), plan, w)
                st.update(logits=logits, lse_r=lse_r, idx=idx, w=w, plan=plan, out=branch if experts else None)
            else:
                gu, m = ar.new(("gu", li), M, 2 * I), ar.wide("m", M, I)
                if coef:
                    st["gu"], m = ops.gemm_gated_fwd_coef(x2, Lw["wgu"], gu, m, self.eps_g, self.eps["lin"], self.act)
                else:
                    st["gu"], m = ops.gemm_gated_fwd(x2, Lw["wgu"], gu, m, self.act)
                branch = self._lin_fwd(m, Lw["wd"], ar.new(("dn", li), M, H))
            stash.append(st)
            h_prev = st["h1"]
        return dict(stash=stash, last=last, row_iv=row_iv, coef=coef, fa=fa,
                    **E.head_fwd(ar, h_prev, branch, False, last, self.norm, self.lm_head, eps))

    # ---------------------------------------------------------------------------------------------
    def _weight_sink(self, req, prev):
        return MoeWeightSink(req, self.cfg, self.device, prev)

    def backward(self, fw, emb, idx, B, S, layer_relevance=False, seed=None, latent=frozenset(), heads=None, attn_map=None, experts=False,
                 weights=None):
        """-> (G at the embedding, layer_R rows or None, dict of the extra read-outs: R_resid [L+1, B, H]; experts: R_expert [L, B, E],
        expert_index [L, B, S, k] and R_block [L, B]); weights: a MoeWeightSink that collects R_W layer by layer, or None"""
        c, ar, dev, dt = self.cfg, self._arena, self.device, self.dtype
        H, I, d, nq, nk, Ne, k = c["hidden"], c["inter"], c["head_dim"], c["n_heads"], c["n_kv"], c["n_experts"], c["top_k"]
        M, rep, nqk, nqkv, scale = B * S, nq // nk, (nq + nk) * d, (nq + 2 * nk) * d, d ** -0.5
        Gh_last, Gs_last, _, rel_last = self._head_bwd(fw, idx, seed, layer_relevance)
        nL, lat = len(self.layers), {}
        if "resid" in latent:
            lat["R_resid"] = torch.empty(nL + 1, B, H, device=dev, dtype=torch.float32)
            ops.colsum_dot(fw["hL_last"], Gh_last, B, fw["last"].shape[0] // B, out=lat["R_resid"][nL])
        if experts:      # (dense layers: exactly 0 / -1)
            lat["R_expert"] = torch.zeros(nL, B, Ne, device=dev, dtype=torch.float32)
            lat["R_block"] = torch.zeros(nL, B, device=dev, dtype=torch.float32)
            lat["expert_index"] = torch.full((nL, B, S, k), -1, device=dev, dtype=torch.int64)
        last, row_iv, fa = fw["last"], fw["row_iv"], fw["fa"]
        Gs = ar.zeros(("Gs", nL & 1), M, H).index_copy_(0, last, Gs_last)
        layer_R = [rel_last] if layer_relevance else None
        if fa:
            ar.f32("half", M).fill_(0.5)          # (fused_attn_bwd's row scale)
        for li in range(nL - 1, -1, -1):
            Lw, st = self.layers[li], fw["stash"][li]
            hs = None if heads is None else heads.layer(li)
            am = None if attn_map is None else attn_map.layer(li)
            ws = None if weights is None else weights.layer(li)
            # ---- MLP half: Gs at the layer's output -> Gs1 at h1 (the norm's identity rule, rstd held constant, and the residual)
            Gs1 = ar.new("Gs1", M, H)
            if st["moe"]:
                Agu, gw = ops.moe_down_dgrad(Gs, Lw["wd_e"], st["coef"], st["m"], st["w"], st["plan"])
                if experts:
                    ops.moe_expert_relevance(st["idx"], st["w"], gw, B, S, Ne, out=lat["R_expert"][li])
                    torch.sum(ops.readout(st["out"], Gs, out=ar.f32("rel_blk", M)).view(B, S), 1, out=lat["R_block"][li])
                    lat["expert_index"][li].copy_(st["idx"].view(B, S, k))
                Gx_e = ops.moe_combine(ops.moe_gate_up_dgrad(Agu, Lw["wgu_e"], st["plan"]), st["plan"])
                Gl = ops.moe_router_bwd(st["logits"], st["lse_r"], st["idx"], st["w"], gw, c["norm_topk"], out=ar.new("Glogits", M, Ne))
                Gx_r = self._lin_bwd(Gl, Lw["wr"], ar.new("Gx2", M, H))
                if ws is not None:
                    ws.experts("down", Gs, st["m"], Lw["wd_e"], st["plan"], st["w"])
                    if ws.wants("gate_up", "router"):          # x2 once more: the forward keeps it in a scratch buffer only (the row-scale kernel)
                        x2 = ar.new("x2w", M, H)
                        ops.rmsnorm_bwd_add2(None, st["h1"], Lw["ln2"], st["rstd2"], None, None, x2, None)
                        ws.experts("gate_up", Agu, x2, Lw["wgu_e"], st["plan"])
                        ws("router", Gl, x2, Lw["wr"])
                Gs1e = ar.new("Gs1e", M, H)
                ops.rmsnorm_bwd_add2(Gs, Gx_e, Lw["ln2"], st["rstd2"], None, None, Gs1e, None)
                ops.rmsnorm_bwd_add2(Gs1e, Gx_r, Lw["ln2"], st["rstd2"], None, None, Gs1, None)
            else:
                if fw["coef"]:
                    Agu = ops.gemm_gated_bwd_coef(Gs, Lw["wd"], st["gu"], ar.wide("Agu", M, 2 * I))
                else:
                    Agu = ops.gemm_gated_bwd(Gs, Lw["wd"], st["gu"], ar.wide("Agu", M, 2 * I), self.eps_g, 0.0, self.act)
                Gx2 = self._lin_bwd(Agu, Lw["wgu"], ar.new("Gx2", M, H))
                ops.rmsnorm_bwd_add2(Gs, Gx2, Lw["ln2"], st["rstd2"], None, None, Gs1, None)
            # ---- attention half: Gs1 -> Gs at the layer's input
            qkn = self._qk_norm(Lw)
            if fa:
                Gs = E.fused_attn_bwd(Gs1, st, Lw, self.cos, self.sin, B, S, self.meta, self._alloc(li), row_iv, qkn, hs, am, ws)
            else:
                qkv, qkr = st["qkv"], st["qkr"]
                q, kk, v = qkr[:, : nq * d], qkr[:, nq * d:], qkv[:, nqk:]
                Gof = self._lin_bwd(Gs1, Lw["wo"], ar.new("Gof", M, nq * d))
                Gho, D = ar.new("Gho", M, nq * d), ar.f32("D", B, nq, S)
                ops.attn_bwd_prep(Gof, st["o"], Gho, D, B, S, nq, d, 0.0, 0.5)
                if hs is not None:
                    hs("out", st["o"], Gof)
                if am is not None:
                    am(q, kk, v, Gho, st["lse"], 2.0, row_iv)
                k_t = q_t = Gho_t = None
                if self.attn_t:
                    k_t, q_t = ops.transpose_heads(kk, B, S, nk, d), ops.transpose_heads(q, B, S, nq, d)
                    Gho_t = ops.transpose_heads(Gho, B, S, nq, d)
                dk_h, dv_h, dqk = ar.new("dk_h", M, nq * d), ar.new("dv_h", M, nq * d), ar.new("dqk", M, nqk)
                Aqkv = ar.new("Aqkv", M, nqkv)
                ops.attn_bwd_dq(q, kk, v, k_t, Gho, st["lse"], D, dqk[:, : nq * d], B, S, nq, nk, d, scale, 0.0, 0.0, row_iv=row_iv)
                ops.attn_bwd_dkv(q, kk, v, q_t, Gho, Gho_t, st["lse"], D, dk_h, dv_h, B, S, nq, nk, d, scale, 0.0, 0.0, row_iv=row_iv)
                if hs is not None:
                    hs("q", q, dqk[:, : nq * d])
                    hs("k", kk, dk_h, rep)
                    hs("v", v, dv_h, rep)
                ops.gqa_reduce(dk_h, dqk[:, nq * d:], M, nk, rep, d)
                ops.gqa_reduce(dv_h, Aqkv[:, nqk:], M, nk, rep, d)
                Gqk = ops.rope_bwd(dqk, None, None, ar.new("Gqkn", M, nqk), self.cos, self.sin, S, nq + nk, d, 0.0, 0.0)
                ops.head_rmsnorm_bwd(Gqk[:, : nq * d], qkn[0], st["rstd_q"], Aqkv[:, : nq * d], nq, d)
                ops.head_rmsnorm_bwd(Gqk[:, nq * d:], qkn[1], st["rstd_k"], Aqkv[:, nq * d: nqk], nk, d)
                if ws is not None:
                    ws("o", Gs1, st["o"], Lw["wo"])
                    if self.folded:          # folded ln1 is ones: the un-normed stream with rs = rstd1 IS the Linear's input
                        ws("qkv", Aqkv, st["h"], Lw["wqkv"], rs=st["rstd1"])
                    elif ws.wants("qkv"):    # the normed rows once more (the forward keeps them in a scratch buffer only)
                        xw = ar.new("xw", M, H)
                        ops.add_rmsnorm_fwd(st["h"], None, Lw["ln1"], c["rms_eps"], y=xw, rstd=ar.f32("xw_rstd", M))
                        ws("qkv", Aqkv, xw, Lw["wqkv"])
                Gx = self._lin_bwd(Aqkv, Lw["wqkv"], ar.new("Gx", M, H))
                Gs = ar.new(("Gs", li & 1), M, H)
                ops.rmsnorm_bwd_add2(Gs1, Gx, Lw["ln1"], st["rstd1"], None, None, Gs, None)
            if layer_relevance:
                layer_R.append(ops.readout(st["h"], Gs, out=ar.f32(("rel", li), M)))
            if "resid" in latent:
                ops.colsum_dot(st["h"], Gs, B, S, out=lat["R_resid"][li])
        return Gs, layer_R, lat

    @torch.no_grad()
    def explain(self, input_ids=None, inputs_embeds=None, target=None, layer_relevance=False, return_G=False, lengths=None, seed=None,
                graph=False, latent=None, heads=None, attn_map=None, experts=False, weights=None, moe_weights=None, weight_layers=None,
                weights_out=None, positions=None, position_weights=None, objective="logit", per_position=False):
        """LlamaLRP.explain for Qwen3-MoE (same arguments and outputs), with
        experts=True: two more outputs -- R_expert [L, B, E] fp32, the relevance of every expert of every layer per prompt (`routing_weights *
        routing_weights.grad` scattered by expert, summed over the prompt's tokens; rows of dense layers are exactly 0, pad tokens contribute
        exactly 0), expert_index [L, B, S, k] int64, the experts each token was routed to (-1 on dense layers), and R_block [L, B] fp32 =
        sum_{t, j} out (*) G at the sparse block's output (0 on dense layers), read off the block's own output and the gradient that reaches
        it: sum_e R_expert[l, b] = 1/2 R_block[l, b].  Every other output is bitwise what it is without the keyword.
        moe_weights (optional): names from {"qkv", "o", "router", "gate_up", "down"} -- the per-weight relevance `weight * weight.grad`
        (DESIGN.md section 17), R_W[name], all fp32 and summed over every token of every prompt of the call: qkv [len(weight_layers),
        (nq + 2 nk) d, H] (q_proj | k_proj | v_proj rows) and o [len(weight_layers), H, nq d] of every requested layer; router [len(moe), E, H]
        (mlp.gate.weight), gate_up [len(moe), E, 2 I, H] (experts.gate_up_proj, [gate | up] rows) and down [len(moe), E, H, I]
        (experts.down_proj) of the SPARSE layers among them; weight_layers, the requested layers, and weight_layers_moe, the sparse ones (the
        rows of the last three).  An expert that received no token is exactly 0; per expert, gate_up and down each sum to R_expert summed
        over the prompts.  weight_layers: ascending layer indices (default: all -- one 30B-A3B layer's gate_up + down are 604 M elements =
        2.42 GB of fp32, 48 layers ~116 GB: ask for the layers you need).  weights_out: a previous call's R_W; this call's values are added to
        it in place and it is returned (dataset-level accumulation).  weight_format="mxfp4" serves it from the codes (no dequantised copy).
        Efficient placement only, no graph=True; moe_weights=None launches nothing and every other output is bitwise what it is without it.
        Not part of it: the MLP matrices of dense (mlp_only_layers) layers, the monkey_patch drop-in, expert-parallel multi-GPU.
        Not served: latent="mlp" (a sparse layer has no single MLP), graph=True and weights= (LlamaLRP / QwenLRP's keyword: its names, shapes
        and layer lists are not this model's -- use moe_weights=) -- all raise ValueError.
        positions / position_weights / objective / per_position: LlamaLRP.explain's answer-span attribution, the same
        arguments, outputs and refusals; experts= and moe_weights= keep working with it (per_position=True takes no read-out keyword)."""
        if weights is not None:
            raise ValueError("Qwen3MoeLRP: weights= (per-weight relevance) is not supported for a model with routed experts; use moe_weights=")
        wr = moe_weight_request(moe_weights, weight_layers, weights_out, self.cfg, self.dtype, getattr(self, "mode", "efficient"), graph)
        names = (latent,) if isinstance(latent, str) else tuple(latent or ())
        if "mlp" in names:
            raise ValueError('Qwen3MoeLRP: latent="mlp" is not defined for a model with sparse layers (no single MLP per layer); '
                             '"trace" and "resid" are served')
        if graph:
            raise ValueError("Qwen3MoeLRP: graph=True is not supported (the routing plan and the expert stashes are allocated per call)")
        am = E.attn_map_request(attn_map, len(self.layers), self.cfg["n_heads"], self.cfg["head_dim"], self.dtype, self.mode)
        hd = E.head_request(heads, self.cfg["head_dim"], self.dtype)
        lat = E.latent_request(latent, self.cfg["hidden"], self.cfg["inter"], self.dtype)
        nb, ns = (input_ids.shape if inputs_embeds is None else inputs_embeds.shape[:2]) if positions is not None else (0, 0)
        span = E.position_request(positions, position_weights, objective, per_position, nb, ns, self.cfg["vocab"], getattr(self, "device", None),
                                  input_ids if inputs_embeds is None else None, target, lengths, seed, graph, getattr(self, "mode", "efficient"),
                                  bool(layer_relevance or return_G or latent or heads or attn_map or weights or moe_weights or experts))
        if span is not None:
            target = None
        B, S, emb, row_iv, idx = E.explain_inputs(input_ids, inputs_embeds, lengths, target, self.cfg["vocab"], self.max_seq, self.dtype,
                                                  self.device, seed)
        if inputs_embeds is None:
            input_ids = input_ids.to(self.device)
        out = self._run(input_ids, emb, B, S, row_iv, idx, layer_relevance, return_G, seed, lat, hd, am, wr, weights_out, span=span, experts=bool(experts))
        if wr[0]:
            out["weight_layers_moe"] = list(wr[2])
        return out

    def generate(self, *args, **kw):
        raise NotImplementedError("Qwen3MoeLRP: generate() / explain_generated() serve the dense LlamaLRP / QwenLRP drivers only (the decode "
                                  "step has no routed-expert layer); produce the answer elsewhere and pass it to explain(positions=...)")

    explain_generated = generate

    @classmethod
    def from_hf(cls, model, **kw):
        cfg, W = weights_from_hf(model)
        kw.setdefault("dtype", next(model.parameters()).dtype)
        return cls(cfg, W, **kw)
