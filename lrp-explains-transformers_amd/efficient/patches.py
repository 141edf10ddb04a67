"""Replacement forwards + patch plumbing: the drop-in surface of lxt.efficient.patches, HIP-backed.

Plumbing keeps the reference's contract (ref: lxt/efficient/patches.py:22-104): patching is
class-level and process-global, double patching is detected by comparing __module__ and answered
with a warning + False, there is no un-patch.  The forwards route every LRP-relevant op through
liblrp_hip.so (efficient/functions.py); they raise if handed CPU tensors (no fallback).
"""
from warnings import warn

import torch

from .rules import stop_gradient, divide_gradient, identity_rule_implicit, _act_name
from .functions import RMSNormFn, LayerNormFn, GatedActFn, LinearFn, AttentionFn, FusedGatedMLPFn, RopeFn, DecoderLayerFn


def check_already_patched(target_fn, new_fn):
    """True (with a warning) if target_fn already comes from this package's patch module"""
    if getattr(target_fn, "__module__", None) == getattr(new_fn, "__module__", object()):
        warn(f"{getattr(target_fn, '__name__', target_fn)} already patched.")
        return True
    return False


def patch_method(fn, module, method_name="forward", keep_original=False):
    """setattr(module, method_name, fn) unless already patched; returns success"""
    if check_already_patched(getattr(module, method_name), fn):
        return False
    if keep_original:
        setattr(module, f"original_{method_name}", getattr(module, method_name))
    setattr(module, method_name, fn)
    return True


def replace_module(patched_module, original_module):
    """copy every public attribute of patched_module onto original_module"""
    if original_module == patched_module:
        return False
    for attr in dir(patched_module):
        if not attr.startswith("__"):
            setattr(original_module, attr, getattr(patched_module, attr))
    return True


def _need_cuda(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: lxt_amd runs on the HIP device only (no CPU fallback); got a CPU tensor")


# ------------------------------------------------------------------------------------------- ownership
# The reference never touches nn.Linear / nn.LayerNorm / nn.Conv2d semantics for OTHER models in the process (its Linear
# stays ATen, lxt/efficient/models/llama.py:9-14).  The default maps here do patch those torch.nn classes -- so that every
# contraction of the explained model runs on liblrp_hip.so -- but the patched forwards only take the HIP path for module
# INSTANCES that belong to an explained model ("owned"); every other instance (a CPU probe, a second un-explained model,
# a module whose weights still require grad) runs its original forward, bit-identical to un-patched PyTorch.
# Ownership is given by adopt(model): called automatically the first time a model class of a patched modeling module is
# invoked (monkey_patch may run before or after the model is built), or by the user for models built from plain torch.nn.
_OWNABLE = (torch.nn.Linear, torch.nn.LayerNorm, torch.nn.Conv2d)


def adopt(model):
    """mark the nn.Linear / nn.LayerNorm / nn.Conv2d instances under `model` as part of an explained model"""
    for m in model.modules():
        if isinstance(m, _OWNABLE) or type(m).__name__ == "Conv1D":
            m.__dict__["_lrp_owned"] = True
        m.__dict__["_lrp_adopted"] = True
    return model


_WARNED = {}


def _owned(m):
    return m.__dict__.get("_lrp_owned", False)


def _operand(param):
    """a parameter as a Function's operand: the Parameter itself when it is trainable (autograd must see it), else a detached alias"""
    return param if param is None or param.requires_grad else param.detach()


def _adopting_call(self, *args, **kwargs):
    if not self.__dict__.get("_lrp_adopted", False):
        adopt(self)
    return torch.nn.Module.__call__(self, *args, **kwargs)


def patch_ownership(module):
    """give every PreTrainedModel class DEFINED in `module` an entry hook that adopts the instance on its first call"""
    try:
        from transformers import PreTrainedModel
    except Exception:  # noqa: BLE001
        return False
    for cls in list(vars(module).values()):
        if isinstance(cls, type) and issubclass(cls, PreTrainedModel) and cls.__module__ == module.__name__:
            if cls.__dict__.get("__call__") is not _adopting_call:
                cls.__call__ = _adopting_call
    return True


# ----------------------------------------------------------------------------------- AttnLRP patches
def rms_norm_forward(self, hidden_states):
    """identity rule on RMSNorm (ref: lxt/efficient/patches.py:111-123) -- fused HIP row kernel"""
    _need_cuda(hidden_states, "rms_norm_forward")
    eps = getattr(self, "variance_epsilon", None)
    if eps is None:
        eps = self.eps
    return RMSNormFn.apply(hidden_states, self.weight, float(eps), 0.0)


def gemma3_rms_norm_forward(self, x):
    """Gemma3RMSNorm: y = x*rstd*(1+w) (ref: lxt/efficient/models/gemma3.py:11-12 patches `_norm`;
    here the whole forward is one kernel with w_offset = 1)"""
    _need_cuda(x, "gemma3_rms_norm_forward")
    return RMSNormFn.apply(x, self.weight, float(self.eps), 1.0)


def layer_norm_forward(self, x):
    """identity rule on LayerNorm's 1/std (ref: lxt/efficient/patches.py:126-142); instances outside an explained model
    keep torch's own forward"""
    if not _owned(self) and hasattr(self, "original_forward"):
        if x.is_cuda and x.requires_grad and torch.is_grad_enabled() and not _WARNED.get("layer_norm"):
            # the reference's class-level patch covers EVERY nn.LayerNorm of the process; here only adopted instances take the rule
            _WARNED["layer_norm"] = True
            warn("lxt_amd.efficient: an nn.LayerNorm that is not part of an adopted model was called under autograd after monkey_patch; it "
                 "runs torch's own forward (plain gradient, NO identity rule on 1/std).  HuggingFace models of the patched module and "
                 "torchvision's VisionTransformer are adopted automatically; for any other model call lxt_amd.efficient.adopt(model) "
                 "(again after adding modules) so that its LayerNorm / Linear / Conv2d instances take the LRP rules.")
        return self.original_forward(x)
    _need_cuda(x, "layer_norm_forward")
    return LayerNormFn.apply(x, self.weight, self.bias, float(self.eps))


def linear_forward(self, x):
    """nn.Linear on the MFMA GEMM, forward and dgrad from the stored weight (bf16: no W^T copy; fp32: one cached on the weight).  Not patched by
    the reference (ATen mm there); part of the default maps here so the whole backward runs on liblrp_hip.so.  Only
    instances of an explained model take this path (see `adopt`); everything else -- foreign modules, CPU probes, dtypes the
    kernels do not serve -- runs torch's own forward unchanged.  A trainable weight / bias is handed over as the Parameter itself, so
    autograd sees it and LinearFn returns its plain gradient (lrp_wgrad / lrp_colsum_affine)."""
    w = self.weight
    if hasattr(self, "original_forward") and (not _owned(self) or x.dtype != w.dtype or x.dtype not in (torch.float32, torch.bfloat16)):
        return self.original_forward(x)
    _need_cuda(x, "linear_forward")
    return LinearFn.apply(x, _operand(w), _operand(self.bias))


def conv1d_forward(self, x):
    """HF's Conv1D (GPT-2's c_attn / c_fc / c_proj: y = x W + b with W stored [in, out]) on the MFMA GEMM: the forward
    uses a cached [out, in] copy (ops.weight_t), the dgrad the NN form on that copy (bf16) or the stored weight (fp32).  The reference leaves these
    on ATen (lxt/efficient/models/gpt2.py:11-32 patches only the MLP forward around them).  A trainable weight rides along as LinearFn's
    `stored` operand and gets its gradient in the stored [in, out] layout."""
    w = self.weight
    if hasattr(self, "original_forward") and (not _owned(self) or x.dtype != w.dtype or x.dtype not in (torch.float32, torch.bfloat16)):
        return self.original_forward(x)
    _need_cuda(x, "conv1d_forward")
    from .. import ops
    wd = w.detach()
    return LinearFn.apply(x, ops.weight_t(wd), _operand(self.bias), None, w if w.requires_grad else None)     # cached [out, in] copy


def conv2d_patch_forward(self, x):
    """nn.Conv2d whose stride equals its kernel (ViT / SigLIP patch embedding) as ONE GEMM over the unfolded patches:
    same arithmetic, un-patched (plain gradient) semantics as in the reference, but forward AND input-gradient run on
    liblrp_hip.so instead of MIOpen (whose backward-data solver search for the 896x896, 14x14/14 SigLIP stem takes
    minutes on a fresh box).  Any other convolution falls through to the original forward.  Trainable weight / bias: LinearFn's gradients."""
    kh, kw = self.kernel_size
    if (not _owned(self) or x.dim() != 4 or not x.is_cuda or tuple(self.stride) != (kh, kw) or self.groups != 1 or tuple(self.dilation) != (1, 1)
            or self.padding not in ((0, 0), "valid", 0) or self.padding_mode != "zeros" or x.dtype not in (torch.float32, torch.bfloat16)):
        return self._conv_forward(x, self.weight, self.bias)
    B, C, Hh, Ww = x.shape
    gh, gw = Hh // kh, Ww // kw
    patches = x[:, :, : gh * kh, : gw * kw].reshape(B, C, gh, kh, gw, kw).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, C * kh * kw)
    w2 = _operand(self.weight).reshape(self.out_channels, C * kh * kw)          # (trainable: autograd reshapes the [out, C kh kw] gradient to 4-D)
    y = LinearFn.apply(patches, w2, _operand(self.bias))
    return y.view(B, gh, gw, self.out_channels).permute(0, 3, 1, 2)


FUSE_MLP = True           # module attribute (no environment knob): False = three GEMMs + the element-wise rule kernel, for A/B measurements


def _fused_mlp_weights(mlp):
    """-> (Wgu interleaved [2 I, H], Wd [H, I]) of an ADOPTED bf16 gated MLP, built once and kept on the module (rebuilt when a weight is replaced
    or written): the fused-epilogue GEMMs want gate and up as one operand with its rows in blocks of [32 gate | 32 up] (ops.interleave_gate_up),
    and the long-K down weight with a row pitch that is no multiple of 4 KiB (engine.fused_layout).  Memory: the interleaved gate/up
    operand is a second copy of those two weights (Llama-3-8B: 7.5 GB; their row order cannot be expressed as a view); the pitch-padded down
    weight REPLACES the module's own storage (down_proj.weight.data becomes the padded view: no second copy).  The copy is only made while it
    leaves at least half of the device's currently free memory free -- a model that just fits keeps running, on the three-GEMM path --, and
    release_fused(model) drops it.  None where the fused kernels do not apply (fp32, biases, I % 32, trainable or foreign modules)."""
    from .. import ops
    from ..engine import fused_layout
    g, u, dn = mlp.gate_proj, mlp.up_proj, mlp.down_proj
    if not (FUSE_MLP and all(isinstance(t, torch.nn.Linear) and _owned(t) and t.bias is None and not t.weight.requires_grad for t in (g, u, dn))):
        return None
    wg, wu, wd = g.weight, u.weight, dn.weight
    if not (wg.is_cuda and wg.dtype == torch.bfloat16 and wu.dtype == wd.dtype == wg.dtype and wg.shape == wu.shape and wg.shape[0] % ops.GATED_IL == 0
            and wd.shape == (wg.shape[1], wg.shape[0])):
        return None
    key = tuple((t.data_ptr(), t._version) for t in (wg, wu, wd))
    hit = mlp.__dict__.get("_lrp_fused_mlp")
    if hit is not None and hit[0] == key:
        return hit[1], hit[2]
    if hit is None and mlp.__dict__.get("_lrp_fused_mlp_refused"):
        return None
    with torch.no_grad():
        pt = fused_layout(wg.shape[1], wg.shape[0], 0, 0, 0, wg.dtype)                  # (the MLP's pitches)
        wpad, pad = pt["Wgu"] - wg.shape[1], pt["Wd"] - wd.shape[1]
        need = 2 * wg.shape[0] * (wg.shape[1] + wpad) * wg.element_size() + (wd.shape[0] * (wd.shape[1] + pad) * wd.element_size() if pad else 0)
        if hit is None and need > torch.cuda.mem_get_info(wg.device)[0] // 2:
            mlp.__dict__["_lrp_fused_mlp_refused"] = True                              # (decided once per module: no per-call memory query)
            return None
        Wgu = ops.interleave_gate_up(wg.detach(), wu.detach(),
                                     out=torch.empty(2 * wg.shape[0], wg.shape[1] + wpad, device=wg.device, dtype=wg.dtype)[:, : wg.shape[1]])
        Wd = wd.detach()
        if pad and wd.stride(0) != wd.shape[1] + pad:
            buf = torch.empty(wd.shape[0], wd.shape[1] + pad, device=wd.device, dtype=wd.dtype)
            Wd = buf[:, : wd.shape[1]]
            Wd.copy_(wd)
            dn.weight.data = Wd                       # the module keeps ONE down weight: the padded one (a strided view; F.linear and state_dict take it)
            key = tuple((t.data_ptr(), t._version) for t in (wg, wu, dn.weight))
    mlp.__dict__["_lrp_fused_mlp"] = (key, Wgu, Wd)
    return Wgu, Wd


def release_fused(model):
    """drop what the drop-in path cached on the modules of `model` (the folded / interleaved operands of _fused_layer_weights and
    _fused_mlp_weights; down_proj weights go back to contiguous storage) -- the reference has no un-patch; this only returns the extra memory"""
    for m in model.modules():
        d = m.__dict__
        d.pop("_lrp_fused_layer_refused", None)
        if (d.pop("_lrp_fused_mlp", None) is not None) | (d.pop("_lrp_fused_layer", None) is not None):
            m = getattr(m, "mlp", m)
            dn = getattr(m, "down_proj", None)
            if dn is not None and not dn.weight.is_contiguous():
                dn.weight.data = dn.weight.data.contiguous()
        d.pop("_lrp_fused_mlp_refused", None)


def gated_mlp_forward(self, x):
    """identity rule on the activation, uniform rule on the product (ref: patches.py:145-157).  Adopted bf16 models: the whole MLP on the
    fused-epilogue GEMMs (FusedGatedMLPFn: 4 launches per layer and direction instead of 3 GEMMs + the rule kernel, bit-identical rule
    arithmetic -- tests/test_kernels_gpu.py::test_gemm_gated_fused_epilogues)"""
    act = _act_name(self.act_fn)
    if act is None:      # unknown activation: compose from the primitives
        gate = identity_rule_implicit(self.act_fn, self.gate_proj(x))
        return self.down_proj(divide_gradient(gate * self.up_proj(x), 2))
    if x.is_cuda and x.dtype == torch.bfloat16 and act in ("silu", "gelu_tanh"):
        fused = _fused_mlp_weights(self)
        if fused is not None:
            return FusedGatedMLPFn.apply(x, fused[0], fused[1], act)
    return self.down_proj(GatedActFn.apply(self.gate_proj(x), self.up_proj(x), act))


FUSE_LAYER = True         # module attribute (no environment knob): False = per-module patches only (A/B measurements, equality tests)


def _fused_layer_weights(layer):
    """-> dict(wqkv, wo, wgu, wd, meta, bqkv, qk_norm, ok, ok_rows) of an ADOPTED bf16 Llama-type decoder layer (Llama, Qwen2: bqkv = [bq; bk; bv],
    Qwen3: qk_norm = (q_norm.weight, k_norm.weight); None otherwise) for DecoderLayerFn, built once and kept on the module: the
    fused [q; k; v] weight and the interleaved gate/up weight with the layer's two RMSNorm weights FOLDED into their columns (W' = W diag(w):
    the same network and the same relevance under every rule -- lxt_amd.engine.LlamaLRP does the same; the norm is then a row scale that runs in
    the GEMM epilogues), stored-weight row pitches of engine.fused_layout.  Memory: a second copy of q/k/v and gate/up (Llama-3-8B: 10.7 GB; the
    padded down weight replaces the module's storage, o is used as stored), made only while it leaves half of the free device memory free;
    release_fused(model) drops it.  None where the fused layer cannot apply; ok_rows[(B, S)]: engine.fused_layer_ok's latest answer (cache: ok)."""
    from .. import ops
    from ..engine import fold_rows, fused_layout
    hit = layer.__dict__.get("_lrp_fused_layer")
    att, mlp = getattr(layer, "self_attn", None), getattr(layer, "mlp", None)
    lins = [getattr(att, n, None) for n in ("q_proj", "k_proj", "v_proj", "o_proj")] + [getattr(mlp, n, None) for n in ("gate_proj", "up_proj", "down_proj")]
    n1, n2 = getattr(layer, "input_layernorm", None), getattr(layer, "post_attention_layernorm", None)
    # the two dense Qwen variants: a bias on q / k / v (Qwen2; all three or none) and the per-head q_norm / k_norm of the layer's RMSNorm type
    # (Qwen3); a bias on o or the MLP, one head norm without the other, or a head norm of another kind stay on the per-module patches
    qkvb = [getattr(t, "bias", None) for t in lins[:3]]
    hn = [getattr(att, a, None) for a in ("q_norm", "k_norm")]
    if not (FUSE_LAYER and all(isinstance(t, torch.nn.Linear) and _owned(t) and not t.weight.requires_grad for t in lins)
            and all(t.bias is None for t in lins[3:]) and len({b is None for b in qkvb}) == 1 and not any(b is not None and b.requires_grad for b in qkvb)
            and n1 is not None and n2 is not None and type(n1) is type(n2) and type(n1).__name__.endswith("RMSNorm")
            and len({t is None for t in hn}) == 1 and all(t is None or (type(t) is type(n1) and not t.weight.requires_grad) for t in hn)):
        return None
    extra = [b for b in qkvb if b is not None] + [t.weight for t in hn if t is not None]
    ws = [t.weight for t in lins] + [n1.weight, n2.weight] + extra
    key = tuple((t.data_ptr(), t._version) for t in ws)
    if hit is not None and hit["key"] == key:
        return hit
    if hit is None and layer.__dict__.get("_lrp_fused_layer_refused"):
        return None
    wq, wk, wv, wo, wg, wu, wd = (t.weight for t in lins)
    cfg = att.config
    nq, nk = cfg.num_attention_heads, cfg.num_key_value_heads
    d = getattr(att, "head_dim", None) or cfg.hidden_size // nq
    H, I = wq.shape[1], wg.shape[0]
    act = _act_name(mlp.act_fn)
    eps1 = getattr(n1, "variance_epsilon", getattr(n1, "eps", None))
    eps2 = getattr(n2, "variance_epsilon", getattr(n2, "eps", None))
    ok = (wq.is_cuda and all(t.dtype == torch.bfloat16 for t in ws) and act in ("silu", "gelu_tanh") and I % ops.GATED_IL == 0 and H % 256 == 0
          and wq.shape == (nq * d, H) and wk.shape == wv.shape == (nk * d, H) and wo.shape == (H, nq * d) and wu.shape == wg.shape
          and wd.shape == (H, I) and d in (64, 128) and nq % nk == 0 and eps1 is not None and eps1 == eps2
          and float(getattr(att, "scaling", d ** -0.5)) > 0 and not getattr(att, "sliding_window", None) and not ops.attn_needs_transposed(wq, d)
          and all(t is None or (t.weight.shape == (d,) and getattr(t, "variance_epsilon", getattr(t, "eps", None)) == eps1) for t in hn))
    if not ok:
        layer.__dict__["_lrp_fused_layer_refused"] = True
        return None
    es, nqkv = wq.element_size(), (nq + 2 * nk) * d
    with torch.no_grad():
        pt = fused_layout(H, I, nq, nk, d, wq.dtype)
        copy_wd = wd.stride(0) != pt["Wd"]
        need = (nqkv * pt["Wqkv"] + 2 * I * pt["Wgu"]) * es + (H * pt["Wd"] * es if copy_wd else 0)
        if need > torch.cuda.mem_get_info(wq.device)[0] // 2:
            layer.__dict__["_lrp_fused_layer_refused"] = True                        # (decided once per layer)
            return None
        Wqkv = fold_rows(torch.empty(nqkv, pt["Wqkv"], device=wq.device, dtype=wq.dtype)[:, :H], (wq, wk, wv), n1.weight)
        tmp = fold_rows(torch.empty(2 * I, H, device=wq.device, dtype=wq.dtype), (wg, wu), n2.weight)
        Wgu = ops.interleave_gate_up(tmp[:I], tmp[I:], out=torch.empty(2 * I, pt["Wgu"], device=wq.device, dtype=wq.dtype)[:, :H])
        del tmp
        Wd = wd.detach()
        if copy_wd:
            Wd = torch.empty(H, pt["Wd"], device=wd.device, dtype=wd.dtype)[:, :I]
            Wd.copy_(wd)
            lins[6].weight.data = Wd                      # ONE down weight: the padded one (see _fused_mlp_weights)
        mlp.__dict__.pop("_lrp_fused_mlp", None)          # the MLP-level copy (if an earlier call made one) is superseded
        bqkv = torch.cat([b.detach() for b in qkvb]).contiguous() if qkvb[0] is not None else None        # [bq; bk; bv], as stored: the fold scales W only
        qk_norm = (hn[0].weight.detach().contiguous(), hn[1].weight.detach().contiguous()) if hn[0] is not None else None
    key = tuple((t.data_ptr(), t._version) for t in [t_.weight for t_ in lins] + [n1.weight, n2.weight] + extra)
    hit = dict(key=key, wqkv=Wqkv, wo=wo.detach(), wgu=Wgu, wd=Wd, meta=(nq, nk, d, float(eps1), act, float(getattr(att, "scaling", d ** -0.5))),
               bqkv=bqkv, qk_norm=qk_norm, ok={}, ok_rows={})
    layer.__dict__["_lrp_fused_layer"] = hit
    return hit


_LAYER_TABLES = {}


def _layer_rope_table(cos, sin, S, d):
    """HF's cos / sin [1, S, d] (model dtype) -> fp32 [S, d] tables for the kernels that index them by position, cached by tensor identity"""
    key = (cos.data_ptr(), sin.data_ptr(), tuple(cos.shape), cos.dtype, cos._version)
    hit = _LAYER_TABLES.get(key)
    if hit is None:
        if len(_LAYER_TABLES) >= 2:
            _LAYER_TABLES.pop(next(iter(_LAYER_TABLES)))
        hit = _LAYER_TABLES[key] = (cos.detach()[0].float().contiguous(), sin.detach()[0].float().contiguous(), cos, sin)
    return hit[0], hit[1]


def decoder_layer_forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                          position_embeddings=None, **kwargs):
    """HF LlamaDecoderLayer.forward for an adopted bf16 model at M = B S rows: the whole layer as ONE autograd node on the fused launch sequence
    of the engine (DecoderLayerFn).  Anything the fused layer does not cover -- fp32, biases, padded / packed batches, sliding windows, KV caches,
    few rows, extra keyword arguments that change the computation -- runs HF's own forward over the per-module patches, as before."""
    from .. import ops
    from ..engine import fused_layer_ok
    h = hidden_states
    fw = None
    if (FUSE_LAYER and torch.is_tensor(h) and h.is_cuda and h.dtype == torch.bfloat16 and h.dim() == 3 and past_key_values is None
            and position_embeddings is not None and not kwargs.get("output_attentions")):
        fw = _fused_layer_weights(self)
    if fw is not None:
        B, S, H = h.shape
        cos, sin = position_embeddings
        d, eps = fw["meta"][2], fw["meta"][3]
        ok = fw["ok_rows"][(B, S)] = fused_layer_ok(B * S, fw, fw["meta"], h.dtype, fw["ok"]).full     # (the engine's eligibility)
        if ok and cos.dim() == 3 and cos.shape[0] == 1 and cos.shape[1] == S and cos.shape[2] == d and not cos.requires_grad:
            causal, window, row_iv = _mask_plan(attention_mask, S, self.self_attn, 0)
            if causal and not window and row_iv is None:
                ct, st = _layer_rope_table(cos, sin, S, d)
                rstd = getattr(h, "_lrp_rstd", None)              # (rstd, eps, tensor version when it was formed)
                if rstd is None or rstd[1] != eps or rstd[0].shape[0] != B * S or rstd[2] != h._version:
                    ones = ops.const_rows(H, 1.0, h.device).to(h.dtype)
                    h2 = h.reshape(B * S, H)
                    _, r = ops.add_rmsnorm_fwd(h2 if h2.is_contiguous() else h2.contiguous(), None, ones, eps)
                else:
                    r = rstd[0]
                out, rstd_out = DecoderLayerFn.apply(h, r, fw, ct, st)
                out._lrp_rstd = (rstd_out, eps, out._version)     # the next layer's 1 / rms, left by this layer's down-projection epilogue
                return out
    return self.original_forward(hidden_states, attention_mask=attention_mask, position_ids=position_ids, past_key_values=past_key_values,
                                 use_cache=use_cache, position_embeddings=position_embeddings, **kwargs)


_ROPE_TABLES = {}


def _rope_tables(cos, sin, B, S, d):
    """HF's cos / sin [1 or B, S, d] (model dtype) -> fp32 [B*S, d] contiguous, cached by tensor identity (one pair per forward, shared by all
    layers; the entry keeps the source alive, at most two are held)"""
    key = (cos.data_ptr(), sin.data_ptr(), tuple(cos.shape), cos.dtype, cos._version, B)
    hit = _ROPE_TABLES.get(key)
    if hit is not None:
        return hit[0], hit[1]
    c, s_ = (t.detach().expand(B, S, d).reshape(B * S, d).float().contiguous() for t in (cos, sin))
    if len(_ROPE_TABLES) >= 2:
        _ROPE_TABLES.pop(next(iter(_ROPE_TABLES)))
    _ROPE_TABLES[key] = (c, s_, cos, sin)
    return c, s_


def _make_rotary(original):
    def apply_rotary_pos_emb(q, k, cos, sin, *args, unsqueeze_dim=1, **kwargs):
        """HF's RoPE on the HIP row kernels for the layout its decoder layers use (q / k [B, H, S, d] transposed views, cos / sin [B, S, d]);
        anything else runs HF's own function.  Un-patched semantics (the reference leaves RoPE alone): plain gradient."""
        ok = (not args and not kwargs and unsqueeze_dim == 1 and q.is_cuda and q.dim() == 4 and k.dim() == 4 and cos.dim() == 3
              and q.dtype in (torch.float32, torch.bfloat16) and k.dtype == q.dtype and cos.shape[-1] == q.shape[-1] == k.shape[-1]
              and q.shape[-1] % 2 == 0 and cos.shape[1] == q.shape[2] == k.shape[2] and cos.shape[0] in (1, q.shape[0])
              and not cos.requires_grad and not sin.requires_grad)
        if not ok:
            return original(q, k, cos, sin, *args, unsqueeze_dim=unsqueeze_dim, **kwargs)
        B, _, S, d = q.shape
        c, s_ = _rope_tables(cos, sin, B, S, d)
        return RopeFn.apply(q, c, s_), RopeFn.apply(k, c, s_)
    apply_rotary_pos_emb.__wrapped__ = original
    return apply_rotary_pos_emb


def patch_rotary(module):
    """replace the modeling module's apply_rotary_pos_emb (a module-level function its attention forwards look up at call time); the original
    stays reachable as .__wrapped__ and unpatch_rotary(module) puts it back"""
    orig = getattr(module, "apply_rotary_pos_emb", None)
    if orig is None:
        return False
    if getattr(orig, "__module__", None) == __name__:
        return False
    module.apply_rotary_pos_emb = _make_rotary(orig)
    return True


def unpatch_rotary(module):
    cur = getattr(module, "apply_rotary_pos_emb", None)
    if cur is not None and getattr(cur, "__module__", None) == __name__ and hasattr(cur, "__wrapped__"):
        module.apply_rotary_pos_emb = cur.__wrapped__
        return True
    return False


def mlp_forward(self, x):
    """identity rule on the activation of a plain 2-layer MLP (ref: patches.py:160-168)"""
    return self.down_proj(identity_rule_implicit(self.act_fn, self.up_proj(x)))


def non_linear_forward(self, x):
    """ref: patches.py:206-211"""
    return identity_rule_implicit(self.original_forward, x)


def dropout_forward(self, x):
    """Dropout is the identity while explaining (ref: patches.py:214-220)"""
    return x


_MASK_VERDICTS = {}


def _mask_plan(attention_mask, q_len, module, window=0):
    """-> (causal, window, row_iv): how the fused attention kernel realises HF's mask.

    HF hands either None (sdpa/flash decide by is_causal) or an additive / boolean 4-D mask [B,1,S,S].  Every mask HF
    builds for the supported families gives each query row ONE contiguous run of visible keys: causal, sliding-window
    causal, left/right padding, packed sequences, Gemma-3's bidirectional image blocks.  The mask is therefore reduced
    ONCE per tensor to per-row intervals [lo, hi) (one pass + one host sync, cached by tensor identity so it is not
    repeated per layer; the entry keeps the mask alive, at most four are held); the pure patterns go to the kernels' structural fast path (no interval arrays), everything
    else passes the int32 interval arrays.  A row whose visible keys are NOT contiguous is refused loudly."""
    if attention_mask is None:
        causal = bool(getattr(module, "is_causal", False)) and q_len > 1
        return causal, (int(window) if causal else 0), None
    m = attention_mask
    # the cache entry HOLDS the mask tensor: its memory cannot be recycled for a different mask while the key is live
    key = (m.data_ptr(), tuple(m.shape), tuple(m.stride()), m.dtype, m._version, int(window))
    hit = _MASK_VERDICTS.get(key)
    if hit is not None:
        return hit[0]
    if m.dim() != 4 or m.shape[1] != 1 or m.shape[-2] != m.shape[-1]:
        raise NotImplementedError(f"lxt_amd attention: unsupported attention_mask shape {tuple(m.shape)}")
    vis = (m if m.dtype == torch.bool else (m == 0))[:, 0]              # [B, S, S]
    B, S, _ = vis.shape
    i = torch.arange(S, device=m.device)
    cnt = vis.sum(-1, dtype=torch.int32)
    lo = torch.where(cnt > 0, vis.to(torch.int8).argmax(-1).to(torch.int32), torch.zeros_like(cnt))
    hi = lo + cnt
    j = i[None, None, :]
    contiguous = (vis == ((j >= lo[..., None]) & (j < hi[..., None]))).all()
    live = cnt > 0                                                       # rows with an empty interval constrain nothing
    w_lo = (i - window + 1).clamp_min(0).to(torch.int32)[None] if window > 0 else torch.zeros(1, S, dtype=torch.int32, device=m.device)
    causal_bounded = ((hi <= (i + 1)[None]) | ~live).all()
    window_bounded = ((lo >= w_lo) | ~live).all() if window > 0 else contiguous
    pure_causal = ((hi == (i + 1)[None]) & (lo == w_lo)).all()
    pure_full = ((lo == 0) & (hi == S)).all()
    flags = torch.stack([contiguous, causal_bounded, window_bounded, pure_causal, pure_full]).tolist()   # the one host sync
    if not flags[0]:
        raise NotImplementedError("lxt_amd attention: a query row of this attention_mask sees a non-contiguous set of keys; "
                                  "supported: causal / sliding-window / padding / packed / block-bidirectional masks")
    if flags[3]:
        plan = (True, int(window), None)
    elif flags[4] and not window:
        plan = (False, 0, None)
    else:
        plan = (bool(flags[1]), int(window) if (window > 0 and flags[2]) else 0, (lo.contiguous(), hi.contiguous()))
    if len(_MASK_VERDICTS) >= 4:
        _MASK_VERDICTS.pop(next(iter(_MASK_VERDICTS)))      # oldest first: a forward uses at most two masks (global / sliding)
    _MASK_VERDICTS[key] = (plan, m)
    return plan


def _make_attention_forward(cp):
    def attention_forward(module, query, key, value, attention_mask=None, scaling=None, dropout=0.0, **kwargs):
        # HF contract: query [B,Hq,S,d], key/value [B,Hkv,S,d] -> (attn_output [B,S,Hq,d], None)
        _need_cuda(query, "attention_forward")
        B, Hq, S, d = query.shape
        if key.shape[2] != S:
            raise NotImplementedError("lxt_amd attention: kv cache / cross attention is outside the explained path")
        window = int(kwargs.get("sliding_window") or 0)
        if window >= S:
            window = 0
        causal, window, row_iv = _mask_plan(attention_mask, S, module, window)
        if kwargs.get("softcap"):
            raise NotImplementedError("attention logit soft-capping is not supported")
        scale = float(scaling) if scaling is not None else d ** -0.5
        out = AttentionFn.apply(query.transpose(1, 2), key.transpose(1, 2), value.transpose(1, 2), scale,
                                causal, window, cp, row_iv)
        return out, None
    return attention_forward


def wrap_attention_forward(forward_fn):
    """kept for API compatibility (ref: patches.py:193-203): the returned callable ignores forward_fn
    and runs the fused HIP attention whose backward already contains the 1/4, 1/4, 1/2 factors."""
    return _make_attention_forward(cp=False)


def cp_wrap_attention_forward(forward_fn):
    return _make_attention_forward(cp=True)


def _patch_attention(module, cp):
    patch_ownership(module)
    patch_rotary(module)
    new_forward = _make_attention_forward(cp)
    if hasattr(module, "eager_attention_forward"):
        if check_already_patched(module.eager_attention_forward, new_forward):
            return False
        module.eager_attention_forward = new_forward
    registry = getattr(module, "ALL_ATTENTION_FUNCTIONS", None)
    if registry is not None:
        for key, value in list(registry.items()):
            if check_already_patched(value, new_forward):
                return False
            # HF's OWN attention functions (eager / sdpa / flash / flex ...) are replaced by the HIP kernel; an entry somebody else registered
            # under a name of their own (a user's custom attention, the tests' CPU oracle) is not ours to take over -- the registry is one
            # process-wide object, and overriding it would reroute every other model that selects that name
            if not str(getattr(value, "__module__", "")).startswith("transformers"):
                continue
            registry[key] = new_forward
    return True


def patch_attention(module):
    """replace eager_attention_forward and every entry of HF's process-wide attention registry
    (ref: patches.py:171-190 wraps them; here they are replaced by the HIP kernel)"""
    return _patch_attention(module, cp=False)


# ------------------------------------------------------------------------------------- CP-LRP patches
def patch_cp_attention(module):
    """CP-LRP: no relevance through softmax, i.e. q and k detached (ref: patches.py:228-255)"""
    return _patch_attention(module, cp=True)


def cp_multi_head_attention_forward(self, query, key, value, key_padding_mask=None, need_weights=True, attn_mask=None,
                                    average_attn_weights=True, is_causal=False):
    """CP-LRP for torch.nn.MultiheadAttention: query and key carry no relevance (ref: patches.py:258-266, which calls the
    original forward on detached q/k).  The case vision transformers use -- self-attention without masks, weights not
    requested -- runs entirely on liblrp_hip.so: three projection GEMMs, the fused attention kernel with its CP backward
    (only dV), the output GEMM.  Everything else takes the reference's route through the original forward."""
    fast = (query.is_cuda and not need_weights and key_padding_mask is None and attn_mask is None and not is_causal
            and self._qkv_same_embed_dim and self.bias_k is None and self.bias_v is None and not self.add_zero_attn
            and query.dim() == 3 and query.dtype in (torch.float32, torch.bfloat16))
    if not fast:
        return self.original_forward(stop_gradient(query), stop_gradient(key), value, key_padding_mask=key_padding_mask,
                                     need_weights=need_weights, attn_mask=attn_mask, average_attn_weights=average_attn_weights,
                                     is_causal=is_causal)
    from .. import ops
    if not self.batch_first:
        query, key, value = query.transpose(0, 1), key.transpose(0, 1), value.transpose(0, 1)
    B, Sq, E = query.shape
    H, d = self.num_heads, self.head_dim
    w, b = self.in_proj_weight.detach(), (self.in_proj_bias.detach() if self.in_proj_bias is not None else None)
    bq, bk, bv = (b[:E], b[E: 2 * E], b[2 * E:]) if b is not None else (None, None, None)
    with torch.no_grad():
        q = ops.gemm_nt(query.detach().reshape(B * Sq, E).contiguous(), w[:E], bq).view(B, Sq, H, d)
        k = ops.gemm_nt(key.detach().reshape(-1, E).contiguous(), w[E: 2 * E], bk).view(B, -1, H, d)
    wv = w[2 * E:]
    v = LinearFn.apply(value, wv, bv).view(B, -1, H, d)
    if k.shape[1] != Sq:
        raise NotImplementedError("lxt_amd MultiheadAttention fast path: cross attention with a different key length")
    o = AttentionFn.apply(q, k, v, d ** -0.5, False, 0, True, None)            # cp=True: dQ = dK = 0, all relevance on V
    op_, ow = self.out_proj, self.out_proj.weight.detach()
    out = LinearFn.apply(o.reshape(B, Sq, E), ow, op_.bias.detach() if op_.bias is not None else None)
    if not self.batch_first:
        out = out.transpose(0, 1)
    return out, None


def cp_gated_mlp_forward(self, x):
    """CP-LRP: the gate is detached, everything flows through up_proj (ref: patches.py:269-280)"""
    gate = self.act_fn(stop_gradient(self.gate_proj(x)))
    return self.down_proj(gate * self.up_proj(x))
