"""Routed experts of a sparse MoE layer (HF Qwen3MoeExperts) on the grouped HIP GEMMs of csrc/moe.hip, forward and LRP backward.
ref: lxt/efficient/models/qwen3_moe.py:14-44 (experts_forward).  The reference loops over the experts that were hit (a device -> host sync
for the list, then a gather, two Linears, the rule ops and an index_add per expert); here one routing plan and four grouped GEMMs serve
every expert at once, with no host sync.  The router stays HF's own module under plain autograd, as in the reference: the relevance that
reaches the routing weights (G_w) flows on through its top-k renorm, softmax and F.linear."""
import torch
from torch.autograd import Function

from .. import ops
from .rules import _act_name

_ACTS = ("silu", "gelu_tanh")


class MoEExpertsFn(Function):
    """out[t] = sum_s w[t, s] (act(x[t] Wg[e]^T) (*) (x[t] Wu[e]^T)) Wd[e]^T over the slots s of token t (e = top_k_index[t, s]; e outside
    [0, E) skips the slot), with the reference's rules: identity rule on act (eps 1e-10), divide_gradient(., 2) on the gated product and on the
    weighted expert output, plain gradients through the Linears and the routing-weight product.  Backward, per (t, s) row:
        G_y = 1/2 w G[t],  G_m = G_y Wd[e],  G_g = 1/2 G_m u act(g) / (g + eps),  G_u = 1/2 G_m act(g),  G_x[t] += (G_g | G_u) Wgu[e],
        G_w[t, s] = 1/2 sum_j y_j G[t]_j.
    Stash per layer: the coefficients [T k, 2 I] and m [T k, I] (activation dtype) and the int32 routing plan; y is never kept."""

    @staticmethod
    def forward(ctx, hidden, top_k_index, top_k_weights, gate_up_proj, down_proj, act):
        x = hidden if hidden.is_contiguous() else hidden.contiguous()
        E = gate_up_proj.shape[0]
        plan = ops.MoePlan(top_k_index, E)
        w = top_k_weights.to(x.dtype).contiguous()
        coef, m = ops.moe_gate_up_fwd(x, gate_up_proj, plan, act)
        y = ops.moe_down_fwd(m, down_proj, plan)
        out = ops.moe_combine(y, plan, w)
        ctx.save_for_backward(gate_up_proj, down_proj, coef, m, w)
        ctx.plan, ctx.w_dtype = plan, top_k_weights.dtype
        return out

    @staticmethod
    def backward(ctx, G):
        Wgu, Wd, coef, m, w = ctx.saved_tensors
        plan = ctx.plan
        G = G.to(m.dtype)
        G = G if G.is_contiguous() else G.contiguous()
        Agu, gw = ops.moe_down_dgrad(G, Wd, coef, m, w, plan)
        gx = ops.moe_combine(ops.moe_gate_up_dgrad(Agu, Wgu, plan), plan)
        return gx, None, gw.to(ctx.w_dtype), None, None, None


def experts_forward(self, hidden_states, top_k_index, top_k_weights):
    """drop-in forward of Qwen3MoeExperts (replaces HF's @use_experts_implementation dispatcher, as the reference's patch does)"""
    if not hidden_states.is_cuda:
        raise RuntimeError("experts_forward: lxt_amd runs on the HIP device only (no CPU fallback); got a CPU tensor")
    act = _act_name(self.act_fn)
    if act not in _ACTS:
        raise NotImplementedError(f"lxt_amd MoE experts: activation {type(self.act_fn).__name__} is not served (the grouped kernels "
                                  f"implement {', '.join(_ACTS)})")
    Wgu, Wd = self.gate_up_proj, self.down_proj
    E, I2, H = Wgu.shape
    if H % 128 or (I2 // 2) % 128:
        raise NotImplementedError(f"lxt_amd MoE experts: hidden size {H} and moe_intermediate_size {I2 // 2} must be multiples of 128 "
                                  "(the grouped GEMMs' 128 x 128 tiles)")
    if E > 1024:
        raise NotImplementedError(f"lxt_amd MoE experts: {E} experts; the routing plan serves at most 1024")
    if hidden_states.dtype not in (torch.float32, torch.bfloat16) or Wgu.dtype != hidden_states.dtype or Wd.dtype != hidden_states.dtype:
        raise NotImplementedError(f"lxt_amd MoE experts: activations {hidden_states.dtype} with expert weights {Wgu.dtype} / {Wd.dtype}; "
                                  "float32 or bfloat16, all the same")
    if not (Wgu.is_contiguous() and Wd.is_contiguous()):
        raise NotImplementedError("lxt_amd MoE experts: gate_up_proj / down_proj must be contiguous (the kernels read them as stored; "
                                  "no copy of the expert weights is made)")
    shp = hidden_states.shape
    x = hidden_states.reshape(-1, H)
    if x.shape[0] == 0:
        return torch.zeros_like(hidden_states)
    out = MoEExpertsFn.apply(x, top_k_index.reshape(x.shape[0], -1), top_k_weights.reshape(x.shape[0], -1), Wgu, Wd, act)
    return out.view(shp)
