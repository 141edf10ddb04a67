/* lrp_hip_moe_router.h -- part of the C ABI of liblrp_hip.so (version 8): the top-k router of a sparse MoE layer on the device and the
 * per-expert relevance read-out (csrc/moe_router.hip).  Included by lrp_hip.h (include that one); error codes, dtype codes and conventions
 * are lrp_hip.h's.  ref: transformers' Qwen3MoeTopKRouter.forward, which lxt/efficient/models/qwen3_moe.py leaves unpatched (plain autograd).
 * Common to the three: one dtype code (LRP_F32 or LRP_BF16) for every activation operand; idx is int64 [T, k] contiguous, what lrp_moe_plan
 * reads; 1 <= k <= 16, k <= E <= 1024, T k < 2^30, else LRP_ESHAPE; a NULL operand, T / E / k < 1 or an unknown dtype -> LRP_EINVAL; all
 * checks run before any launch.  One launch each, no workspace, no atomics, plain vector loads and stores; every output element is written
 * (callers pass uninitialised memory); bitwise repeatable, and a token's (a prompt's) result depends on its own rows only. */
#ifndef LRP_HIP_MOE_ROUTER_H
#define LRP_HIP_MOE_ROUTER_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* lrp_moe_router_fwd: per token row t, in HF's order: p = softmax over E of logits[t, :] in fp32 (exp(x - max) / sum, the logits as stored);
 * the k largest p (ties go to the LOWER expert index, slots in descending p); norm_topk != 0: division by their fp32 sum (added in slot
 * order); ONE rounding to the activation dtype.
 *   logits [T, E] with row pitch ldl (elements; ldl < E -> LRP_ESHAPE; a row that does not start on the 4-byte grid -- the base, or an odd bf16
 *   pitch -- -> LRP_EALIGN: rows are read element by element, 60 experts in bf16 are fine);
 *   idx int64 [T, k], w [T, k] (activation dtype), lse fp32 [T] = log sum_e exp(logits[t, e]), for the backward.
 * One wave64 per row, lane l holds experts l, l + 64, ...; the arg-max is k rounds of an xor butterfly on the (value, index) pair. */
int lrp_moe_router_fwd(const void* logits, void* idx, void* w, float* lse, int T, int E, int k, int64_t ldl, int norm_topk, int dtype,
                       void* stream);

/* lrp_moe_router_bwd: the exact backward of the forward above.  p[e] = exp(logits[t, e] - lse[t]), i_s = idx[t, s], G_w [T, k] (activation
 * dtype, as lrp_moe_gw_reduce writes it):
 *   norm_topk: V = sum_s p[i_s], c = sum_r G_w[r] p[i_r] / V, G_v[s] = (G_w[s] - c) / V;  else G_v = G_w;
 *   G_logits[t, e] = p[e] ([e = i_s] G_v[s] - sum_s G_v[s] p[i_s]).
 * With norm_topk the last sum is 0 analytically and is not formed: unselected experts get exactly 0.  The renorm's backward uses the fp32
 * weight p[i_r] / V that autograd holds (HF rounds to the activation dtype AFTER the division); w, the rounded copy the forward returned,
 * is checked like the other operands and not read -- in bf16 it would put 2^-9 |c| into every G_v.  A slot index outside [0, E) carries
 * nothing.  G_logits [T, E] with row pitch ldg, dense, every element of the E columns written; pitches and bases as in the forward. */
int lrp_moe_router_bwd(const void* logits, const float* lse, const void* idx, const void* w, const void* gw, void* g_logits, int T, int E,
                       int k, int64_t ldl, int64_t ldg, int norm_topk, int dtype, void* stream);

/* lrp_moe_expert_relevance: out[b, e] = sum_{t in prompt b} sum_s [idx[t, s] = e] w[t, s] G_w[t, s], fp32 [B, E] contiguous -- the relevance
 * of every expert for every prompt (T = B S token rows, prompt b owns rows b S .. b S + S - 1).  ref: `routing_weights *
 * routing_weights.grad` scattered by `selected_experts`.  A slot index outside [0, E) is skipped; an expert nobody selects gets 0.
 *   B > 65535 or B S k >= 2^30 -> LRP_ESHAPE.  Products in fp32; a workgroup owns 64 experts of one prompt and adds in a fixed order. */
int lrp_moe_expert_relevance(const void* idx, const void* w, const void* gw, float* out, int B, int S, int k, int E, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRP_HIP_MOE_ROUTER_H */
