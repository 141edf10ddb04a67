/* lrp_hip_moe_wgrad.h -- part of the C ABI of liblrp_hip.so (version 8): the per-weight relevance of the ROUTED EXPERTS of a sparse MoE layer,
 * the grouped form of lrp_hip_wgrad.h (csrc/moe_wgrad.hip).  Included by lrp_hip.h (include that one); error codes, dtype codes and the
 * routing plan (lrp_moe_plan) are lrp_hip.h's, the MXFP4 layout of an expert tensor is lrp_hip_moe_mxfp4.h's. */
#ifndef LRP_HIP_MOE_WGRAD_H
#define LRP_HIP_MOE_WGRAD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LRP_MOE_WGRAD_GATE_UP 0
#define LRP_MOE_WGRAD_DOWN 1

/* lrp_moe_wgrad_rel:  out[e][n, k]  (+)=  W[e][n, k] * sum_{p in e} s(p) G[gp(p), n] X[xp(p), k]      for e < E, n < N, k < K
 * -- `weight * weight.grad` of an expert tensor [E, N, K] (ref: under lxt.efficient.monkey_patch, lxt/efficient/models/qwen3_moe.py:14-44,
 * experts.gate_up_proj [E, 2 I, H] and experts.down_proj [E, H, I] are plain parameters of plain matmuls: logit.backward() leaves their
 * .grad, and the relevance of a weight is weight * weight.grad).  p runs over the plan rows of expert e, off[e] <= p < off[e + 1], in plan
 * order (token order: the plan is stable); perm[p] = t k + slot.  T tokens, k slots, R = T k.
 *   mode LRP_MOE_WGRAD_GATE_UP: G [R, N] in PLAN rows (what lrp_moe_down_dgrad writes: Agu, N = 2 I in [gate | up] order), X [T, K] gathered
 *     by token (the expert's input x2, K = H), s = 1; w is not read (NULL is fine).
 *   mode LRP_MOE_WGRAD_DOWN: G [T, N] gathered by token (the gradient at the block's output, N = H), X [R, K] in plan rows (the stored m,
 *     K = I), s(p) = 1/2 w[perm[p]]: the routing weight, and the 1/2 of divide_gradient(., 2) on the weighted expert output; w [T, k]
 *     contiguous, in the activation dtype.
 *   G (row pitch ldg), X (ldx): unit column stride; both and w LRP_F32 or LRP_BF16.  W [E, N, K] contiguous, in the activation dtype.
 *   out [E, N, K] fp32, contiguous.  accumulate: 0 -> out = ..., else out += ... (read-modify-write by the element's one owner thread).
 *   An expert WITHOUT rows: accumulate = 0 -> its block is written as exact zeros (whatever out and W hold); accumulate != 0 -> its block
 *     is neither read nor written.
 *   LRP_BF16: a 128 x 128 tile of one expert per workgroup, the expert's rows in tiles of 64, both MFMA operands transposed LDS reads,
 *     v_mfma_f32_16x16x32_bf16 with fp32 accumulation over all rows of the expert in one accumulator, plan order; rows past the expert's
 *     count are staged as zeros.  s is folded into G while staging, G' = bf16(float(G) s): in the DOWN mode G takes one extra bf16
 *     rounding (at most 2^-8 relative, bf16's unit roundoff; 1/2 w itself is exact), X and W are used as stored; W acc is an fp32 product.  N and K multiples of 8.
 *   LRP_F32 (the parity path): s G X formed exactly and summed in fp64, W acc rounded once to fp32.  Any N, K >= 1 on the pitch rule below.
 *   lrp_moe_wgrad_rel_q: W as MXFP4 codes [E, N, K / 2] + scales [E, N, K / 32] (lrp_hip_moe_mxfp4.h), decoded in the epilogue (one scale
 *     byte and two code bytes per 4 outputs); K a multiple of 128.  Every decoded value is exact in bf16 and fp32: the result is
 *     BIT-IDENTICAL to lrp_moe_wgrad_rel on lrp_mxfp4_dequant's tensor.  No dequantised copy exists.
 *   lrp_moe_wgrad_rel_ok(..., quantised) -> 1 when the entry (quantised != 0: the _q entry) serves the problem, else the code the entry
 *     would return for it:  an unknown dtype or mode -> LRP_EINVAL;  T / k / E / N / K < 1, E > 1024, T k >= 2^30, ldg < N, ldx < K, more than
 *     65535 row tiles (128 rows in bf16, 64 in fp32), LRP_BF16 with N or K off the grid of 8, quantised with K off the grid of 128
 *     -> LRP_ESHAPE;  a row pitch of G or X that is no multiple of 16 bytes -> LRP_EALIGN.
 *   The entries add (first): NULL G / X / W (codes, scales) / plan / out, NULL w in the DOWN mode -> LRP_EINVAL;  (last): G / X / W (codes) /
 *     out off 16 bytes, plan / scales off 4 bytes, w off its element size -> LRP_EALIGN.  All of it before any launch.
 *   One launch, no host sync, no workspace, no atomics; cnt / off / perm are read on the device; every result element has one owner thread
 *   that sums the expert's rows in plan order: bitwise repeatable.  The caller guarantees a plan of lrp_moe_plan for (T, k, E). */
int lrp_moe_wgrad_rel_ok(int T, int k, int E, int N, int K, int64_t ldg, int64_t ldx, int mode, int dtype, int quantised);
int lrp_moe_wgrad_rel(const void* G, const void* X, const void* W, const void* w, const int* plan, float* out, int T, int k, int E, int N, int K,
                      int64_t ldg, int64_t ldx, int mode, int accumulate, int dtype, void* stream);
int lrp_moe_wgrad_rel_q(const void* G, const void* X, const void* codes, const void* scales, const void* w, const int* plan, float* out, int T,
                        int k, int E, int N, int K, int64_t ldg, int64_t ldx, int mode, int accumulate, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRP_HIP_MOE_WGRAD_H */
