/* lrp_hip_attn_cp.h -- part of the C ABI of liblrp_hip.so (version 8): the two kernels of the CP-LRP rule (ref lxt/efficient/patches.py:228-280,
 * the `cp_LRP` composites of lxt/efficient/models/llama.py, qwen2.py, qwen3.py).  Against the AttnLRP placement q and k are detached -- the
 * attention backward is dV alone, with factor 1 -- and so is the gate of the MLP.  Included by lrp_hip.h (include that one); error codes, dtype
 * codes and conventions are lrp_hip.h's. */
#ifndef LRP_HIP_ATTN_CP_H
#define LRP_HIP_ATTN_CP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* lrp_attn_bwd_dv (csrc/attention_cp.hip): the value gradient of causal attention, summed over the GQA group,
 *     dv[b, j, hk, :] = sum_{h in group hk, ascending} sum_{i >= max(j, q_begin), j in [row_lo[b, i], row_hi[b, i]), ascending query tiles}
 *                           P_h[i, j] G[b, i, h, :],        P_h[i, j] = exp(scale q_h[i].k_hk[j] - lse[b, h, i])
 *   q [B S, Hq d] (pitch ldq) and k [B S, Hkv d] (ldk) rotated as the forward saw them, lse [B, Hq, S] fp32 from lrp_attn_fwd, G [B S, Hq d]
 *   (ldg) the gradient of the attention output (the o-projection's dgrad as it is: no lrp_attn_bwd_prep, no D), dv [B S, Hkv d] (lddv) in the
 *   operand dtype.  Causal, no window.  row_lo / row_hi [B, S] int32 or both NULL: the per-query-row key interval of lrp_attn_bwd_dkv.
 *   q_begin: query rows below it carry no gradient and are not loaded (the tile that holds q_begin is entered and masked).
 *   G_t [B, Hq, d, ldt]: the head-transposed copy of G (lrp_transpose_heads), needed where lrp_attn_needs_transposed(dtype, d) = 1 and ignored
 *   (NULL allowed) where it is 0.
 *   Served (lrp_attn_bwd_dv_ok): LRP_BF16 at d in {64, 96, 128} -- 32x32x16 MFMAs, G^T read out of the row-major tile with transpose reads, one
 *   workgroup of 8 (4) waves per (b, kv head, 256 (128) keys) -- the smaller form while the grid is below 4 workgroups per CU; the result
 *   is bitwise the same -- which walks the group's query heads in ascending order with the dV accumulators in registers; LRP_F32 at d in {16, 32, 64, 128} -- 16x16x4 MFMAs, one workgroup of 4 waves per (b, kv head, 64 keys), the same walk.
 *   No atomics, no dv_h [B S, Hq d] round trip, no lrp_gqa_reduce; the summation order is fixed (heads ascending, query tiles ascending, the
 *   MFMA's own order inside a tile), so the result is bitwise repeatable and a prompt's rows do not depend on the other prompts of the call.
 *   A key no query sees (an empty interval, a pad) gets exact zeros.
 *   NULL q / k / G / lse / dv, one of row_lo / row_hi alone, B < 0, S < 0, Hq < 1, Hkv < 1, Hq % Hkv, d < 16, scale <= 0, q_begin < 0, an
 *   unknown dtype, a missing G_t where it is needed -> LRP_EINVAL.  A (dtype, d) that is not served, B > 65535, Hq > 65535 -> LRP_ESHAPE.
 *   A base off 16 bytes, ldq / ldk / ldg / ldt off the 16-byte grid, lddv % 4, ldt < S -> LRP_EALIGN.  B == 0 or S == 0 -> LRP_OK, nothing
 *   launched.  All of it before any launch. */
int lrp_attn_bwd_dv_ok(int dtype, int d);
int lrp_attn_bwd_dv(const void* q, const void* k, const void* G, const void* G_t, const float* lse, void* dv, int B, int S, int Hq, int Hkv,
                    int d, int64_t ldq, int64_t ldk, int64_t ldg, int64_t ldt, int64_t lddv, float scale, int q_begin, const int* row_lo,
                    const int* row_hi, int dtype, void* stream);

/* lrp_gated_cp_bwd_il (csrc/eltwise.hip): CP-LRP through the gated MLP on the interleaved gate/up layout of lrp_gated_act_bwd_il (blocks of
 * LRP_GATED_IL).  From Gm [M, I] (ldgm) and the pre-activations gu [M, 2 I] (ldgu) write Agu [M, 2 I] (ldagu):
 *     up slots   : act(g) Gm      (act(g) rounded to the storage dtype, as the forward's m = act(g) u formed it)
 *     gate slots : 0 exactly      (the gate is detached)
 * 16-byte loads and stores.  NULL pointers, M < 0, I < 0, I % LRP_GATED_IL, act outside 0 .. 3, an unknown dtype -> LRP_EINVAL;
 * ldgm < I, ldgu < 2 I, ldagu < 2 I -> LRP_ESHAPE; a base or a pitch off the 16-byte grid -> LRP_EALIGN; M == 0 or I == 0 -> LRP_OK. */
int lrp_gated_cp_bwd_il(const void* Gm, const void* gu, void* Agu, int M, int I, int64_t ldgm, int64_t ldgu, int64_t ldagu, int act, int dtype,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRP_HIP_ATTN_CP_H */
