/* lrp_hip_latent.h -- part of the C ABI of liblrp_hip.so (version 8): the per-head and token-to-token read-outs of the latent feature attribution.
 * Included by lrp_hip.h (include that one); error codes, dtype codes and conventions are lrp_hip.h's. */
#ifndef LRP_HIP_LATENT_H
#define LRP_HIP_LATENT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* lrp_headdot (csrc/latent.hip): out[b, h, t] = scale sum_{j < d} x[b S + t, (h / rep) d + j] g'[b S + t, h d + j] for b < B, h < nh, t < S,
 * fp32 [B, nh, S] contiguous (the layout of the attention kernels' lse and D) -- the relevance of every attention head at every position
 * (x = o, q, k or v and g its gradient per QUERY head).  ref: retain_grad() on the attention function's operands, `(x * x.grad).sum(-1)`.
 *   x: [M = B S, (nh / rep) d] with row pitch ldx: nh / rep heads (rep = 1 for q and o, rep = nq / nk for k and v: GQA, query head h reads
 *   kv head h / rep); g: [M, nh d] with row pitch ldg; both LRP_F32 or both LRP_BF16, token-major.
 *   g' = g when cos == sin == NULL; else the forward rotate-half RoPE of g at position t, cos / sin fp32 [>= S, d] with row pitch d:
 *     g'[j] = g[j] cos[t, j] - g[j + d/2] sin[t, j] (j < d/2),  g'[j] = g[j] cos[t, j] + g[j - d/2] sin[t, j] (j >= d/2).
 *   (The fused dQ kernel stores RoPE^T(dq) and only the rotated q is kept; sum_d q dq = sum_d q_rot RoPE(dq_unrot), so the read-out needs no
 *   second copy of q.  Tables that carry an attention_scaling s != 1 apply it twice, once in RoPE^T and once here: pass scale = 1 / s^2.)
 *   NULL x / g / out, an unknown dtype, one of cos / sin without the other -> LRP_EINVAL.  B S != M, nh / rep / d < 1, nh % rep != 0,
 *   d > 256, an odd d with tables, B or ceil(S / 16) > 65535, ldx < (nh / rep) d, ldg < nh d -> LRP_ESHAPE.  x / g / cos / sin bases or
 *   the pitches off the 16-byte grid, d * sizeof(T) not a multiple of 16, out off 4 bytes -> LRP_EALIGN.  All of it before any launch.
 *   One launch, no workspace, no atomics, plain vector stores.  Bitwise deterministic and batch invariant: a (row, head) sum is formed by a
 *   fixed lane group (elements in order inside a lane, lanes by an xor butterfly); a workgroup owns 16 consecutive rows of ONE prompt, counted
 *   from the prompt's first row, and transposes its sums through LDS into runs along t. */
int lrp_headdot(const void* x, const void* g, const float* cos, const float* sin, float* out, int M, int B, int S, int nh, int rep, int d,
                int64_t ldx, int64_t ldg, float scale, int dtype, void* stream);

/* lrp_attn_relmap (csrc/attnmap.hip): out[b, i, j] = gscale sum_{h_lo <= h < h_hi} P_h[i, j] (g[b S + i, h d :] . v[b S + j, (h / rep) d :]) with
 * P_h[i, j] = exp(scale q[b S + i, h d :] . k[b S + j, (h / rep) d :] - lse[b, h, i]), rep = Hq / Hkv, for every (i, j) the mask lets through
 * (causal: j <= i; row_lo / row_hi: row_lo[b S + i] <= j < row_hi[b S + i], as the attention entries of lrp_hip.h read them) and exactly 0
 * elsewhere; fp32 [B, S, S] contiguous, EVERY element written (callers pass uninitialised memory) -- the token-to-token attention relevance
 * `attn_weights * attn_weights.grad` of eager attention, summed over a range of query heads, recomputed per tile from what the flash-style
 * kernels keep.  ref: retain_grad() on the probabilities inside HF's eager_attention_forward, which lxt/efficient/patches.py:193-203 wraps
 * (divide_gradient sits on query / key / value, not on the probabilities: no 1/2 in the map).
 *   q, g: [M = B S, Hq d] (row pitches ldq, ldg), k, v: [M, Hkv d] (ldk, ldv), token-major, consumed in place from the fused QKV output:
 *   q / k as the attention kernels read them (rotated, after Qwen3's head norm); g = the gradient at the o projection's input, or the
 *   dgrad epilogue's Gho = 1/2 of it with gscale = 2.  All four LRP_F32 or all four LRP_BF16.  lse fp32 [B, Hq, S] as lrp_attn_fwd writes
 *   it: the natural-log sum-exp of the SCALED scores, -inf for a row with an empty interval (such a row gives exactly 0, never NaN).
 *   LRP_BF16: d in {64, 128}, both contractions on the bf16 MFMA, fp32 from the accumulators to the store (P and G_P are never rounded).
 *   LRP_F32: any d <= 256 that is a multiple of 4, LDS-tiled FMA (the parity path).
 *   NULL q / k / v / g / lse / out, an unknown dtype -> LRP_EINVAL.  B S != M, B / S / Hq / Hkv / d < 1, Hq % Hkv != 0, a head range that is
 *   empty or not inside [0, Hq), a d the dtype is not served at, ldq / ldg < Hq d, ldk / ldv < Hkv d, one of row_lo / row_hi without the
 *   other, B > 65535 -> LRP_ESHAPE.  q / k / v / g bases or pitches off the 16-byte grid, out / lse / row_lo / row_hi off 4 bytes
 *   -> LRP_EALIGN.  All of it before any launch.
 *   One launch, no "_t" operands, no workspace, no atomics.  A workgroup owns one 64 x 64 tile of one prompt's map, counted from the prompt's
 *   first row, walks the heads in ascending order with the tile in fp32 registers and stores it once: bitwise deterministic and batch
 *   invariant.  A tile no row of it can see (above the diagonal, outside the union of its rows' intervals) is zero-filled without a load. */
int lrp_attn_relmap(const void* q, const void* k, const void* v, const void* g, const float* lse, float* out, int M, int B, int S, int Hq,
                    int Hkv, int d, int h_lo, int h_hi, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldg, float scale, float gscale,
                    int causal, const int* row_lo, const int* row_hi, int dtype, void* stream);

/* lrp_attn_relmap_d256 (csrc/attnmap.hip): lrp_attn_relmap for LRP_BF16 at d == 256 (Gemma-3's head dim) -- the same arguments in the same
 * order, the same out[b, i, j], masks, lse convention, error ladder and guarantees (every element written, masked (i, j) selected to exactly
 * 0, a row with lse = -inf gives 0, dead tiles zero-filled without a load, one launch, no workspace, no atomics, bitwise deterministic and
 * batch invariant); any other dtype or d -> LRP_ESHAPE (an unknown dtype -> LRP_EINVAL).  Both contractions on the bf16 MFMA, fp32 from the
 * accumulators to the store.  K and V are staged in two panels of 128 columns (LDS: 34 KB per workgroup in place of 84 KB); the score and
 * G_P accumulators of the query heads that share the staged kv head live across the two panels, so one staging serves all rep heads of a
 * group for rep <= 4 (a wider group is walked in chunks of 4 heads); the MFMA steps of a head still run in the order of d. */
int lrp_attn_relmap_d256(const void* q, const void* k, const void* v, const void* g, const float* lse, float* out, int M, int B, int S, int Hq,
                         int Hkv, int d, int h_lo, int h_hi, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldg, float scale, float gscale,
                         int causal, const int* row_lo, const int* row_hi, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRP_HIP_LATENT_H */
