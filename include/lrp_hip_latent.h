/* lrp_hip_latent.h -- part of the C ABI of liblrp_hip.so (version 8): the per-head read-out of the latent feature attribution.
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

#ifdef __cplusplus
}
#endif
#endif /* LRP_HIP_LATENT_H */
