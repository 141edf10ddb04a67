/* lrp_hip_decode_site.h -- part of the C ABI of liblrp_hip.so (version 8): the site kernel of a decode step whose model norms q and k per head
 * in front of RoPE (Gemma3LRP.generate): both head norms, RoPE and the cache append in one launch.  Included by lrp_hip.h (include that
 * one); error codes, dtype codes and conventions are lrp_hip.h's, the caches and pos are lrp_hip_decode.h's. */
#ifndef LRP_HIP_DECODE_SITE_H
#define LRP_HIP_DECODE_SITE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* lrp_decode_qknorm_rope_append (csrc/decode_site.hip): per prompt b < B, with p = *pos and N_w(x) = x rsqrt(mean_d(x^2) + eps) (w + w_offset)
 * over one head of d columns, rounded once to the storage type,
 *     q_rot[b, h d + c]  = RoPE_p(N_wq(qk[b, h d : (h + 1) d]))[c]                    h < nq
 *     kc[b, p, h d + c]  = RoPE_p(N_wk(qk[b, (nq + h) d : (nq + h + 1) d]))[c]        h < nk
 *     vc[b, p, :]        = v[b, :]                                                     (a copy, bitwise)
 *   CONTRACT: for every argument set the outputs equal, bit for bit, lrp_head_rmsnorm_fwd on the q columns, lrp_head_rmsnorm_fwd on the k
 *   columns (both with eps, w_offset) and lrp_decode_rope_append on their outputs: the sum of squares in that kernel's order (a lane its 16
 *   bytes in column order, the d / (16 / sizeof(T)) lanes of a head by the xor butterfly from half the group down to 1), rstd = rsqrtf(ss / d +
 *   eps), w_offset == 0: w * T(x rstd), otherwise (x rstd) (w_offset + w) in fp32, one rounding to the storage type where the norm kernel
 *   stored; then out1 = n1 cos[c] - n2 sin[c], out2 = n2 cos[c + d/2] + n1 sin[c + d/2] in fp32 without contraction, one rounding.  No rstd is
 *   written (the step is forward only).
 *   qk [B, (nq + nk) d] (q | k, biased by the caller if the model has a bias) and v [B, nk d]: 2-D views with row pitches ldqk, ldv (the two
 *   column ranges of one projection buffer);  wq, wk [d] in the call's dtype;  cos_t / sin_t fp32 [table_rows, d];  q_rot [B, nq d], pitch ldq.
 *   p < 0, p >= cap or p >= table_rows: NOTHING is written (q_rot neither); the guard is lrp_decode_rope_append's, evaluated on the device
 *   before any address is formed from p.
 *   Head dims: those both composed kernels take -- d * sizeof(T) / 16 a power of two in 1 .. 64 and d <= 256 (fp32: 4, 8, .. 256; bf16: 8, 16,
 *   .. 256).  With d one 16-byte vector the rotate-half partner is in the lane's own vector, otherwise half a lane group away.
 *   NULL qk / v / wq / wk / cos_t / sin_t / pos / q_rot / kc / vc, B < 0, nq < 1, nk < 1, cap < 1, table_rows < 1, an unknown dtype -> LRP_EINVAL.
 *   A head dim outside the list above, ldqk < (nq + nk) d, ldv < nk d, ldq < nq d, ldc < nk d -> LRP_ESHAPE.
 *   qk / v / wq / wk / q_rot / kc / vc / cos_t / sin_t off 16 bytes, pos off 4, a pitch that is not a multiple of 16 bytes -> LRP_EALIGN.
 *   B == 0 -> LRP_OK, nothing launched.  All of it before any launch, in that precedence.
 *   One launch of one-wave workgroups, a lane group of d sizeof(T) / 16 lanes per (prompt, head) -- a head never spans more than one wave;
 *   16-byte loads and stores only, no LDS, no atomics: bitwise repeatable. */
int lrp_decode_qknorm_rope_append(const void* qk, int64_t ldqk, const void* v, int64_t ldv, const void* wq, const void* wk, float eps,
                                  float w_offset, const float* cos_t, const float* sin_t, int table_rows, const int* pos, void* q_rot,
                                  int64_t ldq, void* kc, void* vc, int64_t ldc, int B, int cap, int nq, int nk, int d, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRP_HIP_DECODE_SITE_H */
