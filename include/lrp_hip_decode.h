/* lrp_hip_decode.h -- part of the C ABI of liblrp_hip.so (version 8): the two kernels of a KV-cached decode step (LlamaLRP.generate): RoPE of
 * the new token's q / k with the append of k / v to the cache, and single-query attention over the cache.  Both take the step's column from
 * DEVICE memory, so a captured step replays unchanged at every column.  Included by lrp_hip.h (include that one); error codes, dtype codes
 * and conventions are lrp_hip.h's. */
#ifndef LRP_HIP_DECODE_H
#define LRP_HIP_DECODE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The caches: kc, vc [B, cap, nk d] token-major in the call's dtype, row pitch ldc elements, batch stride cap * ldc.  pos: device int32[1], the
 * column of the step -- ONE column for every prompt of the call (left-padded batches: all prompts end at the same column). */

/* lrp_decode_rope_append (csrc/decode.hip): per prompt b < B, with p = *pos,
 *     q_rot[b, h d + c]  = RoPE_p(qk[b, h d + c])               h < nq   (rotate-half pairs (c, c + d/2); cos / sin[p, :] of fp32 [table_rows, d])
 *     kc[b, p, h d + c]  = RoPE_p(qk[b, (nq + h) d + c])        h < nk
 *     vc[b, p, :]        = v[b, :]                               (a copy, bitwise)
 *   with the arithmetic and rounding order of lrp_rope_fwd: out1 = x1 cos[c] - x2 sin[c], out2 = x2 cos[c + d/2] + x1 sin[c + d/2] in fp32, no
 *   contraction, one rounding to the storage type -- bitwise lrp_rope_fwd(seq = 1) on the same rows with the tables' row p.
 *   qk [B, (nq + nk) d] (q | k, biased / head-normed by the caller) and v [B, nk d]: 2-D views with row pitches ldqk, ldv (the two column ranges
 *   of one qkv buffer);  q_rot [B, nq d] with pitch ldq.
 *   p < 0, p >= cap or p >= table_rows: NOTHING is written (q_rot neither); the guard is evaluated on the device before any address is formed
 *   from p, so no value of *pos can make the kernel store outside [0, cap) rows of a prompt's cache.
 *   NULL qk / v / cos_t / sin_t / pos / q_rot / kc / vc, B < 0, nq < 1, nk < 1, cap < 1, table_rows < 1, an unknown dtype -> LRP_EINVAL.
 *   d odd, d < 2, d > 256, d * sizeof(T) % 16 != 0, ldqk < (nq + nk) d, ldv < nk d, ldq < nq d, ldc < nk d -> LRP_ESHAPE.
 *   qk / v / q_rot / kc / vc / cos_t / sin_t off 16 bytes, pos off 4, a pitch that is not a multiple of 16 bytes -> LRP_EALIGN.
 *   B == 0 -> LRP_OK, nothing launched.  All of it before any launch.
 *   One launch, a thread per 16-byte vector of a (prompt, head) row; 16-byte loads and stores (the rotate-half partner vector too when d/2 is
 *   a whole number of vectors, element by element otherwise). */
int lrp_decode_rope_append(const void* qk, int64_t ldqk, const void* v, int64_t ldv, const float* cos_t, const float* sin_t, int table_rows,
                           const int* pos, void* q_rot, int64_t ldq, void* kc, void* vc, int64_t ldc, int B, int cap, int nq, int nk, int d,
                           int dtype, void* stream);

/* Keys per slab of lrp_attn_decode: a constant of the build.  Slab s holds keys [s SLAB, (s + 1) SLAB) counted from key 0 whatever B, cap and
 * *pos are, which is what makes the result independent of them. */
int lrp_attn_decode_slab(void);

/* Bytes of the workspace lrp_attn_decode needs: ceil(cap / SLAB) slab partials (acc [d], m, l in fp32) per (prompt, query head), rounded up to
 * 16 bytes; -1 for arguments the kernel does not take (B < 1, Hq < 1, d < 8, d > 256, d % 8 != 0, cap < 1). */
int64_t lrp_attn_decode_ws(int B, int Hq, int d, int cap);

/* lrp_attn_decode (csrc/decode.hip): single-query attention over the cache, with p = *pos, rep = Hq / Hkv and l_b = min(max(lo[b], 0), p),
 *     o[b, h, :] = sum_{l_b <= j <= p} softmax_j(scale q[b, h] . kc[b, j, h / rep]) vc[b, j, h / rep]          (o [B, Hq d], pitch ldo)
 *   q [B, Hq d] (pitch ldq; lrp_decode_rope_append's q_rot);  lo int32 [B]: the first live column of a left-padded prompt.
 *   No cache row outside [l_b, p] is loaded: such rows may hold anything (NaN included).  p < 0 or p >= cap: nothing is written.
 *   Launch 1, grid (ceil(cap / SLAB), Hkv, B) -- sized by cap, not by *pos: static under graph replay; a workgroup whose slab lies wholly
 *   outside [l_b, p] exits without a load.  256 threads, 16 lanes per key, K / V straight to registers in 16-byte loads, the rep query heads of
 *   a group share every K / V load (rep <= 8; beyond that, tiles of 8 heads, each loading the slab once), no MFMA (at most 8 live rows), no
 *   LDS for operands.  Scores, running max, sum and accumulators in fp32; a slab leaves (m, l, acc [d]) in ws.
 *   Launch 2, grid (Hq, B), one wave: the live slabs floor(l_b / SLAB) .. floor(p / SLAB) combined in ASCENDING order (their (m, l) fetched 64 at a
 *   time, their acc rows eight at a time), one rounding to the storage type.
 *   No atomics anywhere; every sum has a fixed order that depends on the key's index only: bitwise repeatable, a prompt's result does not
 *   depend on B, on the other prompts or on cap.
 *   NULL q / kc / vc / lo / pos / o / ws, B < 0, Hq < 1, Hkv < 1, cap < 1, an unknown dtype -> LRP_EINVAL.  Hq % Hkv != 0, d % 8 != 0, d < 8,
 *   d > 256, ldq < Hq d, ldo < Hq d, ldc < Hkv d, B > 65535 (a grid dimension), ws_bytes < lrp_attn_decode_ws(B, Hq, d, cap) -> LRP_ESHAPE.  q / kc / vc / o / ws off 16
 *   bytes, lo / pos off 4, a pitch that is not a multiple of 16 bytes -> LRP_EALIGN.  B == 0 -> LRP_OK, nothing launched.  All of it before any
 *   launch. */
int lrp_attn_decode(const void* q, int64_t ldq, const void* kc, const void* vc, int64_t ldc, const int* lo, const int* pos, void* o, int64_t ldo,
                    void* ws, int64_t ws_bytes, int B, int cap, int Hq, int Hkv, int d, float scale, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRP_HIP_DECODE_H */
