/* lrp_hip_wgrad.h -- part of the C ABI of liblrp_hip.so (version 8): the per-weight relevance of a Linear, the one entry that contracts over
 * the token dimension.  Included by lrp_hip.h (include that one); error codes, dtype codes and conventions are lrp_hip.h's. */
#ifndef LRP_HIP_WGRAD_H
#define LRP_HIP_WGRAD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* lrp_wgrad_rel (csrc/wgrad.hip):  out[r(n), k]  (+)=  W[n, k] * sum_{t < M} G[t, n] rs[t] X[t, k]     for n < N, k < K
 * -- `weight * weight.grad` of a Linear y = x W^T whose output gradient is G and whose input is X (ref: under lxt.efficient.monkey_patch the
 * Linears are plain nn.Linear, so logit.backward() leaves weight.grad = G^T X; the relevance of a weight is weight * weight.grad).
 *   G [M, N] (row pitch ldg), X [M, K] (ldx): token-major activations; W [N, K] (ldw): the weight as stored (a padded pitch is fine);
 *   all three LRP_F32 or all three LRP_BF16.  out: fp32, row pitch ldo, at least max r(n) + 1 rows.
 *   rs [M] fp32 or NULL: a per-token scale -- the 1 / rms of the norm in front of the Linear when X is the un-normed residual stream.
 *   rmap [N] int32 or NULL: the output row r(n) of weight row n (NULL: r(n) = n); the caller guarantees an injective map into out's rows
 *     (the library cannot read it on the host).  It lets a gate / up weight stored interleaved in blocks of LRP_GATED_IL land in HF order.
 *   accumulate: 0 -> out = ..., else out += ... (read-modify-write by the element's one owner thread: no atomics).
 *   LRP_BF16: both MFMA operands are transposed LDS reads of row-major 64-token tiles (v_mfma_f32_16x16x32_bf16, fp32 accumulation over
 *     ALL M tokens in one accumulator, token order); rs is folded into G while staging, G' = bf16(float(G) rs[t]) -- G takes the one extra
 *     bf16 rounding (2^-9 relative), X and W are used as stored; W acc is an fp32 product.  N and K multiples of 8.
 *   LRP_F32 (the parity path): LDS-tiled FMA; G rs X is formed and summed in fp64 and W acc rounded once to fp32.  Any N, K >= 1.
 *   Any M >= 1 (rows past M are staged as zeros).
 *   lrp_wgrad_rel_ok(...) -> 1 when the entry serves the problem, else the code the entry would return for it:
 *     an unknown dtype -> LRP_EINVAL;  M / N / K < 1, ldg < N, ldx / ldw / ldo < K, more than 65535 row tiles (128 rows in bf16, 64 in fp32),
 *     LRP_BF16 with N or K off the grid of 8 -> LRP_ESHAPE;  LRP_BF16 with ldg / ldx / ldw off the grid of 8 elements or ldo off the grid
 *     of 4 -> LRP_EALIGN.
 *   lrp_wgrad_rel adds: NULL G / X / W / out -> LRP_EINVAL;  G / X / W / out off 16 bytes (LRP_BF16) or 4 bytes (LRP_F32), rs / rmap off
 *     4 bytes -> LRP_EALIGN.  All of it before any launch.
 *   One launch, no workspace, no atomics; every result element has one owner thread that sums the tokens in order: bitwise repeatable. */
int lrp_wgrad_rel_ok(int M, int N, int K, int64_t ldg, int64_t ldx, int64_t ldw, int64_t ldo, int dtype);
int lrp_wgrad_rel(const void* G, const void* X, const void* W, float* out, const float* rs, const int* rmap, int M, int N, int K,
                  int64_t ldg, int64_t ldx, int64_t ldw, int64_t ldo, int accumulate, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRP_HIP_WGRAD_H */
