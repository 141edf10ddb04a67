/* lrp_hip_param_grad.h -- part of the C ABI of liblrp_hip.so (version 8): the ordinary parameter gradients of a trainable model under the drop-in
 * patches -- the plain weight.grad of a Linear and the column reductions behind norm-weight and bias gradients.
 * Included by lrp_hip.h (include that one); error codes, dtype codes and conventions are lrp_hip.h's. */
#ifndef LRP_HIP_PARAM_GRAD_H
#define LRP_HIP_PARAM_GRAD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* lrp_wgrad (csrc/wgrad.hip):  out[n, k] = sum_{t < M} G[t, n] X[t, k]     for n < N, k < K
 * -- `weight.grad` of a Linear y = x W^T whose output gradient is G and whose input is X (ref: under lxt.efficient.monkey_patch the Linears
 * are plain nn.Linear: logit.backward() leaves weight.grad = G^T X).  lrp_wgrad_rel without its W / rs / rmap / accumulate, in the parameter's
 * dtype.  A weight stored [in, out] (HF's Conv1D) is the same entry with the roles swapped: lrp_wgrad(G := X, X := G) gives out[k, n].
 *   G [M, N] (row pitch ldg), X [M, K] (ldx), out [N, K] (ldo): all three LRP_F32 or all three LRP_BF16.  Only out[n < N, k < K] is written.
 *   LRP_BF16: lrp_wgrad_rel's token loop (transposed LDS reads of row-major 64-token tiles, v_mfma_f32_16x16x32_bf16, fp32 accumulation over
 *     ALL M tokens in one accumulator, token order); the epilogue reads nothing: it rounds the accumulator ONCE to bf16 (round-to-nearest-
 *     even) and stores 8 bytes per 16 x 16 tile and lane.  out equals bf16(lrp_wgrad_rel with W = 1) bit for bit.  N and K multiples of 8.
 *   LRP_F32 (the parity path): LDS-tiled FMA; G X is formed and summed in fp64 and rounded once to fp32.  Any N, K >= 1.
 *   Any M >= 1 (rows past M are staged as zeros).
 *   lrp_wgrad_ok(...) -> 1 when the entry serves the problem, else the code the entry would return for it:
 *     an unknown dtype -> LRP_EINVAL;  M / N / K < 1, ldg < N, ldx / ldo < K, more than 65535 row tiles (128 rows in bf16, 64 in fp32),
 *     LRP_BF16 with N or K off the grid of 8 -> LRP_ESHAPE;  LRP_BF16 with ldg / ldx off the grid of 8 elements or ldo off the grid of 4
 *     -> LRP_EALIGN.
 *   lrp_wgrad adds: NULL G / X / out -> LRP_EINVAL;  G / X off 16 bytes or out off 8 bytes (LRP_BF16), any of them off 4 bytes (LRP_F32)
 *     -> LRP_EALIGN.  All of it before any launch.
 *   One launch, no workspace, no atomics; every result element has one owner thread that sums the tokens in order: bitwise repeatable. */
int lrp_wgrad_ok(int M, int N, int K, int64_t ldg, int64_t ldx, int64_t ldo, int dtype);
int lrp_wgrad(const void* G, const void* X, void* out, int M, int N, int K, int64_t ldg, int64_t ldx, int64_t ldo, int dtype, void* stream);

/* lrp_colsum_affine (csrc/param_grad.hip):  dw[j] = sum_{t < M} g[t, j] (x[t, j] - mu[t]) rs[t],   db[j] = sum_{t < M} g[t, j]     for j < N
 * -- the gradients of the vector parameters of y = (x - mu) rs w + b with the row statistics held constant (ref: the patched norm forwards
 * of lxt.efficient detach 1 / std; weight.grad and bias.grad are then these two column sums), and the bias gradient of a Linear.
 *   g, x: [M, N] with row pitches ldg, ldx (elements; any pitch >= N), both LRP_F32 or both LRP_BF16.  dw, db: fp32 [N].
 *   mu, rs: fp32 [M] or NULL (a NULL mu reads as 0, a NULL rs as 1).  RMSNorm, Gemma's (1 + w) norm: mu NULL, rs = 1 / rms; a per-head norm:
 *     the same with M = tokens * heads rows of N = head_dim; LayerNorm: mu = mean, rs = 1 / std.
 *   dw NULL: x, mu and rs are not read (a Linear's bias gradient).  db NULL: it is skipped.  One of the two must be given.
 *   A term of dw is formed in fp64 and rounded once when mu is given (x - mu cancels), else it is the fp32 product g (x rs).
 *   Sums (lrp_colsum_dot's discipline): fp32 partials of fixed 64-row chunks, rows of a chunk in a fixed order, go to the caller's workspace
 *     `ws` of lrp_colsum_affine_ws(M, N) bytes (0 for M <= 64: ws may be NULL); a second launch adds the chunks in order.  No atomics:
 *     bitwise repeatable.  Both bases and both pitches on the 16-byte grid: one 16-byte load per lane and row, a row's tail past the last
 *     16-byte vector element-wise; otherwise one element per lane.
 *   lrp_colsum_affine_ws: M / N < 1 -> LRP_ESHAPE.
 *   lrp_colsum_affine: NULL g, dw and db both NULL, dw without x, an unknown dtype, M > 64 without ws -> LRP_EINVAL;  M / N < 1, ldg < N,
 *     ldx < N (with dw), more than 65535 column blocks -> LRP_ESHAPE;  g / x off their element size, mu / rs / dw / db / ws off 4 bytes
 *     -> LRP_EALIGN.  All of it before any launch. */
int64_t lrp_colsum_affine_ws(int M, int N);
int lrp_colsum_affine(const void* g, const void* x, const float* mu, const float* rs, float* dw, float* db, void* ws, int M, int N, int64_t ldg,
                      int64_t ldx, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRP_HIP_PARAM_GRAD_H */
