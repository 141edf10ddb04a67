/* lrp_hip_span.h -- part of the C ABI of liblrp_hip.so (version 8): the head seed of an answer-span explanation (many explained rows per
 * prompt, a weight per row, the logit or the log-probability as the explained function).  Included by lrp_hip.h (include that one); error
 * codes, dtype codes and conventions are lrp_hip.h's. */
#ifndef LRP_HIP_SPAN_H
#define LRP_HIP_SPAN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LRP_SPAN_LOGIT 0     /* f = l[idx]                    : no dense seed, the one-hot route of lrp_head_seed with rs as its row scale */
#define LRP_SPAN_LOGPROB 1   /* f = log_softmax(l)[idx]       : seed[r, j] = w_r (delta(j, idx_r) - softmax(l)_j)                          */

/* lrp_span_seed (csrc/span.hip): per row r < R of fp32 logits [R, V] (row pitch ld_logits), with m = max_j l_j, s = sum_j exp(l_j - m):
 *     logit[r]   = l[idx_r]                       (the stored value, bitwise)
 *     logprob[r] = (l[idx_r] - m) - log s         (= logit - lse with lse = m + log s; the maximum is taken off before the cancellation)
 *     rs[r]      = w_r rstd[r]                    (rs != NULL; the row scale lrp_head_seed takes in place of rstd: weight and final norm)
 *     seed[r, j] = w_r (delta(j, idx_r) - exp(l_j - m) / s)   for j < V   (objective == LRP_SPAN_LOGPROB), rounded ONCE to seed_dtype
 *   -- the gradient of sum_r w_r f(r) over the explained rows' logits.  ref: `log_softmax(logits[b, pos]).gather(tgt)` summed with weights
 *   and differentiated by autograd under lxt.efficient.monkey_patch.
 *   idx [R] int32 in [0, V) (the caller's contract; a row whose index is outside gets NaN in logit / logprob and a seed without the delta,
 *   and reads nothing out of bounds);  w [R] fp32 or NULL (= 1);  rstd [R] fp32, needed when rs is given;  seed [R, V] LRP_F32 or LRP_BF16
 *   with row pitch ld_seed, written only for LRP_SPAN_LOGPROB (NULL otherwise);  logit, logprob [R] fp32.  A row with w_r = 0 gives
 *   rs[r] = 0 and a seed row of zeros exactly (finite logits).
 *   NULL logits / idx / logit / logprob, R < 0, V < 1, an unknown objective, LRP_SPAN_LOGPROB without seed or with an unknown seed_dtype,
 *   rs without rstd -> LRP_EINVAL.  ld_logits < V, ld_seed < V -> LRP_ESHAPE.  logits / w / rstd / logit / logprob / rs off 4 bytes, seed off
 *   its element size -> LRP_EALIGN.  R == 0 -> LRP_OK, nothing launched.  All of it before any launch.
 *   One launch, one workgroup per row (256 threads; 1024 for V > 8192), two or three passes over the row (max; sum; seed -- at V = 128256 a
 *   row is 513 KB: the later passes are L2 hits), 16-byte loads and stores where the bases and pitches are on the 16-byte grid (the row's tail
 *   past the last whole vector, and any row otherwise, element by element), no LDS beyond the cross-wave reduction, no atomics.  A thread
 *   adds its elements in index order, a wave its lanes by an xor butterfly, the workgroup its waves in wave order: bitwise repeatable, and a
 *   row's result does not depend on the other rows of the call. */
int lrp_span_seed(const float* logits, int64_t ld_logits, const int* idx, const float* w, const float* rstd, int R, int V, int objective,
                  void* seed, int64_t ld_seed, int seed_dtype, float* logit, float* logprob, float* rs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRP_HIP_SPAN_H */
