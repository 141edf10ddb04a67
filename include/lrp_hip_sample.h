/* lrp_hip_sample.h -- part of the C ABI of liblrp_hip.so (version 8): the next token of a sampled continuation (temperature, top-k, top-p,
 * min-p, a counter-based uniform per row).  Included by lrp_hip.h (include that one); error codes and conventions are lrp_hip.h's. */
#ifndef LRP_HIP_SAMPLE_H
#define LRP_HIP_SAMPLE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* lrp_sample_rows (csrc/sample.hip): per row b < B of fp32 logits [B, V] (row pitch ld_logits; every entry finite or -inf, at least one
 * finite), with m = max_j l_j, T = temperature and q_j = exp((l_j - m) / T), draw one column.  Every filter is an upper set of the raw
 * logits, so the kept set is { j : l_j >= tau } for one threshold tau that is a logit of the row:
 *     top_k  (>= 1; 0 or >= V: off)  keep l_j >= the k-th largest logit; ties at the k-th value are all kept (exact on the stored values)
 *     top_p  (in (0, 1); >= 1: off)  after top-k, masses inside the top-k set: keep j iff the mass of the kept tokens with a STRICTLY larger
 *                                    logit is < top_p Z_k.  The largest logit is always kept; a tie group is kept or dropped whole
 *     min_p  (in (0, 1]; 0: off)     keep l_j >= m + T log(min_p), the threshold formed in fp64 (independent of the other two)
 *     draw   Z = sum of q over the kept columns, c_j the running sum of kept q in ascending column order: idx[b] = the first kept j with
 *            c_j > u Z.  top_k == 1 is the arg-max: the lowest column among the tied maxima for every u (lrp_argmax_rows's index)
 *     sample_logprob[b] = log(q_idx / Z)     n_kept[b] = the size of the kept set     u_out[b] = the uniform used
 *   u: u_in[b] when u_in is given (values outside [0, 1) are clamped into it), else Philox4x32-10 with key = (low, high 32 bits of seeds[b])
 *   and counter = (step, streams[b] or 0, 0, 0):  u = (word 0 >> 8) 2^-24 in [0, 1).
 *   ref: HF's TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper, MinPLogitsWarper in that order, then the inverse CDF at u.
 *   Masses are summed as fixed-point integers (q <= 1 taken to 44 fractional bits, truncated): the sums are associative, so the result is
 *   bitwise repeatable and does not depend on the pitch, the alignment or the other rows of the call; a column whose q is below 2^-44 is
 *   kept and counted but never drawn.
 *   NULL logits / idx, neither seeds nor u_in, B < 0, V < 1, temperature <= 0 or not finite, top_k < 0, top_p <= 0, min_p outside [0, 1],
 *   step < 0 -> LRP_EINVAL.  ld_logits < V -> LRP_ESHAPE.  A pointer off its element size (seeds: 8 bytes, the others 4) -> LRP_EALIGN.
 *   B == 0 -> LRP_OK, nothing launched.  All of it before any launch.  Whatever the row holds, nothing is read or written out of bounds and
 *   idx lands in [0, V).
 *   One launch, one workgroup per row (256 threads; 1024 for V > 8192), 16-byte loads where base and pitch are on the 16-byte grid.  The row
 *   is not sorted: tau comes from a radix select over the order-preserving 32-bit image of the logits, four 8-bit digits, 256-bin LDS
 *   histograms of counts (top-k) and of mass (top-p); the draw is a chunked prefix sum in column order.  Passes over the row: 1 (max) + 4 with
 *   top_k + 4 with top_p + 1 (draw); all filters off: 2.  LDS integer atomics only, no global atomics. */
int lrp_sample_rows(const float* logits, int64_t ld_logits, int B, int V, float temperature, int top_k, float top_p, float min_p,
                    const int64_t* seeds, const int* streams, int step, const float* u_in, int* idx, float* sample_logprob, int* n_kept,
                    float* u_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRP_HIP_SAMPLE_H */
