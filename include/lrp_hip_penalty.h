/* lrp_hip_penalty.h -- part of the C ABI of liblrp_hip.so (version 8): the token history of one generate() call and the repetition /
 * presence / frequency penalties and the logit bias applied to a step's logits before the arg-max or the draw.  Included by lrp_hip.h
 * (include that one); error codes and conventions are lrp_hip.h's. */
#ifndef LRP_HIP_PENALTY_H
#define LRP_HIP_PENALTY_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The history table: hist int32 [B, V], row pitch ld_hist (elements).  Entry (b, j):
 *     bit 31        1 iff column j occurs in the prompt of row b (set by lrp_token_hist_init, never cleared afterwards)
 *     bits 0 .. 30  c = the number of times column j was generated in this call (lrp_logit_penalty's `last`); it saturates at 2^31 - 1
 * so "in the prompt" is hist < 0 and c = hist & 0x7FFFFFFF.  Entries in the pitch padding (columns >= V) are never read or written. */

/* lrp_token_hist_init (csrc/penalty.hip): hist[b, 0 .. V) = 0 for every row b < B, then bit 31 of hist[b, ids[b, s]] is set for every
 * lo[b] <= s < S (lo NULL: every s; columns before lo[b] are the pads of a left-padded prompt and are no history; a negative lo[b] counts
 * as 0).  ids int64 [B, S], row pitch ld_ids.  An id outside [0, V) is skipped: nothing is written out of bounds whatever ids holds.
 *   Two launches on `stream`: the zero fill (16-byte stores where base and pitch are on the 16-byte grid), then one thread per (b, s)
 *   storing the constant 0x80000000 -- threads that meet on one entry store the same word, so no atomics.
 *   NULL ids / hist, B < 0, S < 0, V < 1 -> LRP_EINVAL.  ld_ids < S or ld_hist < V -> LRP_ESHAPE.  ids off 8 bytes, lo / hist off 4 ->
 *   LRP_EALIGN.  B == 0 -> LRP_OK, nothing launched.  All of it before any launch. */
int lrp_token_hist_init(const int64_t* ids, int64_t ld_ids, const int* lo, int B, int S, int V, int* hist, int64_t ld_hist, void* stream);

/* lrp_logit_penalty (csrc/penalty.hip): out[b, j] = the processed logit of column j of row b, logits and out fp32 [B, V] with row pitches
 * ld_logits / ld_out (out distinct from logits; logits is not written).  One launch.
 *   history   when last (int32 [B]) is given and 0 <= last[b] < V, c of hist[b, last[b]] is first increased by 1 (saturating) and stored back
 *             by the thread that owns that column; the new count is the one used below.  No other entry of hist is written.
 *   then, with x = logits[b, j], seen = bit 31 of hist[b, j], c = its count, rp / pp / fp the three penalties, every line ONE individually
 *   rounded fp32 operation (no fused multiply-add), in exactly this order:
 *     1. if rp != 1 and (seen or c > 0):   x = (x < 0) ? x * rp : x / rp          (HF's RepetitionPenaltyLogitsProcessor over prompt + generated)
 *     2. if c > 0:                         t = fp * (float)c ;  x = x - t          ((float)c: round to nearest even)
 *     3. if c > 0:                         x = x - pp                              (2, 3: the OpenAI / vLLM definitions, generated tokens only)
 *     4. if bias (fp32 [V]) is given:      x = x + bias[j]                         (-inf bans column j)
 *   x < 0 is false for -0 (it is divided).  A -inf logit stays -inf (rp > 0, pp / fp / (float)c finite, bias < +inf).
 *   NULL logits / out / hist, out == logits, B < 0, V < 1, rp <= 0 or not finite, pp or fp not finite -> LRP_EINVAL.  ld_logits, ld_out or
 *   ld_hist < V -> LRP_ESHAPE.  A pointer off 4 bytes -> LRP_EALIGN.  B == 0 -> LRP_OK, nothing launched.  All of it before any launch.
 *   An element-wise streaming kernel, grid (1024-column chunks, rows): 12 bytes per element (+ 4 with bias), 16-byte loads and stores where
 *   the bases and pitches are on the 16-byte grid, element by element otherwise and on the row's tail.  No LDS, no atomics; a row's result
 *   depends on that row only; bitwise repeatable; nothing is read or written outside [0, V) of a row. */
int lrp_logit_penalty(const float* logits, int64_t ld_logits, float* out, int64_t ld_out, int B, int V, int* hist, int64_t ld_hist, const int* last,
                      float repetition_penalty, float presence_penalty, float frequency_penalty, const float* bias, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRP_HIP_PENALTY_H */
