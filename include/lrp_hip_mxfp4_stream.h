/* lrp_hip_mxfp4_stream.h -- part of the C ABI of liblrp_hip.so (version 8): the weight-streaming Linear forward on MXFP4 weights
 * (csrc/linear_stream_q.hip), the quantised twin of lrp_linear_stream_fwd_tk.  Included by lrp_hip.h (include that one); error codes, dtype
 * codes and conventions are lrp_hip.h's, the format is lrp_hip_mxfp4.h's.
 *
 *     z[M, N] = x[M, K] . D[N, K]^T (+ bias[N])
 * where D is the bf16 matrix lrp_mxfp4_dequant makes of codes [N, K / 2] (row pitch ldc BYTES) and scales [N, K / 32] (row pitch ldsc BYTES).
 * D is never written: the kernel reads the 4.25 bits per element, decodes them (v_cvt_scalef32_pk_bf16_fp4) on the way into the LDS image the
 * plain kernel stages, and runs the plain kernel's fragments, MFMAs, K splits and epilogue on it.
 *
 * BIT IDENTITY: for every argument set both entries accept, z equals, bit for bit, lrp_mxfp4_dequant into a bf16 matrix of any pitch followed
 * by lrp_linear_stream_fwd_tk with the same ws / tickets presence (each decoded value is exact in bf16; every accumulator receives the same
 * MFMAs on the same operand bits in the same order; the splits use the same count, K ranges and slab order).  E = 255 therefore gives what
 * lrp_mxfp4_dequant gives (a NaN block); the quantiser never emits it.
 *
 * One launch.  No atomics other than the ticket protocol it shares with the plain kernel (split form only); every sum has a fixed order:
 * bitwise repeatable.  Rows of codes / scales past N, and x rows past M, are never fetched; z rows / columns outside [M, N] never stored. */
#ifndef LRP_HIP_MXFP4_STREAM_H
#define LRP_HIP_MXFP4_STREAM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Can lrp_linear_stream_fwd_q serve the problem, and is it the right kernel for it?  Host code.  lrp_linear_stream_ok(M, N, K, ldx, K) -- the
 * plain kernel's answer on the dequantised shape: bf16, 1 <= M <= 128, K % 512 == 0, N * K < 2^30, enough 64-row workgroups (with K splits
 * where the weight is narrow) -- and the format's pitch rules: ldc >= K / 2, ldc % 16 == 0, ldsc >= K / 32, ldsc % 4 == 0, N * ldc < 2^30. */
int lrp_linear_stream_q_ok(int M, int N, int K, int64_t ldx, int64_t ldc, int64_t ldsc);

/* x [M, K] bf16 (dtype LRP_BF16; row pitch ldx elements), bias [N] bf16 or NULL, z [M, N] in out_dtype (LRP_BF16 / LRP_F32; pitch ldz).
 * ws / tickets: as lrp_linear_stream_fwd_tk -- lrp_linear_stream_fwd_ws(M, N, K) bytes and lrp_linear_stream_fwd_tickets(M, N, K) zero-initialised
 * 32-bit words private to the stream (re-armed to 0 by the launch): with both, narrow weights run lrp_linear_stream_fwd_splits(M, N, K) K
 * splits; with either NULL the full-K form runs, whatever the workgroup count.
 * All checks before any launch: a NULL x / codes / scales / z, a negative size, a dtype or out_dtype that is neither LRP_BF16 nor LRP_F32
 * -> LRP_EINVAL.  M == 0 or N == 0 -> LRP_OK, nothing launched.  dtype LRP_F32, M > 128, K < 512, K % 512 != 0, ldx < K, ldc < K / 2,
 * ldsc < K / 32, N * K, M * ldx, N * ldc or N * ldsc >= 2^30 -> LRP_ESHAPE.  x or codes off the 16-byte grid, ldx % 8, ldc % 16, scales or ldsc
 * off the 4-byte grid -> LRP_EALIGN; in the split form also z or ws off 16 bytes or ldz % 4 (as in the plain entry). */
int lrp_linear_stream_fwd_q(const void* x, const void* codes, const void* scales, const void* bias, void* z, int M, int N, int K, int64_t ldx,
                            int64_t ldc, int64_t ldsc, int64_t ldz, int dtype, int out_dtype, void* ws, void* tickets, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRP_HIP_MXFP4_STREAM_H */
