/* lrp_hip_moe_mxfp4.h -- part of the C ABI of liblrp_hip.so (version 8): the four grouped expert GEMMs of the MoE section of lrp_hip.h with
 * the expert weights held as MXFP4 and decoded INSIDE the GEMM (csrc/moe_mxfp4.hip).  Included by lrp_hip.h (include that one); error codes,
 * dtype codes, the routing plan and every operand other than the weight are those of the unquantised sibling (same name without _q).
 *
 * Layout of a quantised expert tensor.  An expert tensor [E, N, K] (gate_up_proj [E, 2 I, H], down_proj [E, H, I]) is the 2-D format of
 * lrp_hip_mxfp4.h applied to the tensor viewed as [E N, K], contiguous:
 *   - codes  [E, N, K / 2]  uint8, byte j of a row holds element 2 j in its low nibble and element 2 j + 1 in its high nibble;
 *   - scales [E, N, K / 32] uint8, one e8m0 byte per 32 consecutive elements of a STORED row (value 2^(E - 127));
 * so lrp_mxfp4_quantize / lrp_mxfp4_dequant with rows = E N, cols = K, ldc = K / 2, lds = K / 32 produce and invert it unchanged.  Row
 * pitches and expert strides are implied (no padding).  Blocks always run along the stored row: in the two forwards (B read as [N, K]) that
 * is the contraction dimension, in the two dgrads (B read as [K, N]) the output dimension.  H and I are multiples of 128, so K / 32 is a
 * multiple of 4 and every row of codes sits on the 16-byte grid when the base does.
 *
 * Contract.  Every decoded value is exact in bf16 and in fp32, it lands in the same LDS slot the unquantised kernel fills, and every
 * accumulator receives the same MFMAs on ascending K: each output is BIT-IDENTICAL to lrp_mxfp4_dequant into a dtype tensor followed by the
 * sibling.  No scratch copy of the weights exists and nothing but the one GEMM is launched; 0.53 bytes are read per weight element.
 *
 * All checks run before any launch, in the sibling's order and with its codes; in the place of the sibling's weight check: codes or scales
 * NULL -> LRP_EINVAL; codes base off the 16-byte grid or scales base off the 4-byte grid -> LRP_EALIGN. */
#ifndef LRP_HIP_MOE_MXFP4_H
#define LRP_HIP_MOE_MXFP4_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* lrp_moe_gate_up_fwd with Wgu [E, 2 I, H] as codes [E, 2 I, H / 2] + scales [E, 2 I, H / 32] */
int lrp_moe_gate_up_fwd_q(const void* x, const void* codes, const void* scales, const int* plan, void* coef, void* m, int T, int k, int E, int H,
                          int I, int64_t ldx, int64_t ldcoef, int64_t ldm, int act, int dtype, void* stream);

/* lrp_moe_down_fwd with Wd [E, H, I] as codes [E, H, I / 2] + scales [E, H, I / 32] */
int lrp_moe_down_fwd_q(const void* m, const void* codes, const void* scales, const int* plan, void* y, int T, int k, int E, int H, int I,
                       int64_t ldm, int64_t ldy, int dtype, void* stream);

/* lrp_moe_down_dgrad with Wd as above (read as [K = H, N = I]: the blocks run along the output dimension) */
int lrp_moe_down_dgrad_q(const void* G, const void* codes, const void* scales, const void* coef, const void* m, const void* w, const int* plan,
                         void* Agu, float* gw_part, int T, int k, int E, int H, int I, int64_t ldg, int64_t ldcoef, int64_t ldm, int64_t ldagu,
                         int dtype, void* stream);

/* lrp_moe_gate_up_dgrad with Wgu as above (read as [K = 2 I, N = H]) */
int lrp_moe_gate_up_dgrad_q(const void* Agu, const void* codes, const void* scales, const int* plan, void* gx_rows, int T, int k, int E, int H,
                            int I, int64_t ldagu, int64_t ldgx, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRP_HIP_MOE_MXFP4_H */
