/* lrp_hip_mxfp4.h -- part of the C ABI of liblrp_hip.so (version 8): weight-only MXFP4 storage, the quantiser and its exact inverse
 * (csrc/mxfp4.hip).  Included by lrp_hip.h (include that one); error codes, dtype codes and conventions are lrp_hip.h's.
 *
 * The format (OCP Microscaling MXFP4: e2m1 elements, one power-of-two e8m0 scale per 32 elements), in full:
 *   - a row of a [rows, cols] matrix is cut into blocks of 32 consecutive elements along cols (the contraction dimension K of a stored [N, K]
 *     weight); cols % 32 == 0;
 *   - a block has ONE scale byte E, meaning X = 2^(E - 127), E <= 254 (E = 255 is NaN; the quantiser never emits it);
 *   - and 32 four-bit codes c: sign c >> 3, exponent e = (c >> 1) & 3, mantissa m = c & 1; magnitude m * 0.5 for e = 0, else
 *     (1 + m / 2) * 2^(e - 1) -- the magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6; the element is +-magnitude * X;
 *   - byte j of a row of codes holds element 2 j in its low nibble and element 2 j + 1 in its high nibble;
 *   - storage: codes [rows, cols / 2] uint8 with row pitch ldc (bytes), scales [rows, cols / 32] uint8 with row pitch lds (bytes).
 * 4 + 8 / 32 = 4.25 bits per element.
 *
 * Common to the two: dtype LRP_BF16 or LRP_F32 is the type of the un-quantised matrix (w / out, row pitch ldw / ldo in elements).  All checks run
 * before any launch: a NULL pointer or an unknown dtype -> LRP_EINVAL; rows < 1, cols < 32, cols % 32 != 0, a pitch smaller than its row, or
 * rows * cols / 32 >= 2^31 (the grid limit) -> LRP_ESHAPE; w / out / codes whose base or row pitch is off the 16-byte grid, scales whose base or row pitch
 * is off the 4-byte grid -> LRP_EALIGN.  One launch each, no workspace, no atomics, plain 16-byte vector loads and stores of w / out / codes;
 * every output byte of the rows' cols (cols / 2, cols / 32) is written (callers pass uninitialised memory); bitwise repeatable. */
#ifndef LRP_HIP_MXFP4_H
#define LRP_HIP_MXFP4_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* lrp_mxfp4_quantize: per block, amax = max |w_i|.  amax == 0 -> E = 0 and all codes 0.  Else E = floor(log2 amax) - 2 + 127 clamped to
 * [0, 254] (the exponent is taken from amax's bits), and each code is |w_i| / X -- a power-of-two scaling, exact in fp32 -- rounded to the nearest
 * magnitude, ties to the code with m = 0 (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4); anything above 6 saturates
 * to 6 (amax / X lies in [4, 8)).  The sign is kept, except that an element that rounds to magnitude 0 gets code 0 whatever its sign (so does
 * -0.0): quantize(dequant(codes, scales)) reproduces codes and scales byte for byte.  Non-finite input is the caller's to refuse. */
int lrp_mxfp4_quantize(const void* w, void* codes, void* scales, int rows, int cols, int64_t ldw, int64_t ldc, int64_t lds, int dtype,
                       void* stream);

/* lrp_mxfp4_dequant: out[r, i] = +-magnitude * X in dtype, row pitch ldo.  The product has two significant bits: exact in bf16 and in fp32
 * (E < 2 reaches the subnormals of both; E = 253, 254 with the codes of 4 and 6 pass their range and give inf -- the quantiser emits E <= 252
 * for finite input).  E = 255 gives NaN in the whole block. */
int lrp_mxfp4_dequant(const void* codes, const void* scales, void* out, int rows, int cols, int64_t ldc, int64_t lds, int64_t ldo, int dtype,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRP_HIP_MXFP4_H */
