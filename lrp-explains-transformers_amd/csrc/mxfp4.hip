// mxfp4.hip -- weight-only MXFP4 storage (e2m1 codes, one e8m0 scale per 32 elements along K): the quantiser and its exact inverse
// (C ABI and the format in full: include/lrp_hip_mxfp4.h).  Both are HBM-bound streaming kernels without reuse:
//   * dequant (the hot one: once per layer and pass in front of the GEMMs): a wave64 owns 64 consecutive blocks of one row.  Lane l LOADS the
//     16 code bytes of block l -- one 1-KiB wave instruction -- and the block's scale byte; the 2048 outputs leave in rounds of one 16-byte
//     store per lane, lane l writing the l-th 16-byte piece of the round's 1 KiB, so loads AND stores are fully coalesced.  The piece a lane
//     stores belongs to another lane's block: four code words and the scale travel by wave shuffle (ds_bpermute; ~20 per KiB stored, far
//     under the LDS rate).  0.53 bytes read and 2 written per bf16 element; ~7 VALU per element, under half of what the CU issues in the
//     time HBM takes for it.  No LDS allocation, 22 VGPRs: full occupancy, the latency is hidden by waves.
//   * quantise (load time only): one lane per block, 16-byte loads of its 32 elements, one 16-byte store of codes, one scale byte.
// Plain vector loads and stores only: no atomics, no workspace, every output byte is written.
#include "common.hpp"

namespace {

constexpr int MX_BLOCK = 32;      // elements per scale
constexpr int MX_WG = 256;        // threads per workgroup (whole waves work independently: no barrier anywhere)

LRP_DEVICE float bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }
LRP_DEVICE uint32_t f32_bits(float x) { return __builtin_bit_cast(uint32_t, x); }

// X = 2^(E - 127) as fp32: E = 0 is the subnormal 2^-127, E = 255 NaN
LRP_DEVICE float mx_scale(uint32_t E) { return bits_f32(E == 255u ? 0x7fc00000u : E == 0u ? 0x00400000u : E << 23); }

// element i (0 ... 7) of a word of eight codes -> +-magnitude * X.  The three magnitude bits k, placed at fp32's bits 22 ... 24, ARE the e2m1
// value scaled by 2^-126 (exponent field e, one mantissa bit m, and fp32's subnormal rule is e2m1's: k = 1 is 2^-127); two exact
// power-of-two multiplications bring it to magnitude * X, the sign bit rides along.  (fp32 denormals are honoured: the HIP default on gfx9.)
LRP_DEVICE float mx_decode(uint32_t word, int i, float X) {
    const uint32_t c = word >> (4 * i);
    return bits_f32(((c & 7u) << 22) | ((c & 8u) << 28)) * 0x1p126f * X;
}

template <typename T>
__global__ __launch_bounds__(MX_WG) void mxfp4_dequant_kernel(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales,
                                                              T* __restrict__ out, int rows, int nblk, int tpr, int64_t ldc, int64_t lds,
                                                              int64_t ldo) {
    constexpr int EPL = Vec16<T>::N;           // elements per 16-byte store: 8 (bf16) / 4 (fp32)
    constexpr int LPB = MX_BLOCK / EPL;        // lanes that store one block: 4 / 8; also the number of rounds
    constexpr int BPR = 64 / LPB;              // blocks stored per round: 16 / 8
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * (MX_WG / 64) + (threadIdx.x >> 6);
    if (tile >= (int64_t)rows * tpr) return;
    const int64_t row = tile / tpr;
    const int b0 = (int)(tile % tpr) * 64;     // first block of this wave's 64
    const bool have = b0 + lane < nblk;
    u32x4 cw = {0u, 0u, 0u, 0u};
    uint32_t E = 0;
    if (have) {
        cw = *reinterpret_cast<const u32x4*>(codes + row * ldc + (int64_t)(b0 + lane) * 16);
        E = scales[row * lds + b0 + lane];
    }
    const float X = mx_scale(E);
    const int sub = lane % LPB;                // which 16-byte piece of its block a lane stores
    T* orow = out + row * ldo + (int64_t)b0 * MX_BLOCK;
#pragma unroll
    for (int j = 0; j < LPB; ++j) {
        const int src = j * BPR + lane / LPB;  // the lane that loaded the block this lane stores a piece of in round j
        const uint32_t w0 = __shfl(cw[0], src, 64), w1 = __shfl(cw[1], src, 64), w2 = __shfl(cw[2], src, 64), w3 = __shfl(cw[3], src, 64);
        const float Xs = __shfl(X, src, 64);
        const int wi = sub * EPL / 8;          // bf16: a whole word per lane; fp32: half a word
        uint32_t word = wi == 0 ? w0 : wi == 1 ? w1 : wi == 2 ? w2 : w3;
        if constexpr (EPL == 4) word >>= 16 * (sub & 1);
        Vec16<T> v;
#pragma unroll
        for (int i = 0; i < EPL; ++i) v.set(i, mx_decode(word, i, Xs));
        if (b0 + src < nblk) st16(orow + (int64_t)(j * 64 + lane) * EPL, v);
    }
}

template <typename T>
__global__ __launch_bounds__(MX_WG) void mxfp4_quantize_kernel(const T* __restrict__ w, uint8_t* __restrict__ codes,
                                                               uint8_t* __restrict__ scales, int64_t total, int nblk, int64_t ldw,
                                                               int64_t ldc, int64_t lds) {
    constexpr int N = Vec16<T>::N;
    const int64_t g = (int64_t)blockIdx.x * MX_WG + threadIdx.x;      // (row, block) in row-major order
    if (g >= total) return;
    const int64_t row = g / nblk;
    const int b = (int)(g % nblk);
    const T* src = w + row * ldw + (int64_t)b * MX_BLOCK;
    float x[MX_BLOCK];
    uint32_t amax = 0;                          // max |w_i| on the bit patterns: monotonic for finite values
#pragma unroll
    for (int q = 0; q < MX_BLOCK / N; ++q) {
        const Vec16<T> v = ld16(src + q * N);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            x[q * N + i] = v.get(i);
            amax = max(amax, f32_bits(x[q * N + i]) & 0x7fffffffu);
        }
    }
    // floor(log2 amax) = (exponent field) - 127 for a normal amax; E = that - 2 + 127, clamped: a subnormal amax clamps to 0 either way
    const int E = amax == 0u ? 0 : min(max((int)(amax >> 23) - 2, 0), 254);
    u32x4 cw;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t word = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float xi = x[q * 8 + i];
            const float a = ldexpf(fabsf(xi), 127 - E);      // |w_i| / X, exact
            // nearest of 0, 0.5, 1, 1.5, 2, 3, 4, 6: the code is the number of midpoints passed; a tie goes to the even code (m = 0)
            uint32_t c = (uint32_t)(a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.f);
            if (c != 0u) c |= (f32_bits(xi) >> 28) & 8u;
            word |= c << (4 * i);
        }
        cw[q] = word;
    }
    *reinterpret_cast<u32x4*>(codes + row * ldc + (int64_t)b * 16) = cw;
    scales[row * lds + b] = (uint8_t)E;
}

inline bool al(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// the checks both entry points share; ldx: the pitch (elements) of the un-quantised matrix x
int check_mxfp4(const void* x, const void* codes, const void* scales, int rows, int cols, int64_t ldx, int64_t ldc, int64_t lds, int dtype) {
    if (!x || !codes || !scales || (dtype != LRP_F32 && dtype != LRP_BF16)) return LRP_EINVAL;
    if (rows < 1 || cols < MX_BLOCK || cols % MX_BLOCK != 0) return LRP_ESHAPE;
    if (ldx < cols || ldc < cols / 2 || lds < cols / MX_BLOCK) return LRP_ESHAPE;
    if ((int64_t)rows * (cols / MX_BLOCK) >= (1ll << 31)) return LRP_ESHAPE;
    const int es = dtype == LRP_F32 ? 4 : 2;
    if (!al(x, 16) || (ldx * es) % 16 != 0 || !al(codes, 16) || ldc % 16 != 0 || !al(scales, 4) || lds % 4 != 0) return LRP_EALIGN;
    return LRP_OK;
}

}  // namespace

extern "C" int lrp_mxfp4_quantize(const void* w, void* codes, void* scales, int rows, int cols, int64_t ldw, int64_t ldc, int64_t lds,
                                  int dtype, void* stream) {
    const int rc = check_mxfp4(w, codes, scales, rows, cols, ldw, ldc, lds, dtype);
    if (rc != LRP_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = cols / MX_BLOCK;
    const int64_t total = (int64_t)rows * nblk;
    const dim3 grid((unsigned)((total + MX_WG - 1) / MX_WG)), block(MX_WG);
    if (dtype == LRP_BF16)
        hipLaunchKernelGGL(mxfp4_quantize_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)w, (uint8_t*)codes, (uint8_t*)scales, total, nblk,
                           ldw, ldc, lds);
    else
        hipLaunchKernelGGL(mxfp4_quantize_kernel<float>, grid, block, 0, st, (const float*)w, (uint8_t*)codes, (uint8_t*)scales, total, nblk,
                           ldw, ldc, lds);
    return lrp_check_launch();
}

extern "C" int lrp_mxfp4_dequant(const void* codes, const void* scales, void* out, int rows, int cols, int64_t ldc, int64_t lds, int64_t ldo,
                                 int dtype, void* stream) {
    const int rc = check_mxfp4(out, codes, scales, rows, cols, ldo, ldc, lds, dtype);
    if (rc != LRP_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = cols / MX_BLOCK;
    const int tpr = (nblk + 63) / 64;          // wave tiles (64 blocks) per row
    const int64_t tiles = (int64_t)rows * tpr;
    const dim3 grid((unsigned)((tiles + MX_WG / 64 - 1) / (MX_WG / 64))), block(MX_WG);
    if (dtype == LRP_BF16)
        hipLaunchKernelGGL(mxfp4_dequant_kernel<bf16_t>, grid, block, 0, st, (const uint8_t*)codes, (const uint8_t*)scales, (bf16_t*)out, rows,
                           nblk, tpr, ldc, lds, ldo);
    else
        hipLaunchKernelGGL(mxfp4_dequant_kernel<float>, grid, block, 0, st, (const uint8_t*)codes, (const uint8_t*)scales, (float*)out, rows,
                           nblk, tpr, ldc, lds, ldo);
    return lrp_check_launch();
}
