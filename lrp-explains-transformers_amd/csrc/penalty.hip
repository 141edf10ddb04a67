// penalty.hip -- the token history of a generate() call and the penalties on a step's logits (include/lrp_hip_penalty.h:
// lrp_token_hist_init, lrp_logit_penalty).
//
// hist int32 [B, V]: bit 31 = the column occurs in the prompt, bits 0..30 = how often it was generated in this call.  Both kernels are
// element-wise streams over a grid of (column chunks, rows), so one row of a 128 k vocabulary is spread over more than a hundred workgroups:
// 256 threads, 4 columns per thread as one 16-byte access where the bases and the pitches are on the 16-byte grid (the tail of such a row and
// every row of an unaligned call go element by element, thread t on columns t, t + 256, ... of the chunk: still coalesced).  No LDS, no atomics.
// The arithmetic is the header's sequence of individually rounded fp32 operations (-ffp-contract=off): the test holds it bit for bit.
#include "common.hpp"

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;

constexpr int NT = 256;
constexpr int CHUNK = 4 * NT;          // columns of one workgroup
constexpr int SEEN = (int)0x80000000u;
constexpr int CMASK = 0x7FFFFFFF;

LRP_DEVICE float penalise(float x, int h, float rp, float pp, float fp) {
    const int c = h & CMASK;
    if (rp != 1.0f && h != 0) x = x < 0.0f ? x * rp : x / rp;
    if (c > 0) {
        const float t = fp * (float)c;
        x = x - t;
        x = x - pp;
    }
    return x;
}

LRP_DEVICE int bump(int h) { return (h & CMASK) == CMASK ? h : h + 1; }

__global__ __launch_bounds__(NT) void hist_zero_kernel(int* __restrict__ hist, int64_t ldh, int B, int V, int vec) {
    const int64_t j0 = (int64_t)blockIdx.x * CHUNK;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        int* h = hist + b * ldh;
        const int64_t j = j0 + 4 * threadIdx.x;
        if (vec && j + 3 < V) {
            *reinterpret_cast<i32x4*>(h + j) = i32x4{0, 0, 0, 0};
        } else if (vec) {
            for (int64_t e = j; e < j + 4 && e < V; ++e) h[e] = 0;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t e = j0 + threadIdx.x + k * NT;
                if (e < V) h[e] = 0;
            }
        }
    }
}

__global__ __launch_bounds__(NT) void hist_flag_kernel(const int64_t* __restrict__ ids, int64_t ldi, const int* __restrict__ lo, int B, int S, int V,
                                                       int* __restrict__ hist, int64_t ldh) {
    const int64_t s = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (s >= S) return;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        if (lo && s < lo[b]) continue;
        const int64_t id = ids[b * ldi + s];
        if (id >= 0 && id < V) hist[b * ldh + id] = SEEN;
    }
}

__global__ __launch_bounds__(NT) void logit_penalty_kernel(const float* __restrict__ logits, int64_t ldl, float* __restrict__ out, int64_t ldo, int B,
                                                           int V, int* __restrict__ hist, int64_t ldh, const int* __restrict__ last, float rp,
                                                           float pp, float fp, const float* __restrict__ bias, int vec) {
    const int64_t j0 = (int64_t)blockIdx.x * CHUNK;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const float* l = logits + b * ldl;
        float* o = out + b * ldo;
        int* h = hist + b * ldh;
        const int64_t lastb = last ? (int64_t)last[b] : -1;          // (outside [0, V): matches no column)
        auto one = [&](int64_t e) {
            int he = h[e];
            if (e == lastb) { he = bump(he); h[e] = he; }
            float x = penalise(l[e], he, rp, pp, fp);
            if (bias) x = x + bias[e];
            o[e] = x;
        };
        const int64_t j = j0 + 4 * threadIdx.x;
        if (vec && j + 3 < V) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(l + j);
            i32x4 hv = *reinterpret_cast<const i32x4*>(h + j);
            f32x4 bv = {0.f, 0.f, 0.f, 0.f};
            if (bias) bv = *reinterpret_cast<const f32x4*>(bias + j);
            if (lastb >= j && lastb < j + 4) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j + e == lastb) { hv[e] = bump(hv[e]); h[j + e] = hv[e]; }
            }
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                y[e] = penalise(x[e], hv[e], rp, pp, fp);
                if (bias) y[e] = y[e] + bv[e];
            }
            *reinterpret_cast<f32x4*>(o + j) = y;
        } else if (vec) {
            for (int64_t e = j; e < j + 4 && e < V; ++e) one(e);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t e = j0 + threadIdx.x + k * NT;
                if (e < V) one(e);
            }
        }
    }
}

inline bool on16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool onN(const void* p, int n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
inline bool finite(float x) { return x >= -3.4028234663852886e38f && x <= 3.4028234663852886e38f; }
inline dim3 col_row_grid(int64_t cols, int per_block, int B) {
    return dim3((unsigned)((cols + per_block - 1) / per_block), (unsigned)(B < 65535 ? B : 65535));
}

}  // namespace

extern "C" int lrp_token_hist_init(const int64_t* ids, int64_t ld_ids, const int* lo, int B, int S, int V, int* hist, int64_t ld_hist,
                                   void* stream) {
    if (!ids || !hist || B < 0 || S < 0 || V < 1) return LRP_EINVAL;
    if (ld_ids < S || ld_hist < V) return LRP_ESHAPE;
    if (!onN(ids, 8) || !onN(lo, 4) || !onN(hist, 4)) return LRP_EALIGN;
    if (B == 0) return LRP_OK;
    hipStream_t st = (hipStream_t)stream;
    const int vec = on16(hist) && ld_hist % 4 == 0;
    hipLaunchKernelGGL(hist_zero_kernel, col_row_grid(V, CHUNK, B), dim3(NT), 0, st, hist, ld_hist, B, V, vec);
    if (S > 0) hipLaunchKernelGGL(hist_flag_kernel, col_row_grid(S, NT, B), dim3(NT), 0, st, ids, ld_ids, lo, B, S, V, hist, ld_hist);
    return lrp_check_launch();
}

extern "C" int lrp_logit_penalty(const float* logits, int64_t ld_logits, float* out, int64_t ld_out, int B, int V, int* hist, int64_t ld_hist,
                                 const int* last, float repetition_penalty, float presence_penalty, float frequency_penalty, const float* bias,
                                 void* stream) {
    if (!logits || !out || !hist || (const float*)out == logits || B < 0 || V < 1) return LRP_EINVAL;
    if (!(repetition_penalty > 0.f) || !finite(repetition_penalty) || !finite(presence_penalty) || !finite(frequency_penalty)) return LRP_EINVAL;
    if (ld_logits < V || ld_out < V || ld_hist < V) return LRP_ESHAPE;
    if (!onN(logits, 4) || !onN(out, 4) || !onN(hist, 4) || !onN(last, 4) || !onN(bias, 4)) return LRP_EALIGN;
    if (B == 0) return LRP_OK;
    const int vec = on16(logits) && on16(out) && on16(hist) && on16(bias) && ld_logits % 4 == 0 && ld_out % 4 == 0 && ld_hist % 4 == 0;
    hipLaunchKernelGGL(logit_penalty_kernel, col_row_grid(V, CHUNK, B), dim3(NT), 0, (hipStream_t)stream, logits, ld_logits, out, ld_out, B, V, hist,
                       ld_hist, last, repetition_penalty, presence_penalty, frequency_penalty, bias, vec);
    return lrp_check_launch();
}
