// latent.hip -- latent feature attribution read-outs (include/lrp_hip.h: lrp_colsum_dot).
//
// out[b, j] = sum_{t < S} x[b S + t, j] g[b S + t, j]: the token-summed relevance of every hidden unit (a residual-stream dimension with
// x = h, g = G_h; an MLP neuron with x = m, g = G_m).  HBM-bound: 2 B S N sizeof(T) bytes are read once.
//
// Order of the sums (bitwise deterministic, batch invariant):
//   a workgroup owns a chunk of CS_ROWS rows of ONE prompt and 64 V columns (V = 16 / sizeof(T): one 16-byte load per lane and row, a wave
//   reads 1 KiB of a row); its four waves take rows r0 + w, r0 + w + 4, ... in order, the waves' sums are added in wave order -> one fp32
//   partial per (prompt, chunk, column) in the caller's workspace; a second kernel adds a prompt's chunk partials in chunk order.  Chunks
//   start at the prompt's first row, so a prompt's result depends on its own rows only.  One chunk per prompt (S <= CS_ROWS): the first
//   kernel writes out directly and no workspace is needed.
#include "common.hpp"

namespace {

constexpr int CS_ROWS = 64;     // rows of one workgroup (16 per wave)
constexpr int CS_WAVES = 4;

inline int64_t cs_chunks(int S) { return ((int64_t)S + CS_ROWS - 1) / CS_ROWS; }

template <typename T>
__global__ __launch_bounds__(64 * CS_WAVES) void colsum_dot_part_kernel(const T* __restrict__ x, const T* __restrict__ g, float* __restrict__ part,
                                                                       int S, int N, int64_t ldx, int64_t ldg, int nch) {
    constexpr int V = 16 / sizeof(T);
    __shared__ float red[CS_WAVES - 1][V][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.y, b = blockIdx.z;
    const int64_t j0 = ((int64_t)blockIdx.x * 64 + lane) * V;
    const int r0 = c * CS_ROWS, r1 = min(S, r0 + CS_ROWS);
    const int64_t row0 = (int64_t)b * S;
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    if (j0 + V <= N) {
#pragma unroll 8
        for (int r = r0 + w; r < r1; r += CS_WAVES) {
            const Vec16<T> a = ld16(x + (row0 + r) * ldx + j0);
            const Vec16<T> e = ld16(g + (row0 + r) * ldg + j0);
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] += a.get(k) * e.get(k);
        }
    } else if (j0 < N) {                      // the row's tail (N % V != 0): element-wise
        const int nt = (int)(N - j0);
        for (int r = r0 + w; r < r1; r += CS_WAVES) {
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (k < nt) acc[k] += to_f32(x[(row0 + r) * ldx + j0 + k]) * to_f32(g[(row0 + r) * ldg + j0 + k]);
        }
    }
    if (w > 0) {
#pragma unroll
        for (int k = 0; k < V; ++k) red[w - 1][k][lane] = acc[k];
    }
    __syncthreads();
    if (w != 0 || j0 >= N) return;
#pragma unroll
    for (int q = 0; q < CS_WAVES - 1; ++q) {
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] += red[q][k][lane];
    }
    float* dst = part + ((int64_t)b * nch + c) * N + j0;
#pragma unroll
    for (int k = 0; k < V; ++k)
        if (j0 + k < N) dst[k] = acc[k];
}

__global__ __launch_bounds__(256) void colsum_dot_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, int N, int nch) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (j >= N) return;
    const float* p = part + (int64_t)b * nch * N + j;
    float s = 0.f;
    for (int c = 0; c < nch; ++c) s += p[(int64_t)c * N];
    out[(int64_t)b * N + j] = s;
}

}  // namespace

#define DISPATCH_T(dtype, ...)                                              \
    if (dtype == LRP_F32) { typedef float T; __VA_ARGS__ }                  \
    else if (dtype == LRP_BF16) { typedef bf16_t T; __VA_ARGS__ }           \
    else return LRP_EINVAL;

extern "C" int64_t lrp_colsum_dot_ws(int B, int S, int N) {
    if (B < 1 || S < 1 || N < 1) return LRP_ESHAPE;
    const int64_t nch = cs_chunks(S);
    return nch == 1 ? 0 : (int64_t)B * nch * N * (int64_t)sizeof(float);
}

extern "C" int lrp_colsum_dot(const void* x, const void* g, float* out, void* ws, int M, int N, int B, int S, int64_t ldx, int64_t ldg,
                              int dtype, void* stream) {
    if (!x || !g || !out || (dtype != LRP_F32 && dtype != LRP_BF16)) return LRP_EINVAL;
    if (B < 1 || S < 1 || N < 1 || (int64_t)B * S != (int64_t)M || B > 65535 || cs_chunks(S) > 65535 || ldx < N || ldg < N) return LRP_ESHAPE;
    const int nch = (int)cs_chunks(S);
    if (nch > 1 && !ws) return LRP_EINVAL;
    const int V = dtype == LRP_BF16 ? 8 : 4;
    if (((uintptr_t)x | (uintptr_t)g) % 16 || ldx % V || ldg % V || (uintptr_t)out % 4 || (uintptr_t)ws % 4) return LRP_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    float* part = nch == 1 ? out : (float*)ws;
    const dim3 grid((unsigned)((N + 64 * V - 1) / (64 * V)), (unsigned)nch, (unsigned)B);
    DISPATCH_T(dtype, {
        hipLaunchKernelGGL((colsum_dot_part_kernel<T>), grid, dim3(64 * CS_WAVES), 0, st, (const T*)x, (const T*)g, part, S, N, ldx, ldg, nch);
    })
    if (nch > 1) {
        const int rc = lrp_check_launch();
        if (rc != LRP_OK) return rc;
        hipLaunchKernelGGL(colsum_dot_reduce_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)B), dim3(256), 0, st, (const float*)ws, out, N, nch);
    }
    return lrp_check_launch();
}
