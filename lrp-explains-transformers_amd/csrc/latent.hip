// latent.hip -- latent feature attribution read-outs (include/lrp_hip.h: lrp_colsum_dot; include/lrp_hip_latent.h: lrp_headdot).
//
// ---- lrp_colsum_dot
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

// ---- lrp_headdot
// out[b, h, t] = scale sum_{j < d} x[b S + t, (h / rep) d + j] g'[b S + t, h d + j]: the relevance of every attention head at every position
// (x = o, q, k or v; g = its gradient, per QUERY head; g' = g, or the forward rotate-half RoPE of g at position t -- the fused dQ kernel
// leaves RoPE^T(dq) and only the rotated q is kept: sum_d q dq = sum_d q_rot RoPE(dq_unrot)).  HBM-bound: x and g are read once, 16 bytes
// per lane; the rotation's partner vector and the fp32 tables are re-reads of lines the workgroup has in cache.
//
// Order of the sums (bitwise deterministic, batch invariant, no atomics): a workgroup owns HD_ROWS consecutive rows of ONE prompt, counted
// from the prompt's first row, and a block of up to HD_HEADS heads (all of them for nh <= 64).  A (row, head) dot belongs to a group of LG
// lanes (the power of two >= d / V, V = 16 / sizeof(T)): a lane multiplies its V elements in order, the group adds its lanes by an
// xor butterfly.  Consecutive groups take consecutive heads of a row, so a wave reads 1 KiB runs of g.  The sums go through an LDS tile
// [head][row] and leave as runs of HD_ROWS floats along t for each head (plain vector stores).
// Every load is in bounds by construction: a group past the last (row, head) of the block re-reads the last one and stores nothing, a lane
// past d reads element 0 and adds 0.
constexpr int HD_ROWS = 16;     // rows of one workgroup: B ceil(S / 16) workgroups (512 at B S = 8192: two per CU)
constexpr int HD_HEADS = 64;    // heads of one workgroup (LDS tile 64 x 17 floats)
constexpr int HD_UNROLL = 4;    // (row, head) items a group has in flight

inline int64_t hd_chunks(int S) { return ((int64_t)S + HD_ROWS - 1) / HD_ROWS; }

template <typename T, bool ROPE>
__global__ __launch_bounds__(256) void headdot_kernel(const T* __restrict__ x, const T* __restrict__ g, const float* __restrict__ cs,
                                                      const float* __restrict__ sn, float* __restrict__ out, int S, int nh, int rep, int d,
                                                      int64_t ldx, int64_t ldg, float scale, int lg_shift) {
    constexpr int V = 16 / sizeof(T);
    __shared__ float tile[HD_HEADS][HD_ROWS + 1];
    const int LG = 1 << lg_shift, NG = 256 >> lg_shift;
    const int gi = threadIdx.x >> lg_shift, li = threadIdx.x & (LG - 1);
    const int h0 = blockIdx.x * HD_HEADS, nhb = min(HD_HEADS, nh - h0);
    const int r0 = blockIdx.y * HD_ROWS, nr = min(HD_ROWS, S - r0), b = blockIdx.z;
    const int64_t row0 = (int64_t)b * S + r0;
    const int items = nr * nhb, half = d >> 1;
    const bool act = li * V < d;
    const int j = act ? li * V : 0;
    // the rotation's partner of elements j .. j + V - 1: one 16-byte vector when d / 2 is a multiple of V, else element by element
    const bool lo = j < half, pvec = (half % V) == 0;
    const int jp = lo ? j + half : j - half;
    for (int it0 = 0; it0 < items; it0 += NG * HD_UNROLL) {
        Vec16<T> xa[HD_UNROLL], ga[HD_UNROLL], gp[HD_UNROLL];
        int rr[HD_UNROLL], hh[HD_UNROLL];
#pragma unroll
        for (int u = 0; u < HD_UNROLL; ++u) {
            const int item = min(it0 + u * NG + gi, items - 1);
            rr[u] = item / nhb;
            hh[u] = item - rr[u] * nhb;
            const int h = h0 + hh[u];
            const T* gr = g + (row0 + rr[u]) * ldg + (int64_t)h * d;
            xa[u] = ld16(x + (row0 + rr[u]) * ldx + (int64_t)(h / rep) * d + j);
            ga[u] = ld16(gr + j);
            if constexpr (ROPE) {
                if (pvec) {
                    gp[u] = ld16(gr + jp);
                } else {
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        const int e = j + k;                       // (j + k < d: d is a multiple of V)
                        gp[u].set(k, to_f32(gr[e < half ? e + half : e - half]));
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < HD_UNROLL; ++u) {
            float acc = 0.f;
            if constexpr (ROPE) {
                const float* c = cs + (int64_t)(r0 + rr[u]) * d + j;
                const float* s = sn + (int64_t)(r0 + rr[u]) * d + j;
#pragma unroll
                for (int k4 = 0; k4 < V; k4 += 4) {
                    const f32x4 cv = *reinterpret_cast<const f32x4*>(c + k4), sv = *reinterpret_cast<const f32x4*>(s + k4);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float p = gp[u].get(k4 + k) * sv[k];
                        const bool low = pvec ? lo : (j + k4 + k < half);
                        acc += xa[u].get(k4 + k) * (ga[u].get(k4 + k) * cv[k] + (low ? -p : p));
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k) acc += xa[u].get(k) * ga[u].get(k);
            }
            acc = act ? acc : 0.f;
            for (int m = LG >> 1; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
            if (li == 0 && it0 + u * NG + gi < items) tile[hh[u]][rr[u]] = acc * scale;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nhb * HD_ROWS; i += 256) {
        const int h = i / HD_ROWS, r = i - h * HD_ROWS;
        if (r < nr) out[((int64_t)b * nh + h0 + h) * S + r0 + r] = tile[h][r];
    }
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

extern "C" int lrp_headdot(const void* x, const void* g, const float* cos, const float* sin, float* out, int M, int B, int S, int nh, int rep,
                           int d, int64_t ldx, int64_t ldg, float scale, int dtype, void* stream) {
    if (!x || !g || !out || (dtype != LRP_F32 && dtype != LRP_BF16) || (cos == nullptr) != (sin == nullptr)) return LRP_EINVAL;
    if (B < 1 || S < 1 || (int64_t)B * S != (int64_t)M || nh < 1 || rep < 1 || d < 1 || nh % rep != 0 || d > 256 || (cos && (d & 1)) ||
        B > 65535 || hd_chunks(S) > 65535 || ldx < (int64_t)(nh / rep) * d || ldg < (int64_t)nh * d)
        return LRP_ESHAPE;
    const int V = dtype == LRP_BF16 ? 8 : 4;
    if (((uintptr_t)x | (uintptr_t)g | (uintptr_t)cos | (uintptr_t)sin) % 16 || ldx % V || ldg % V || d % V || (uintptr_t)out % 4) return LRP_EALIGN;
    int lg_shift = 0;
    while ((V << lg_shift) < d) ++lg_shift;             // lanes of a (row, head) group: 1 .. 64
    const dim3 grid((unsigned)((nh + HD_HEADS - 1) / HD_HEADS), (unsigned)hd_chunks(S), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_T(dtype, {
        if (cos)
            hipLaunchKernelGGL((headdot_kernel<T, true>), grid, dim3(256), 0, st, (const T*)x, (const T*)g, cos, sin, out, S, nh, rep, d, ldx, ldg,
                               scale, lg_shift);
        else
            hipLaunchKernelGGL((headdot_kernel<T, false>), grid, dim3(256), 0, st, (const T*)x, (const T*)g, cos, sin, out, S, nh, rep, d, ldx, ldg,
                               scale, lg_shift);
    })
    return lrp_check_launch();
}
