// param_grad.hip -- the column reductions behind the gradients of vector parameters (include/lrp_hip_param_grad.h: lrp_colsum_affine):
//   dw[j] = sum_{t < M} g[t, j] (x[t, j] - mu[t]) rs[t]      the weight of an RMSNorm / Gemma (1 + w) norm / per-head norm (mu = NULL), of a LayerNorm
//   db[j] = sum_{t < M} g[t, j]                              the bias of a LayerNorm, a Linear, a Conv1D, a patch Conv2d
// HBM-bound: g (and x) are read once, 16 bytes per lane and row where the operands allow it.
//
// Order of the sums (lrp_colsum_dot's discipline, csrc/latent.hip: bitwise repeatable, no atomics):
//   a workgroup owns a chunk of PG_ROWS rows and 64 V columns (V = 16 / sizeof(T) elements per lane when both bases and both row pitches
//   sit on the 16-byte grid, else V = 1: one element per lane, any pitch); its four waves take rows r0 + w, r0 + w + 4, ... in order, the
//   waves' sums are added in wave order -> one fp32 partial per (chunk, column) in the caller's workspace; a second kernel adds the chunk
//   partials in chunk order.  One chunk (M <= PG_ROWS): the first kernel writes dw / db directly and no workspace is needed.
// A term of dw: with mu the difference needs more than fp32 (x - mu cancels), so g (x - mu) rs is formed in fp64 and rounded ONCE to fp32;
// without mu it is the fp32 product g (x rs) -- two roundings, one when rs is NULL too (x 1.0f is exact).  The sums are fp32.
#include "common.hpp"

namespace {

constexpr int PG_ROWS = 64;     // rows of one workgroup (16 per wave)
constexpr int PG_WAVES = 4;

inline int64_t pg_chunks(int M) { return ((int64_t)M + PG_ROWS - 1) / PG_ROWS; }

template <bool MU>
LRP_DEVICE float pg_term(float g, float x, float mu, float rs) {
    if constexpr (MU) return (float)((double)g * (((double)x - (double)mu) * (double)rs));
    else return g * (x * rs);
}

template <typename T, int V, bool DW, bool DB, bool MU>
__global__ __launch_bounds__(64 * PG_WAVES) void colsum_affine_part_kernel(const T* __restrict__ g, const T* __restrict__ x,
                                                                          const float* __restrict__ mu, const float* __restrict__ rs,
                                                                          float* __restrict__ part_w, float* __restrict__ part_b, int M, int N,
                                                                          int64_t ldg, int64_t ldx) {
    __shared__ float red[PG_WAVES - 1][2][V][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x;
    const int64_t j0 = ((int64_t)blockIdx.y * 64 + lane) * V;
    const int r0 = c * PG_ROWS, r1 = min(M, r0 + PG_ROWS);
    float aw[V], ab[V];
#pragma unroll
    for (int k = 0; k < V; ++k) aw[k] = ab[k] = 0.f;
    if constexpr (V > 1) {
        if (j0 + V <= N) {
#pragma unroll 4
            for (int r = r0 + w; r < r1; r += PG_WAVES) {
                const Vec16<T> e = ld16(g + (int64_t)r * ldg + j0);
                if constexpr (DW) {
                    const Vec16<T> a = ld16(x + (int64_t)r * ldx + j0);
                    const float m = MU ? mu[r] : 0.f, s = rs ? rs[r] : 1.f;
#pragma unroll
                    for (int k = 0; k < V; ++k) aw[k] += pg_term<MU>(e.get(k), a.get(k), m, s);
                }
                if constexpr (DB) {
#pragma unroll
                    for (int k = 0; k < V; ++k) ab[k] += e.get(k);
                }
            }
        } else if (j0 < N) {                  // the row's tail (N % V != 0): element-wise
            const int nt = (int)(N - j0);
            for (int r = r0 + w; r < r1; r += PG_WAVES) {
                const float m = (DW && MU) ? mu[r] : 0.f, s = (DW && rs) ? rs[r] : 1.f;
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    if (k < nt) {
                        const float e = to_f32(g[(int64_t)r * ldg + j0 + k]);
                        if constexpr (DW) aw[k] += pg_term<MU>(e, to_f32(x[(int64_t)r * ldx + j0 + k]), m, s);
                        if constexpr (DB) ab[k] += e;
                    }
                }
            }
        }
    } else {
        if (j0 < N) {
            for (int r = r0 + w; r < r1; r += PG_WAVES) {
                const float e = to_f32(g[(int64_t)r * ldg + j0]);
                if constexpr (DW) aw[0] += pg_term<MU>(e, to_f32(x[(int64_t)r * ldx + j0]), MU ? mu[r] : 0.f, rs ? rs[r] : 1.f);
                if constexpr (DB) ab[0] += e;
            }
        }
    }
    if (w > 0) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if constexpr (DW) red[w - 1][0][k][lane] = aw[k];
            if constexpr (DB) red[w - 1][1][k][lane] = ab[k];
        }
    }
    __syncthreads();
    if (w != 0 || j0 >= N) return;
#pragma unroll
    for (int q = 0; q < PG_WAVES - 1; ++q) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if constexpr (DW) aw[k] += red[q][0][k][lane];
            if constexpr (DB) ab[k] += red[q][1][k][lane];
        }
    }
    const int64_t o = (int64_t)c * N + j0;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        if (j0 + k < N) {
            if constexpr (DW) part_w[o + k] = aw[k];
            if constexpr (DB) part_b[o + k] = ab[k];
        }
    }
}

// blockIdx.y = 0: dw from part_w, 1: db from part_b (a NULL output is skipped)
__global__ __launch_bounds__(256) void colsum_affine_reduce_kernel(const float* __restrict__ part_w, const float* __restrict__ part_b,
                                                                  float* __restrict__ dw, float* __restrict__ db, int N, int nch) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const float* p = blockIdx.y ? part_b : part_w;
    float* out = blockIdx.y ? db : dw;
    if (j >= N || !out) return;
    float s = 0.f;
    for (int c = 0; c < nch; ++c) s += p[(int64_t)c * N + j];
    out[j] = s;
}

template <typename T, int V>
void pg_launch(dim3 grid, hipStream_t st, const void* g, const void* x, const float* mu, const float* rs, float* pw, float* pb, int M, int N,
               int64_t ldg, int64_t ldx) {
    lrp_with_bool(pw != nullptr, [&](auto DW) {
        lrp_with_bool(pb != nullptr, [&](auto DB) {
            lrp_with_bool(mu != nullptr, [&](auto MU) {
                constexpr bool dw = decltype(DW)::value, dbias = decltype(DB)::value, hasmu = decltype(MU)::value;
                if constexpr ((dw || dbias) && (dw || !hasmu))
                    hipLaunchKernelGGL((colsum_affine_part_kernel<T, V, dw, dbias, hasmu>), grid, dim3(64 * PG_WAVES), 0, st, (const T*)g,
                                       (const T*)x, mu, rs, pw, pb, M, N, ldg, ldx);
            });
        });
    });
}

}  // namespace

extern "C" int64_t lrp_colsum_affine_ws(int M, int N) {
    if (M < 1 || N < 1) return LRP_ESHAPE;
    const int64_t nch = pg_chunks(M);
    return nch == 1 ? 0 : 2 * nch * N * (int64_t)sizeof(float);
}

extern "C" int lrp_colsum_affine(const void* g, const void* x, const float* mu, const float* rs, float* dw, float* db, void* ws, int M, int N,
                                 int64_t ldg, int64_t ldx, int dtype, void* stream) {
    if (!g || (!dw && !db) || (dw && !x) || (dtype != LRP_F32 && dtype != LRP_BF16)) return LRP_EINVAL;
    if (M < 1 || N < 1 || ldg < N || (dw && ldx < N)) return LRP_ESHAPE;
    const int es = dtype == LRP_BF16 ? 2 : 4, VV = 16 / es;
    const int nch = (int)pg_chunks(M);
    if (nch > 1 && !ws) return LRP_EINVAL;
    if (!dw) { x = nullptr; mu = nullptr; rs = nullptr; ldx = 0; }     // a bias gradient: x and the row statistics are not read
    if (((uintptr_t)g | (uintptr_t)x) % es || ((uintptr_t)mu | (uintptr_t)rs | (uintptr_t)dw | (uintptr_t)db | (uintptr_t)ws) % 4) return LRP_EALIGN;
    const bool vec = ((uintptr_t)g | (uintptr_t)x) % 16 == 0 && ldg % VV == 0 && ldx % VV == 0;
    const int V = vec ? VV : 1;
    const int64_t cb = ((int64_t)N + 64 * V - 1) / (64 * V);
    if (cb > 65535) return LRP_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    float* pw = dw ? (nch == 1 ? dw : (float*)ws) : nullptr;
    float* pb = db ? (nch == 1 ? db : (float*)ws + (int64_t)nch * N) : nullptr;
    const dim3 grid((unsigned)nch, (unsigned)cb);
    if (dtype == LRP_F32) {
        if (vec) pg_launch<float, 4>(grid, st, g, x, mu, rs, pw, pb, M, N, ldg, ldx);
        else pg_launch<float, 1>(grid, st, g, x, mu, rs, pw, pb, M, N, ldg, ldx);
    } else {
        if (vec) pg_launch<bf16_t, 8>(grid, st, g, x, mu, rs, pw, pb, M, N, ldg, ldx);
        else pg_launch<bf16_t, 1>(grid, st, g, x, mu, rs, pw, pb, M, N, ldg, ldx);
    }
    if (nch > 1) {
        const int rc = lrp_check_launch();
        if (rc != LRP_OK) return rc;
        hipLaunchKernelGGL(colsum_affine_reduce_kernel, dim3((unsigned)((N + 255) / 256), 2u), dim3(256), 0, st, (const float*)pw, (const float*)pb,
                           dw, db, N, nch);
    }
    return lrp_check_launch();
}
