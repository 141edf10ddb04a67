// wgrad.hip -- the per-weight relevance of a Linear, out[r(n), k] (+)= W[n, k] sum_t G[t, n] rs[t] X[t, k]  (include/lrp_hip_wgrad.h):
// the one GEMM form of the library that contracts over the TOKEN dimension, with the product by W and the accumulate in its epilogue.
// The LDS operand images (layout and bank argument), the transposed fragment read, the staging store and the tile constants are
// wgrad_tiles.hpp's, shared with the grouped form (moe_wgrad.hip).  The accumulator clear, the MFMA block of a staged tile and the epilogue
// loops are WRITTEN OUT here although that header has them as functions: see its head for the measurement that decided it.
//
// bf16 (wgrad_rel_bf16_kernel): a 128 (n) x 128 (k) tile per 4-wave workgroup, the tokens in tiles of 64.
//   Staging goes through registers (4 + 4 global 16-byte loads per thread and token tile, issued one tile ahead of their LDS stores, so the
//   loads of tile t + 1 can be in flight under the MFMAs of tile t -- the intent; no trace confirms the overlap, and the measured rate in DESIGN.md
//   section 16 says the token loop is what binds); rs is folded into G while staging: G' = bf16(float(G) rs[t]), one extra rounding.
//   The epilogue reads 4 bf16 of W, multiplies in fp32 and stores (or adds to) one float4 per 16 x 16 tile.
// fp32 (wgrad_rel_f32_kernel, the parity path): 64 x 64 outputs per workgroup, tokens in tiles of 16.  The token sum runs in fp64 (G rs X is
// formed exactly) and W acc is rounded ONCE to fp32, so the parity path's own error is one fp32 rounding whatever M is.
// Both kernels: one launch, no workspace, no atomics; a result element is formed by one thread in token order -- bitwise repeatable.
//
// lrp_wgrad (PLAIN = true of both kernels): the plain weight.grad of the same Linear, out[n, k] = sum_t G[t, n] X[t, k], in the operands' dtype.
// The token loops are the ones above (one body, two epilogues); the plain epilogue reads nothing: bf16 rounds the fp32 accumulator once
// (round-to-nearest-even) and stores one 8-byte bf16x4 per 16 x 16 tile and lane, fp32 rounds the fp64 sum once.
#include "wgrad_tiles.hpp"

namespace {

template <bool RS, bool PLAIN>
__global__ __launch_bounds__(256) void wgrad_rel_bf16_kernel(const bf16_t* __restrict__ G, const bf16_t* __restrict__ X,
                                                             const bf16_t* __restrict__ W, void* __restrict__ outp,
                                                             const float* __restrict__ rs, const int* __restrict__ rmap, int M, int N, int K,
                                                             int64_t ldg, int64_t ldx, int64_t ldw, int64_t ldo, int accumulate) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.y * WG_TILE, k0 = blockIdx.x * WG_TILE;
    // ---- staging: thread -> 16-byte chunk sch of the token rows srow + 16 i
    const int sch = tid & 15, srow = tid >> 4;
    const bool gcol = n0 + sch * 8 < N, xcol = k0 + sch * 8 < K;      // (N, K are multiples of 8: a chunk is inside or outside as a whole)
    const bf16_t* gp = G + n0 + sch * 8;
    const bf16_t* xp = X + k0 + sch * 8;
    u32x4 gr[4], xr[4];
    float rsv[4];
    auto load = [&](int t0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = t0 + srow + 16 * i;
            const bool ok = t < M;
            gr[i] = (ok && gcol) ? *reinterpret_cast<const u32x4*>(gp + (int64_t)t * ldg) : u32x4{0u, 0u, 0u, 0u};
            xr[i] = (ok && xcol) ? *reinterpret_cast<const u32x4*>(xp + (int64_t)t * ldx) : u32x4{0u, 0u, 0u, 0u};
            if constexpr (RS) rsv[i] = ok ? rs[t] : 0.f;
        }
    };
    // ---- fragment addresses: lane 4 q + p of a 16-lane group supplies row q, columns 4 p .. 4 p + 3 of the group's 4 x 16 block
    const int wn = wave >> 1, wk = wave & 1;
    const int i16 = lane & 15, hi = lane >> 4, q = i16 >> 2, p = i16 & 3;
    f32x4 acc[4][4];                                                   // [k tile jx][n tile jg]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    load(0);
    for (int t0 = 0; t0 < M; t0 += WG_TT) {
        __syncthreads();                                               // the previous tile's fragment reads are done
        wg_stage<RS>(smem, srow, sch, gr, xr, rsv);
        __syncthreads();
        if (t0 + WG_TT < M) load(t0 + WG_TT);                          // (uniform branch) in flight under the MFMAs below
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int r0 = 32 * ks + 8 * hi + q, r1 = r0 + 4;
            bf16x8 fg[4], fx[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cg = 8 * wn + 2 * j + (p >> 1), cx = 8 * wk + 2 * j + (p >> 1);
                fg[j] = wg_frag_tr(smem, wg_off(r0, cg) + 8 * (p & 1), wg_off(r1, cg) + 8 * (p & 1));
                fx[j] = wg_frag_tr(smem + WG_OPND, wg_off(r0, cx) + 8 * (p & 1), wg_off(r1, cx) + 8 * (p & 1));
            }
#pragma unroll
            for (int jx = 0; jx < 4; ++jx)
#pragma unroll
                for (int jg = 0; jg < 4; ++jg) acc[jx][jg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fx[jx], fg[jg], acc[jx][jg], 0, 0, 0);
        }
    }
    if constexpr (PLAIN) {
        // ---- plain epilogue: out[n, k .. k + 3] = bf16(acc), one rounding, nothing read
        bf16_t* out = static_cast<bf16_t*>(outp);
#pragma unroll
        for (int jg = 0; jg < 4; ++jg) {
            const int n = n0 + 64 * wn + 16 * jg + i16;
            if (n >= N) continue;
#pragma unroll
            for (int jx = 0; jx < 4; ++jx) {
                const int k = k0 + 64 * wk + 16 * jx + 4 * hi;
                if (k >= K) continue;                                  // (K is a multiple of 8: k < K means k + 3 < K)
                bf16x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (bf16_t)acc[jx][jg][e];
                *reinterpret_cast<bf16x4*>(out + (int64_t)n * ldo + k) = v;
            }
        }
        return;
    }
    // ---- epilogue: out[r(n), k .. k + 3] (+)= W[n, k .. k + 3] acc
    float* out = static_cast<float*>(outp);
#pragma unroll
    for (int jg = 0; jg < 4; ++jg) {
        const int n = n0 + 64 * wn + 16 * jg + i16;
        if (n >= N) continue;
        const int64_t orow = rmap ? (int64_t)rmap[n] : (int64_t)n;
#pragma unroll
        for (int jx = 0; jx < 4; ++jx) {
            const int k = k0 + 64 * wk + 16 * jx + 4 * hi;
            if (k >= K) continue;                                      // (K is a multiple of 8: k < K means k + 3 < K)
            const bf16x4 w = *reinterpret_cast<const bf16x4*>(W + (int64_t)n * ldw + k);
            float* dst = out + orow * ldo + k;
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (float)w[e] * acc[jx][jg][e];
            if (accumulate) {
                const f32x4 old = *reinterpret_cast<const f32x4*>(dst);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += old[e];
            }
            *reinterpret_cast<f32x4*>(dst) = v;
        }
    }
}

template <bool PLAIN>
__global__ __launch_bounds__(256) void wgrad_rel_f32_kernel(const float* __restrict__ G, const float* __restrict__ X, const float* __restrict__ W,
                                                            float* __restrict__ out, const float* __restrict__ rs, const int* __restrict__ rmap,
                                                            int M, int N, int K, int64_t ldg, int64_t ldx, int64_t ldw, int64_t ldo,
                                                            int accumulate) {
    __shared__ float Gs[WF_TT][WF_TILE], Xs[WF_TT][WF_TILE], Rs[WF_TT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n0 = blockIdx.y * WF_TILE, k0 = blockIdx.x * WF_TILE;
    double acc[4][4];
    wf_clear(acc);
    for (int t0 = 0; t0 < M; t0 += WF_TT) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, r = e >> 6, c = e & 63, t = t0 + r;
            Gs[r][c] = (t < M && n0 + c < N) ? G[(int64_t)t * ldg + n0 + c] : 0.f;
            Xs[r][c] = (t < M && k0 + c < K) ? X[(int64_t)t * ldx + k0 + c] : 0.f;
        }
        if (tid < WF_TT) Rs[tid] = (t0 + tid < M) ? (rs ? rs[t0 + tid] : 1.f) : 0.f;
        __syncthreads();
#pragma unroll 4
        for (int tt = 0; tt < WF_TT; ++tt) {
            const double r = (double)Rs[tt];
            double g[4], x[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) g[a] = (double)Gs[tt][ty * 4 + a] * r;         // exact: 24 + 24 bits
#pragma unroll
            for (int b = 0; b < 4; ++b) x[b] = (double)Xs[tt][tx * 4 + b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fma(g[a], x[b], acc[a][b]);
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int n = n0 + ty * 4 + a;
        if (n >= N) continue;
        const int64_t orow = rmap ? (int64_t)rmap[n] : (int64_t)n;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int k = k0 + tx * 4 + b;
            if (k >= K) continue;
            float* dst = out + orow * ldo + k;
            if constexpr (PLAIN) {
                *dst = (float)acc[a][b];
                continue;
            }
            float v = (float)((double)W[(int64_t)n * ldw + k] * acc[a][b]);
            if (accumulate) v += *dst;
            *dst = v;
        }
    }
}

}  // namespace

extern "C" int lrp_wgrad_rel_ok(int M, int N, int K, int64_t ldg, int64_t ldx, int64_t ldw, int64_t ldo, int dtype) {
    const int ok = wg_shape_ok(N, K, dtype);                              // (LRP_EINVAL or LRP_ESHAPE: both are judged before any LRP_EALIGN)
    if (ok != 1) return ok;
    if (M < 1 || N < 1 || K < 1 || ldg < N || ldx < K || ldw < K || ldo < K) return LRP_ESHAPE;
    if (dtype == LRP_BF16 && (ldg % 8 || ldx % 8 || ldw % 8 || ldo % 4)) return LRP_EALIGN;
    return 1;
}

extern "C" int lrp_wgrad_rel(const void* G, const void* X, const void* W, float* out, const float* rs, const int* rmap, int M, int N, int K,
                             int64_t ldg, int64_t ldx, int64_t ldw, int64_t ldo, int accumulate, int dtype, void* stream) {
    if (!G || !X || !W || !out) return LRP_EINVAL;
    const int ok = lrp_wgrad_rel_ok(M, N, K, ldg, ldx, ldw, ldo, dtype);
    if (ok != 1) return ok;
    const uintptr_t opnd = (uintptr_t)G | (uintptr_t)X | (uintptr_t)W | (uintptr_t)out;
    if (opnd % (dtype == LRP_BF16 ? 16 : 4) || ((uintptr_t)rs | (uintptr_t)rmap) % 4) return LRP_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == LRP_BF16) {
        const dim3 grid((unsigned)((K + WG_TILE - 1) / WG_TILE), (unsigned)((N + WG_TILE - 1) / WG_TILE));
        lrp_with_bool(rs != nullptr, [&](auto RS) {
            hipLaunchKernelGGL((wgrad_rel_bf16_kernel<decltype(RS)::value, false>), grid, dim3(256), WG_LDS, st, (const bf16_t*)G, (const bf16_t*)X,
                               (const bf16_t*)W, (void*)out, rs, rmap, M, N, K, ldg, ldx, ldw, ldo, accumulate);
        });
    } else {
        const dim3 grid((unsigned)((K + WF_TILE - 1) / WF_TILE), (unsigned)((N + WF_TILE - 1) / WF_TILE));
        hipLaunchKernelGGL(wgrad_rel_f32_kernel<false>, grid, dim3(256), 0, st, (const float*)G, (const float*)X, (const float*)W, out, rs, rmap, M, N, K,
                           ldg, ldx, ldw, ldo, accumulate);
    }
    return lrp_check_launch();
}

extern "C" int lrp_wgrad_ok(int M, int N, int K, int64_t ldg, int64_t ldx, int64_t ldo, int dtype) {
    const int ok = wg_shape_ok(N, K, dtype);
    if (ok != 1) return ok;
    if (M < 1 || N < 1 || K < 1 || ldg < N || ldx < K || ldo < K) return LRP_ESHAPE;
    if (dtype == LRP_BF16 && (ldg % 8 || ldx % 8 || ldo % 4)) return LRP_EALIGN;      // out: one 8-byte bf16x4 store per lane
    return 1;
}

extern "C" int lrp_wgrad(const void* G, const void* X, void* out, int M, int N, int K, int64_t ldg, int64_t ldx, int64_t ldo, int dtype,
                         void* stream) {
    if (!G || !X || !out) return LRP_EINVAL;
    const int ok = lrp_wgrad_ok(M, N, K, ldg, ldx, ldo, dtype);
    if (ok != 1) return ok;
    if (dtype == LRP_BF16 ? (((uintptr_t)G | (uintptr_t)X) % 16 || (uintptr_t)out % 8) : (((uintptr_t)G | (uintptr_t)X | (uintptr_t)out) % 4))
        return LRP_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == LRP_BF16) {
        const dim3 grid((unsigned)((K + WG_TILE - 1) / WG_TILE), (unsigned)((N + WG_TILE - 1) / WG_TILE));
        hipLaunchKernelGGL((wgrad_rel_bf16_kernel<false, true>), grid, dim3(256), WG_LDS, st, (const bf16_t*)G, (const bf16_t*)X,
                           (const bf16_t*)nullptr, out, (const float*)nullptr, (const int*)nullptr, M, N, K, ldg, ldx, (int64_t)0, ldo, 0);
    } else {
        const dim3 grid((unsigned)((K + WF_TILE - 1) / WF_TILE), (unsigned)((N + WF_TILE - 1) / WF_TILE));
        hipLaunchKernelGGL(wgrad_rel_f32_kernel<true>, grid, dim3(256), 0, st, (const float*)G, (const float*)X, (const float*)nullptr,
                           (float*)out, (const float*)nullptr, (const int*)nullptr, M, N, K, ldg, ldx, (int64_t)0, ldo, 0);
    }
    return lrp_check_launch();
}
