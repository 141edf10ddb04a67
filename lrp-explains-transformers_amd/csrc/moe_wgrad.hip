// moe_wgrad.hip -- the per-weight relevance of the routed experts of a sparse MoE layer (include/lrp_hip_moe_wgrad.h): the grouped form of
// wgrad.hip,  out[e][n, k] (+)= W[e][n, k] sum_{p in e} s(p) G[gp(p), n] X[xp(p), k],  the contraction running over the plan rows of ONE expert.
//
// Row addressing (plan layout: moe.hip; p = off[e] + t, t < cnt[e]; perm[p] = token k + slot):
//   gate_up: G row p (plan order), X row perm[p] / k (gathered by token), s = 1
//   down:    G row perm[p] / k (gathered by token), s = 1/2 w[perm[p]], X row p (plan order)
// off, cnt and perm are read on the device: no host sync, no workspace, no atomics.  The plan is stable (token order inside an expert), so
// the order of every sum is fixed: bitwise repeatable.
//
// bf16 (moe_wgrad_bf16_kernel): wgrad_rel_bf16_kernel's form -- a 128 (n) x 128 (k) tile per 4-wave workgroup, blockIdx.z = expert, the
// expert's rows walked in tiles of 64.  The LDS operand images, the transposed fragment read, the staging store, the MFMA block of a staged
// tile and the walk over a lane's accumulators are wgrad_tiles.hpp's (the dense kernel shares the first three and keeps the others written
// out: see that header); this file owns the row resolution, the global loads, the token loop and the epilogues.  Rows past the expert's count are staged as ZEROS; the row index (plan row or gathered token) and the
// scale are resolved ONE TILE AHEAD of the loads that use them (perm -> row is a dependent load chain: resolved a tile early it is off the
// loop's critical path), the loads one tile ahead of their LDS stores.  s is folded into G while staging (the down mode), G' = bf16(float(G)
// s): one extra bf16 rounding (1/2 w is exact).
// An expert WITHOUT rows (a branch that is uniform over the workgroup): accumulate = 0 -> its block is written as exact zeros whatever out
// and W hold; accumulate != 0 -> the block is not touched (and nothing of it is read).
// _q (W held as MXFP4, include/lrp_hip_moe_mxfp4.h): the epilogue reads one scale byte and two code bytes per 4 outputs and decodes them
// with the grouped GEMMs' helper (mx_decode8) -- every decoded value is exact in bf16 / fp32, so the result is bit-identical to the plain
// entry on the dequantised tensor.
// fp32 (moe_wgrad_f32_kernel, the parity path): the grouped form of wgrad_rel_f32_kernel: 64 x 64 outputs per workgroup, rows in tiles of
// 16, s G X formed exactly and summed in fp64, W acc rounded ONCE to fp32.
#include "moe_gemm.hpp"
#include "wgrad_tiles.hpp"

namespace {

constexpr int MW_GATE_UP = 0, MW_DOWN = 1;        // (LRP_MOE_WGRAD_GATE_UP / _DOWN)

// 4 of the 8 values of one code word times its block scale, as fp32 (every decoded value is exact in T)
template <typename T> LRP_DEVICE void mw_decode4(uint32_t word, uint32_t sc, float* w) {
    T v[8];
    mx_decode8(word, sc, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = (float)v[e];
}

// what an epilogue needs once per output row n of expert ex: row n of W[e] (Q: of its code and scale bytes) and of out[e]
struct MwRow {
    const void* w;
    const uint8_t* sc;
    float* out;
};
template <typename T, bool Q>
LRP_DEVICE MwRow mw_row(const void* W, const uint8_t* scales, float* out, int ex, int N, int K, int n) {
    const int64_t row = (int64_t)ex * N + n;
    if constexpr (Q) return MwRow{reinterpret_cast<const uint8_t*>(W) + row * (K >> 1), scales + row * (K >> 5), out + row * K};
    else return MwRow{reinterpret_cast<const T*>(W) + row * K, nullptr, out + row * K};
}

// W[e][n, k .. k + 3] as fp32: read as stored, or decoded from one scale byte and two code bytes (k is a multiple of 4, K of 128)
template <typename T, bool Q>
LRP_DEVICE void mw_weight4(const MwRow& r, int k, float* w) {
    if constexpr (Q) {
        const uint32_t word = *reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(r.w) + (k >> 1));
        mw_decode4<T>(word, r.sc[k >> 5], w);
    } else {
        const T* p = reinterpret_cast<const T*>(r.w) + k;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = (float)p[e];
    }
}

// the fp32 kernel's form: the 4 weights around column k of row `row` of the whole [E N, K] MXFP4 tensor, addressed from its base (with the
// row pointers of mw_row the fp32 MXFP4 epilogue grew by 118 instructions; in this form the fp32 kernels compile to their previous text)
LRP_DEVICE void mw_weight4_q(const void* W, const uint8_t* scales, int64_t row, int K, int k, float* w) {
    const uint8_t* codes = reinterpret_cast<const uint8_t*>(W);
    const uint32_t word = *reinterpret_cast<const uint16_t*>(codes + row * (K >> 1) + (k >> 1));
    mw_decode4<float>(word, scales[row * (K >> 5) + (k >> 5)], w);
}

template <int MODE, bool Q>
__global__ __launch_bounds__(256) void moe_wgrad_bf16_kernel(const bf16_t* __restrict__ G, const bf16_t* __restrict__ X, const void* __restrict__ W,
                                                             const uint8_t* __restrict__ scales, const bf16_t* __restrict__ w,
                                                             const int* __restrict__ plan, float* __restrict__ out, int R, int kslots, int E,
                                                             int N, int K, int64_t ldg, int64_t ldx, int accumulate) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int n0 = blockIdx.y * WG_TILE, k0 = blockIdx.x * WG_TILE, ex = blockIdx.z;
    const PlanView P = plan_view(plan, R, E);
    const int M = P.cnt[ex], p0 = P.off[ex];
    const WgLane L = wg_lane(tid);
    f32x4 acc[4][4];
    if (M == 0) {                                                          // (uniform: the whole workgroup leaves here)
        if (accumulate) return;
        wg_for_each(
            n0, k0, L, N, K, acc, [&](int n) { return out + ((int64_t)ex * N + n) * K; },
            [&](float* orow, int k, const f32x4&) { *reinterpret_cast<f32x4*>(orow + k) = f32x4{0.f, 0.f, 0.f, 0.f}; });     // (acc is not read)
        return;
    }
    // ---- staging: thread -> 16-byte chunk sch of the expert rows srow + 16 i
    const int sch = tid & 15, srow = tid >> 4;
    const bool gcol = n0 + sch * 8 < N, xcol = k0 + sch * 8 < K;      // (N, K are multiples of 8: a chunk is inside or outside as a whole)
    const bf16_t* gp = G + n0 + sch * 8;
    const bf16_t* xp = X + k0 + sch * 8;
    u32x4 gr[4], xr[4];
    float sv[4], svn[4];
    int grow[4], xrow[4];                                              // resolved rows of the NEXT tile to load; -1: past the expert's count
    auto resolve = [&](int t0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = t0 + srow + 16 * i;
            grow[i] = xrow[i] = -1;
            svn[i] = 0.f;
            if (t < M) {
                const int flat = P.perm[p0 + t], tok = flat / kslots;
                if constexpr (MODE == MW_GATE_UP) {
                    grow[i] = p0 + t;
                    xrow[i] = tok;
                } else {
                    grow[i] = tok;
                    xrow[i] = p0 + t;
                    svn[i] = 0.5f * (float)w[flat];
                }
            }
        }
    };
    auto load = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool ok = grow[i] >= 0;
            gr[i] = (ok && gcol) ? *reinterpret_cast<const u32x4*>(gp + (int64_t)grow[i] * ldg) : u32x4{0u, 0u, 0u, 0u};
            xr[i] = (ok && xcol) ? *reinterpret_cast<const u32x4*>(xp + (int64_t)xrow[i] * ldx) : u32x4{0u, 0u, 0u, 0u};
            sv[i] = svn[i];
        }
    };
    wg_clear(acc);

    resolve(0);
    load();
    resolve(WG_TT);
    for (int t0 = 0; t0 < M; t0 += WG_TT) {
        __syncthreads();                                               // the previous tile's fragment reads are done
        wg_stage<MODE == MW_DOWN>(smem, srow, sch, gr, xr, sv);
        __syncthreads();
        if (t0 + WG_TT < M) {                                          // (uniform branch) in flight under the MFMAs below
            load();
            resolve(t0 + 2 * WG_TT);
        }
        wg_mma_tile(smem, L, acc);
    }
    // ---- epilogue: out[e][n, k .. k + 3] (+)= W[e][n, k .. k + 3] acc
    auto row = [&](int n) { return mw_row<bf16_t, Q>(W, scales, out, ex, N, K, n); };
    wg_for_each(n0, k0, L, N, K, acc, row, [&](const MwRow& r, int k, const f32x4& a) {
        float wv[4];
        mw_weight4<bf16_t, Q>(r, k, wv);
        float* dst = r.out + k;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = wv[e] * a[e];
        if (accumulate) {
            const f32x4 old = *reinterpret_cast<const f32x4*>(dst);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += old[e];
        }
        *reinterpret_cast<f32x4*>(dst) = v;
    });
}

template <int MODE, bool Q>
__global__ __launch_bounds__(256) void moe_wgrad_f32_kernel(const float* __restrict__ G, const float* __restrict__ X, const void* __restrict__ W,
                                                            const uint8_t* __restrict__ scales, const float* __restrict__ w,
                                                            const int* __restrict__ plan, float* __restrict__ out, int R, int kslots, int E,
                                                            int N, int K, int64_t ldg, int64_t ldx, int accumulate) {
    __shared__ float Gs[WF_TT][WF_TILE], Xs[WF_TT][WF_TILE], Ss[WF_TT];
    __shared__ int Gi[WF_TT], Xi[WF_TT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n0 = blockIdx.y * WF_TILE, k0 = blockIdx.x * WF_TILE, ex = blockIdx.z;
    const PlanView P = plan_view(plan, R, E);
    const int M = P.cnt[ex], p0 = P.off[ex];
    float* oute = out + (int64_t)ex * N * K;
    if (M == 0 && accumulate) return;                                  // (uniform)
    double acc[4][4];
    wf_clear(acc);
    for (int t0 = 0; t0 < M; t0 += WF_TT) {
        __syncthreads();
        if (tid < WF_TT) {
            const int t = t0 + tid;
            int gi = -1, xi = -1;
            float s = 0.f;
            if (t < M) {
                const int flat = P.perm[p0 + t], tok = flat / kslots;
                gi = MODE == MW_GATE_UP ? p0 + t : tok;
                xi = MODE == MW_GATE_UP ? tok : p0 + t;
                s = MODE == MW_GATE_UP ? 1.f : 0.5f * w[flat];
            }
            Gi[tid] = gi;
            Xi[tid] = xi;
            Ss[tid] = s;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, r = e >> 6, c = e & 63;
            const int gi = Gi[r], xi = Xi[r];
            Gs[r][c] = (gi >= 0 && n0 + c < N) ? G[(int64_t)gi * ldg + n0 + c] : 0.f;
            Xs[r][c] = (xi >= 0 && k0 + c < K) ? X[(int64_t)xi * ldx + k0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int tt = 0; tt < WF_TT; ++tt) {
            const double r = (double)Ss[tt];
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
        const int64_t wrow = (int64_t)ex * N + n;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int k = k0 + tx * 4 + b;
            if (k >= K) continue;
            float* dst = oute + (int64_t)n * K + k;
            if (M == 0) {                                              // (accumulate = 0 here) exact zeros, W is not read
                *dst = 0.f;
                continue;
            }
            float wv;
            if constexpr (Q) {                                         // (K is a multiple of 128: k - b is a multiple of 4 inside one block)
                float w4[4];
                mw_weight4_q(W, scales, wrow, K, k - b, w4);
                wv = w4[b];
            } else {
                wv = reinterpret_cast<const float*>(W)[wrow * K + k];
            }
            float v = (float)((double)wv * acc[a][b]);
            if (accumulate) v += *dst;
            *dst = v;
        }
    }
}

int mw_check(int T, int k, int E, int N, int K, int64_t ldg, int64_t ldx, int mode, int dtype, int quantised) {
    if (mode != MW_GATE_UP && mode != MW_DOWN) return LRP_EINVAL;
    const int ok = wg_shape_ok(N, K, dtype);                               // (LRP_EINVAL or LRP_ESHAPE: both are judged before any LRP_EALIGN)
    if (ok != 1) return ok;
    if (T < 1 || k < 1 || E < 1 || N < 1 || K < 1) return LRP_ESHAPE;
    if (E > MOE_EMAX || (int64_t)T * k >= (1ll << 30)) return LRP_ESHAPE;
    if (ldg < N || ldx < K) return LRP_ESHAPE;
    if (quantised && K % 128) return LRP_ESHAPE;                          // rows of scale bytes on the 4-byte grid (lrp_hip_moe_mxfp4.h)
    if ((ldg * esz(dtype)) % 16 || (ldx * esz(dtype)) % 16) return LRP_EALIGN;
    return 1;
}

template <bool Q>
int mw_launch(const void* G, const void* X, const void* W, const void* scales, const void* w, const int* plan, float* out, int T, int k, int E,
              int N, int K, int64_t ldg, int64_t ldx, int mode, int accumulate, int dtype, void* stream) {
    if (!G || !X || !W || !plan || !out || (Q && !scales) || (mode == MW_DOWN && !w)) return LRP_EINVAL;
    const int ok = mw_check(T, k, E, N, K, ldg, ldx, mode, dtype, Q ? 1 : 0);
    if (ok != 1) return ok;
    if (!al16(G) || !al16(X) || !al16(W) || !al16(out)) return LRP_EALIGN;
    if (((uintptr_t)plan | (uintptr_t)scales) % 4 || (uintptr_t)w % esz(dtype)) return LRP_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* sc = reinterpret_cast<const uint8_t*>(scales);
    const int R = T * k;
    if (dtype == LRP_BF16) {
        const dim3 grid((unsigned)((K + WG_TILE - 1) / WG_TILE), (unsigned)((N + WG_TILE - 1) / WG_TILE), (unsigned)E);
        lrp_with_bool(mode == MW_DOWN, [&](auto DOWN) {
            constexpr int MODE = decltype(DOWN)::value ? MW_DOWN : MW_GATE_UP;
            hipLaunchKernelGGL((moe_wgrad_bf16_kernel<MODE, Q>), grid, dim3(256), WG_LDS, st, (const bf16_t*)G, (const bf16_t*)X, W, sc,
                               (const bf16_t*)w, plan, out, R, k, E, N, K, ldg, ldx, accumulate);
        });
    } else {
        const dim3 grid((unsigned)((K + WF_TILE - 1) / WF_TILE), (unsigned)((N + WF_TILE - 1) / WF_TILE), (unsigned)E);
        lrp_with_bool(mode == MW_DOWN, [&](auto DOWN) {
            constexpr int MODE = decltype(DOWN)::value ? MW_DOWN : MW_GATE_UP;
            hipLaunchKernelGGL((moe_wgrad_f32_kernel<MODE, Q>), grid, dim3(256), 0, st, (const float*)G, (const float*)X, W, sc, (const float*)w,
                               plan, out, R, k, E, N, K, ldg, ldx, accumulate);
        });
    }
    return lrp_check_launch();
}

}  // namespace

extern "C" int lrp_moe_wgrad_rel_ok(int T, int k, int E, int N, int K, int64_t ldg, int64_t ldx, int mode, int dtype, int quantised) {
    return mw_check(T, k, E, N, K, ldg, ldx, mode, dtype, quantised);
}

extern "C" int lrp_moe_wgrad_rel(const void* G, const void* X, const void* W, const void* w, const int* plan, float* out, int T, int k, int E,
                                 int N, int K, int64_t ldg, int64_t ldx, int mode, int accumulate, int dtype, void* stream) {
    return mw_launch<false>(G, X, W, nullptr, w, plan, out, T, k, E, N, K, ldg, ldx, mode, accumulate, dtype, stream);
}

extern "C" int lrp_moe_wgrad_rel_q(const void* G, const void* X, const void* codes, const void* scales, const void* w, const int* plan,
                                   float* out, int T, int k, int E, int N, int K, int64_t ldg, int64_t ldx, int mode, int accumulate,
                                   int dtype, void* stream) {
    return mw_launch<true>(G, X, codes, scales, w, plan, out, T, k, E, N, K, ldg, ldx, mode, accumulate, dtype, stream);
}
