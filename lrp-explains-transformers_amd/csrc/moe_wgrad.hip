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
// expert's rows walked in tiles of 64, both MFMA operands ds_read_b64_tr_b16 reads of the xor-swizzled row-major LDS images (same offsets
// as wgrad.hip: see the bank argument there), v_mfma_f32_16x16x32_bf16 into one fp32 accumulator set.  Rows past the expert's count are
// staged as ZEROS under a full EXEC mask; the row index (plan row or gathered token) and the scale are resolved ONE TILE AHEAD of the
// loads that use them (perm -> row is a dependent load chain: resolved a tile early it is off the loop's critical path), the loads one
// tile ahead of their LDS stores.  s is folded into G while staging, G' = bf16(float(G) s): one extra bf16 rounding (1/2 w is exact).
// A separate kernel, not a shared template with wgrad.hip: the dense kernel compiles exactly as it did.
// An expert WITHOUT rows (a branch that is uniform over the workgroup): accumulate = 0 -> its block is written as exact zeros whatever out
// and W hold; accumulate != 0 -> the block is not touched (and nothing of it is read).
// _q (W held as MXFP4, include/lrp_hip_moe_mxfp4.h): the epilogue reads one scale byte and two code bytes per 4 outputs and decodes them
// with the grouped GEMMs' helper (mx_decode8) -- every decoded value is exact in bf16 / fp32, so the result is bit-identical to the plain
// entry on the dequantised tensor.
// fp32 (moe_wgrad_f32_kernel, the parity path): the grouped form of wgrad_rel_f32_kernel: 64 x 64 outputs per workgroup, rows in tiles of
// 16, s G X formed exactly and summed in fp64, W acc rounded ONCE to fp32.
#include "moe_gemm.hpp"

namespace {

typedef __attribute__((ext_vector_type(4))) short mw_s16x4;
typedef __attribute__((ext_vector_type(8))) short mw_s16x8;
typedef __attribute__((address_space(3))) mw_s16x4* mw_lds_s16x4_t;

constexpr int MW_TILE = 128;                      // output rows (n) and columns (k) of a workgroup's tile
constexpr int MW_TT = 64;                         // expert rows per staging tile
constexpr int MW_OPND = MW_TT * 256;              // bytes of one operand image
constexpr int MW_LDS = 2 * MW_OPND;
constexpr int MW_GATE_UP = 0, MW_DOWN = 1;        // (LRP_MOE_WGRAD_GATE_UP / _DOWN)

LRP_DEVICE uint32_t mw_off(int row, int ch) { return 256u * (uint32_t)row + 16u * (uint32_t)(ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

LRP_DEVICE bf16x8 mw_frag_tr(const char* img, uint32_t off0, uint32_t off1) {
    const mw_s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((mw_lds_s16x4_t)(img + off0));
    const mw_s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((mw_lds_s16x4_t)(img + off1));
    const mw_s16x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(bf16x8, v);
}

// W[e][n, k .. k + 3] as fp32: read as stored, or decoded from one scale byte and two code bytes (k is a multiple of 4, K of 128)
template <typename T, bool Q>
LRP_DEVICE void mw_weight4(const void* W, const uint8_t* scales, int64_t row, int K, int k, float* w) {
    if constexpr (Q) {
        const uint8_t* codes = reinterpret_cast<const uint8_t*>(W);
        const uint32_t word = *reinterpret_cast<const uint16_t*>(codes + row * (K >> 1) + (k >> 1));
        const uint32_t sc = scales[row * (K >> 5) + (k >> 5)];
        T v[8];
        mx_decode8(word, sc, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = (float)v[e];
    } else {
        const T* p = reinterpret_cast<const T*>(W) + row * K + k;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = (float)p[e];
    }
}

template <int MODE, bool Q>
__global__ __launch_bounds__(256) void moe_wgrad_bf16_kernel(const bf16_t* __restrict__ G, const bf16_t* __restrict__ X, const void* __restrict__ W,
                                                             const uint8_t* __restrict__ scales, const bf16_t* __restrict__ w,
                                                             const int* __restrict__ plan, float* __restrict__ out, int R, int kslots, int E,
                                                             int N, int K, int64_t ldg, int64_t ldx, int accumulate) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.y * MW_TILE, k0 = blockIdx.x * MW_TILE, ex = blockIdx.z;
    const PlanView P = plan_view(plan, R, E);
    const int M = P.cnt[ex], p0 = P.off[ex];
    const int wn = wave >> 1, wk = wave & 1;
    const int i16 = lane & 15, hi = lane >> 4, q = i16 >> 2, p = i16 & 3;
    float* oute = out + (int64_t)ex * N * K;
    if (M == 0) {                                                          // (uniform: the whole workgroup leaves here)
        if (accumulate) return;
#pragma unroll
        for (int jg = 0; jg < 4; ++jg) {
            const int n = n0 + 64 * wn + 16 * jg + i16;
            if (n >= N) continue;
#pragma unroll
            for (int jx = 0; jx < 4; ++jx) {
                const int k = k0 + 64 * wk + 16 * jx + 4 * hi;
                if (k < K) *reinterpret_cast<f32x4*>(oute + (int64_t)n * K + k) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
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
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t o = mw_off(srow + 16 * i, sch);
            u32x4 g = gr[i];
            if constexpr (MODE == MW_DOWN) {
                bf16x8 v = __builtin_bit_cast(bf16x8, g);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = (bf16_t)((float)v[e] * sv[i]);
                g = __builtin_bit_cast(u32x4, v);
            }
            *reinterpret_cast<u32x4*>(smem + o) = g;
            *reinterpret_cast<u32x4*>(smem + MW_OPND + o) = xr[i];
        }
    };
    f32x4 acc[4][4];                                                   // [k tile jx][n tile jg]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    resolve(0);
    load();
    resolve(MW_TT);
    for (int t0 = 0; t0 < M; t0 += MW_TT) {
        __syncthreads();                                               // the previous tile's fragment reads are done
        store();
        __syncthreads();
        if (t0 + MW_TT < M) {                                          // (uniform branch) in flight under the MFMAs below
            load();
            resolve(t0 + 2 * MW_TT);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int r0 = 32 * ks + 8 * hi + q, r1 = r0 + 4;
            bf16x8 fg[4], fx[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cg = 8 * wn + 2 * j + (p >> 1), cx = 8 * wk + 2 * j + (p >> 1);
                fg[j] = mw_frag_tr(smem, mw_off(r0, cg) + 8 * (p & 1), mw_off(r1, cg) + 8 * (p & 1));
                fx[j] = mw_frag_tr(smem + MW_OPND, mw_off(r0, cx) + 8 * (p & 1), mw_off(r1, cx) + 8 * (p & 1));
            }
#pragma unroll
            for (int jx = 0; jx < 4; ++jx)
#pragma unroll
                for (int jg = 0; jg < 4; ++jg) acc[jx][jg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fx[jx], fg[jg], acc[jx][jg], 0, 0, 0);
        }
    }
    // ---- epilogue: out[e][n, k .. k + 3] (+)= W[e][n, k .. k + 3] acc
#pragma unroll
    for (int jg = 0; jg < 4; ++jg) {
        const int n = n0 + 64 * wn + 16 * jg + i16;
        if (n >= N) continue;
        const int64_t wrow = (int64_t)ex * N + n;
#pragma unroll
        for (int jx = 0; jx < 4; ++jx) {
            const int k = k0 + 64 * wk + 16 * jx + 4 * hi;
            if (k >= K) continue;                                      // (K is a multiple of 8: k < K means k + 3 < K)
            float wv[4];
            mw_weight4<bf16_t, Q>(W, scales, wrow, K, k, wv);
            float* dst = oute + (int64_t)n * K + k;
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = wv[e] * acc[jx][jg][e];
            if (accumulate) {
                const f32x4 old = *reinterpret_cast<const f32x4*>(dst);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += old[e];
            }
            *reinterpret_cast<f32x4*>(dst) = v;
        }
    }
}

constexpr int MF_TILE = 64, MF_TT = 16;

template <int MODE, bool Q>
__global__ __launch_bounds__(256) void moe_wgrad_f32_kernel(const float* __restrict__ G, const float* __restrict__ X, const void* __restrict__ W,
                                                            const uint8_t* __restrict__ scales, const float* __restrict__ w,
                                                            const int* __restrict__ plan, float* __restrict__ out, int R, int kslots, int E,
                                                            int N, int K, int64_t ldg, int64_t ldx, int accumulate) {
    __shared__ float Gs[MF_TT][MF_TILE], Xs[MF_TT][MF_TILE], Ss[MF_TT];
    __shared__ int Gi[MF_TT], Xi[MF_TT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n0 = blockIdx.y * MF_TILE, k0 = blockIdx.x * MF_TILE, ex = blockIdx.z;
    const PlanView P = plan_view(plan, R, E);
    const int M = P.cnt[ex], p0 = P.off[ex];
    float* oute = out + (int64_t)ex * N * K;
    if (M == 0 && accumulate) return;                                  // (uniform)
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int t0 = 0; t0 < M; t0 += MF_TT) {
        __syncthreads();
        if (tid < MF_TT) {
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
        for (int tt = 0; tt < MF_TT; ++tt) {
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
                mw_weight4<float, true>(W, scales, wrow, K, k - b, w4);
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
    if (dtype != LRP_F32 && dtype != LRP_BF16) return LRP_EINVAL;
    if (mode != MW_GATE_UP && mode != MW_DOWN) return LRP_EINVAL;
    if (T < 1 || k < 1 || E < 1 || N < 1 || K < 1) return LRP_ESHAPE;
    if (E > MOE_EMAX || (int64_t)T * k >= (1ll << 30)) return LRP_ESHAPE;
    if (ldg < N || ldx < K) return LRP_ESHAPE;
    const int tile = dtype == LRP_BF16 ? MW_TILE : MF_TILE;
    if (((int64_t)N + tile - 1) / tile > 65535) return LRP_ESHAPE;
    if (dtype == LRP_BF16 && (N % 8 || K % 8)) return LRP_ESHAPE;          // 16-byte chunks of G and X rows: inside or outside as a whole
    if (quantised && K % 128) return LRP_ESHAPE;                           // rows of scale bytes on the 4-byte grid (lrp_hip_moe_mxfp4.h)
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
        const dim3 grid((unsigned)((K + MW_TILE - 1) / MW_TILE), (unsigned)((N + MW_TILE - 1) / MW_TILE), (unsigned)E);
        lrp_with_bool(mode == MW_DOWN, [&](auto DOWN) {
            constexpr int MODE = decltype(DOWN)::value ? MW_DOWN : MW_GATE_UP;
            hipLaunchKernelGGL((moe_wgrad_bf16_kernel<MODE, Q>), grid, dim3(256), MW_LDS, st, (const bf16_t*)G, (const bf16_t*)X, W, sc,
                               (const bf16_t*)w, plan, out, R, k, E, N, K, ldg, ldx, accumulate);
        });
    } else {
        const dim3 grid((unsigned)((K + MF_TILE - 1) / MF_TILE), (unsigned)((N + MF_TILE - 1) / MF_TILE), (unsigned)E);
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
