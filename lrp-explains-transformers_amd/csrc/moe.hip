// moe.hip -- routed experts of a sparse MoE layer (Qwen3-MoE's Qwen3MoeExperts) on grouped GEMMs, forward and LRP backward.
// ref: lxt/efficient/models/qwen3_moe.py:14-44 (experts_forward: per expert a gather, gate/up Linear, identity rule on act, uniform rule
// on the product, down Linear, routing-weight product, uniform rule, index_add).  See include/lrp_hip.h "MoE" and DESIGN.md section 9.
//
// One ROUTING PLAN per layer (three launches, no host sync, no atomics whose ORDER matters -- the per-chunk histograms use LDS atomics
// whose integer sums do not depend on order) groups the T k (token, slot) rows by expert, stably (token order inside an expert):
//   plan (int32): cnt[E] | off[E + 1] (exclusive scan) | toff[E + 1] (prefix of 128-row M tiles) | perm[R] (plan row -> t k + s) |
//                 inv[R] (t k + s -> plan row, -1 for a skipped slot) | hist[ceil(R / 256)][E] (scan workspace)
// Four grouped GEMMs walk the plan's tile list; no activation is ever copied into plan order -- the A rows of the gate/up forward and of the
// down-projection dgrad are GATHERED through perm in the staging loads, and the expert weights are read as stored (no second copy).
//
// Tile shape: 128 x 128 (M x N), 256 threads = 2 x 2 waves of 64 x 64.  With 128-512 rows per expert (one to four prompts of 2048 at
// 30B-A3B's 128 experts / top 8) a 256-row tile would be half empty at one prompt; 128 rows keep the tail waste to ~25 % there.
// Placement: work items are ordered expert-major (all M x N tiles of one expert are consecutive) and every XCD takes ONE contiguous eighth of
// the list (block b runs on XCD b % 8), so the tiles that read the same expert's weight panel run on one XCD and share its L2: an expert's
// 2 I H weight bytes come from HBM about once per direction instead of once per M tile.  The grid is persistent (<= 2 blocks per CU) and
// sized from the host-side upper bound ceil(R / 128) + E on M tiles; each block walks its XCD's range and binary-searches toff for the expert.
#include "moe_gemm.hpp"

namespace {

// ---- routing plan ------------------------------------------------------------------------------------------------------------------------
// 1: per-chunk expert histogram
__global__ __launch_bounds__(256) void moe_hist_kernel(const int64_t* __restrict__ idx, int* __restrict__ plan, int R, int E) {
    __shared__ int h[MOE_EMAX];
    for (int e = threadIdx.x; e < E; e += 256) h[e] = 0;
    __syncthreads();
    const int r = blockIdx.x * MOE_CH + threadIdx.x;
    if (r < R) {
        const int64_t e = idx[r];
        if (e >= 0 && e < E) atomicAdd(&h[e], 1);
    }
    __syncthreads();
    int* hist = plan_view(plan, R, E).hist + (int64_t)blockIdx.x * E;
    for (int e = threadIdx.x; e < E; e += 256) hist[e] = h[e];
}

// 2: one block -- per expert, the running count over chunks (hist becomes the exclusive per-chunk base), then the scans over experts
__global__ __launch_bounds__(1024) void moe_scan_kernel(int* __restrict__ plan, int R, int E) {
    PlanView v = plan_view(plan, R, E);
    int* cnt = plan;
    int* off = plan + E;
    int* toff = off + E + 1;
    const int nch = (R + MOE_CH - 1) / MOE_CH;
    for (int e = threadIdx.x; e < E; e += 1024) {
        int run = 0;
        for (int c = 0; c < nch; ++c) {
            int* hp = v.hist + (int64_t)c * E + e;
            const int s = *hp;
            *hp = run;
            run += s;
        }
        cnt[e] = run;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int o = 0, t = 0;
        for (int e = 0; e < E; ++e) {
            off[e] = o;
            toff[e] = t;
            o += cnt[e];
            t += (cnt[e] + MOE_BM - 1) / MOE_BM;
        }
        off[E] = o;
        toff[E] = t;
    }
}

// 3: stable scatter -- a row's place is off[e] + (rows of e in earlier chunks) + (rows of e earlier in this chunk)
__global__ __launch_bounds__(256) void moe_scatter_kernel(const int64_t* __restrict__ idx, int* __restrict__ plan, int R, int E) {
    __shared__ int es[MOE_CH];
    PlanView v = plan_view(plan, R, E);
    const int r = blockIdx.x * MOE_CH + threadIdx.x;
    int e = -1;
    if (r < R) {
        const int64_t e64 = idx[r];
        e = (e64 >= 0 && e64 < E) ? (int)e64 : -1;
    }
    es[threadIdx.x] = e;
    __syncthreads();
    if (r >= R) return;
    int* perm = const_cast<int*>(v.perm);
    int* inv = const_cast<int*>(v.inv);
    if (e < 0) {
        inv[r] = -1;
        return;
    }
    int rank = 0;
    for (int j = 0; j < (int)threadIdx.x; ++j) rank += (es[j] == e);
    const int p = v.off[e] + v.hist[(int64_t)blockIdx.x * E + e] + rank;
    perm[p] = r;
    inv[r] = p;
}

// out[t] = sum_s w[t, s] rows[inv[t k + s]] (w == nullptr: weight 1), slots in order, fp32 accumulate, one rounding
template <typename T>
__global__ __launch_bounds__(256) void moe_combine_kernel(const T* __restrict__ rows, const T* __restrict__ w, const int* __restrict__ plan,
                                                         T* __restrict__ out, int R, int k, int E, int H, int64_t ldr, int64_t ldo) {
    constexpr int V = 16 / (int)sizeof(T);
    const PlanView P = plan_view(plan, R, E);
    const int t = blockIdx.x;
    for (int c = threadIdx.x; c < H / V; c += blockDim.x) {
        float acc[V];
#pragma unroll
        for (int q = 0; q < V; ++q) acc[q] = 0.f;
        for (int s = 0; s < k; ++s) {
            const int p = P.inv[(int64_t)t * k + s];
            if (p < 0) continue;
            const float wv = w ? to_f32(w[(int64_t)t * k + s]) : 1.f;
            const Vec16<T> v = ld16(rows + (int64_t)p * ldr + c * V);
#pragma unroll
            for (int q = 0; q < V; ++q) acc[q] += wv * v.get(q);
        }
        Vec16<T> o;
#pragma unroll
        for (int q = 0; q < V; ++q) o.set(q, acc[q]);
        st16(out + (int64_t)t * ldo + c * V, o);
    }
}

// G_w[t, s] = 1/2 sum over column tiles of the partials (fixed order); 0 for a skipped slot
template <typename T>
__global__ __launch_bounds__(256) void moe_gw_kernel(const float* __restrict__ gwp, const int* __restrict__ plan, T* __restrict__ gw,
                                                    int R, int E, int ntn) {
    const PlanView P = plan_view(plan, R, E);
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const int p = P.inv[r];
    float s = 0.f;
    if (p >= 0)
        for (int n = 0; n < ntn; ++n) s += gwp[(int64_t)p * ntn + n];
    gw[r] = from_f32<T>(0.5f * s);
}

}  // namespace

extern "C" int64_t lrp_moe_plan_ints(int T, int k, int E) {
    if (T < 1 || k < 1 || E < 1 || E > MOE_EMAX || (int64_t)T * k >= (1ll << 30)) return LRP_ESHAPE;
    return plan_ints(T * k, E);
}

extern "C" int lrp_moe_plan(const void* idx, int* plan, int T, int k, int E, void* stream) {
    if (!idx || !plan || T < 1 || k < 1 || E < 1) return LRP_EINVAL;
    if (E > MOE_EMAX || (int64_t)T * k >= (1ll << 30)) return LRP_ESHAPE;
    if ((reinterpret_cast<uintptr_t>(idx) & 7) || (reinterpret_cast<uintptr_t>(plan) & 3)) return LRP_EALIGN;
    const int R = T * k, nch = (R + MOE_CH - 1) / MOE_CH;
    hipStream_t st = (hipStream_t)stream;
    const int64_t* ix = reinterpret_cast<const int64_t*>(idx);
    hipLaunchKernelGGL(moe_hist_kernel, dim3(nch), dim3(256), 0, st, ix, plan, R, E);
    hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(1024), 0, st, plan, R, E);
    hipLaunchKernelGGL(moe_scatter_kernel, dim3(nch), dim3(256), 0, st, ix, plan, R, E);
    return lrp_check_launch();
}

extern "C" int lrp_moe_gate_up_fwd(const void* x, const void* Wgu, const int* plan, void* coef, void* m, int T, int k, int E, int H, int I,
                                   int64_t ldx, int64_t ldcoef, int64_t ldm, int act, int dtype, void* stream) {
    MOE_CHECK(check_dims(T, k, E, H, I, dtype));
    if (!plan) return LRP_EINVAL;
    if (act != LRP_ACT_SILU && act != LRP_ACT_GELU_TANH) return LRP_EINVAL;
    MOE_CHECK(check_mat(x, ldx, H, dtype));
    MOE_CHECK(check_mat(Wgu, H, H, dtype));
    MOE_CHECK(check_mat(coef, ldcoef, 2 * (int64_t)I, dtype));
    MOE_CHECK(check_mat(m, ldm, I, dtype));
    MoeGemmArgs a = base_args(plan, T, k, E, H, I);
    a.A = x; a.lda = ldx;
    a.B = Wgu; a.sB = 2 * (int64_t)I * H; a.ldb = H;
    a.C = m; a.ldc = ldm; a.coef = coef; a.ldcoef = ldcoef;
    a.N = 2 * I; a.K = H;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == LRP_BF16)
        return act == LRP_ACT_SILU ? launch_gemm<bf16_t, A_GATHER, B_NT_GU, EP_COEF, LRP_ACT_SILU>(a, st)
                                   : launch_gemm<bf16_t, A_GATHER, B_NT_GU, EP_COEF, LRP_ACT_GELU_TANH>(a, st);
    return act == LRP_ACT_SILU ? launch_gemm<float, A_GATHER, B_NT_GU, EP_COEF, LRP_ACT_SILU>(a, st)
                               : launch_gemm<float, A_GATHER, B_NT_GU, EP_COEF, LRP_ACT_GELU_TANH>(a, st);
}

extern "C" int lrp_moe_down_fwd(const void* m, const void* Wd, const int* plan, void* y, int T, int k, int E, int H, int I, int64_t ldm,
                                int64_t ldy, int dtype, void* stream) {
    MOE_CHECK(check_dims(T, k, E, H, I, dtype));
    if (!plan) return LRP_EINVAL;
    MOE_CHECK(check_mat(m, ldm, I, dtype));
    MOE_CHECK(check_mat(Wd, I, I, dtype));
    MOE_CHECK(check_mat(y, ldy, H, dtype));
    MoeGemmArgs a = base_args(plan, T, k, E, H, I);
    a.A = m; a.lda = ldm;
    a.B = Wd; a.sB = (int64_t)H * I; a.ldb = I;
    a.C = y; a.ldc = ldy;
    a.N = H; a.K = I;
    hipStream_t st = (hipStream_t)stream;
    return dtype == LRP_BF16 ? launch_gemm<bf16_t, A_ROWS, B_NT, EP_STORE, 0>(a, st) : launch_gemm<float, A_ROWS, B_NT, EP_STORE, 0>(a, st);
}

extern "C" int lrp_moe_combine(const void* rows, const void* w, const int* plan, void* out, int T, int k, int E, int H, int64_t ldr,
                               int64_t ldo, int dtype, void* stream) {
    if (T < 1 || k < 1 || E < 1 || H < 1 || !plan || (dtype != LRP_F32 && dtype != LRP_BF16)) return LRP_EINVAL;
    if (E > MOE_EMAX || (int64_t)T * k >= (1ll << 30)) return LRP_ESHAPE;
    if ((H * esz(dtype)) % 16 != 0) return LRP_EALIGN;
    MOE_CHECK(check_mat(rows, ldr, H, dtype));
    MOE_CHECK(check_mat(out, ldo, H, dtype));
    if (w && (reinterpret_cast<uintptr_t>(w) % esz(dtype))) return LRP_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int R = T * k;
    if (dtype == LRP_BF16)
        hipLaunchKernelGGL(moe_combine_kernel<bf16_t>, dim3(T), dim3(256), 0, st, (const bf16_t*)rows, (const bf16_t*)w, plan, (bf16_t*)out, R,
                           k, E, H, ldr, ldo);
    else
        hipLaunchKernelGGL(moe_combine_kernel<float>, dim3(T), dim3(256), 0, st, (const float*)rows, (const float*)w, plan, (float*)out, R, k,
                           E, H, ldr, ldo);
    return lrp_check_launch();
}

extern "C" int lrp_moe_down_dgrad(const void* G, const void* Wd, const void* coef, const void* m, const void* w, const int* plan, void* Agu,
                                  float* gw_part, int T, int k, int E, int H, int I, int64_t ldg, int64_t ldcoef, int64_t ldm,
                                  int64_t ldagu, int dtype, void* stream) {
    MOE_CHECK(check_dims(T, k, E, H, I, dtype));
    if (!plan || !w || !gw_part) return LRP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(w) % esz(dtype)) || (reinterpret_cast<uintptr_t>(gw_part) & 3)) return LRP_EALIGN;
    MOE_CHECK(check_mat(G, ldg, H, dtype));
    MOE_CHECK(check_mat(Wd, I, I, dtype));
    MOE_CHECK(check_mat(coef, ldcoef, 2 * (int64_t)I, dtype));
    MOE_CHECK(check_mat(m, ldm, I, dtype));
    MOE_CHECK(check_mat(Agu, ldagu, 2 * (int64_t)I, dtype));
    MoeGemmArgs a = base_args(plan, T, k, E, H, I);
    a.A = G; a.lda = ldg;
    a.B = Wd; a.sB = (int64_t)H * I; a.ldb = I;
    a.C = Agu; a.ldc = ldagu; a.coef = const_cast<void*>(coef); a.ldcoef = ldcoef;
    a.m = m; a.ldm = ldm; a.w = w; a.gwp = gw_part;
    a.N = I; a.K = H;
    hipStream_t st = (hipStream_t)stream;
    return dtype == LRP_BF16 ? launch_gemm<bf16_t, A_GATHER, B_NN, EP_DGRAD, 0>(a, st)
                             : launch_gemm<float, A_GATHER, B_NN, EP_DGRAD, 0>(a, st);
}

extern "C" int lrp_moe_gw_reduce(const float* gw_part, const int* plan, void* gw, int T, int k, int E, int I, int dtype, void* stream) {
    if (!gw_part || !plan || !gw || T < 1 || k < 1 || E < 1 || I < 1 || (dtype != LRP_F32 && dtype != LRP_BF16)) return LRP_EINVAL;
    if (E > MOE_EMAX || (int64_t)T * k >= (1ll << 30) || I % MOE_BN != 0) return LRP_ESHAPE;
    if ((reinterpret_cast<uintptr_t>(gw) % esz(dtype)) || (reinterpret_cast<uintptr_t>(gw_part) & 3)) return LRP_EALIGN;
    const int R = T * k;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == LRP_BF16)
        hipLaunchKernelGGL(moe_gw_kernel<bf16_t>, dim3((R + 255) / 256), dim3(256), 0, st, gw_part, plan, (bf16_t*)gw, R, E, I / MOE_BN);
    else
        hipLaunchKernelGGL(moe_gw_kernel<float>, dim3((R + 255) / 256), dim3(256), 0, st, gw_part, plan, (float*)gw, R, E, I / MOE_BN);
    return lrp_check_launch();
}

extern "C" int lrp_moe_gate_up_dgrad(const void* Agu, const void* Wgu, const int* plan, void* gx_rows, int T, int k, int E, int H, int I,
                                     int64_t ldagu, int64_t ldgx, int dtype, void* stream) {
    MOE_CHECK(check_dims(T, k, E, H, I, dtype));
    if (!plan) return LRP_EINVAL;
    MOE_CHECK(check_mat(Agu, ldagu, 2 * (int64_t)I, dtype));
    MOE_CHECK(check_mat(Wgu, H, H, dtype));
    MOE_CHECK(check_mat(gx_rows, ldgx, H, dtype));
    MoeGemmArgs a = base_args(plan, T, k, E, H, I);
    a.A = Agu; a.lda = ldagu;
    a.B = Wgu; a.sB = 2 * (int64_t)I * H; a.ldb = H;
    a.C = gx_rows; a.ldc = ldgx;
    a.N = H; a.K = 2 * I;
    hipStream_t st = (hipStream_t)stream;
    return dtype == LRP_BF16 ? launch_gemm<bf16_t, A_ROWS, B_NN, EP_STORE, 0>(a, st) : launch_gemm<float, A_ROWS, B_NN, EP_STORE, 0>(a, st);
}
