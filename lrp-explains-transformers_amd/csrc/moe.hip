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
#include <algorithm>

#include "common.hpp"

namespace {

constexpr int MOE_BM = 128, MOE_BN = 128;
constexpr int MOE_KB = 128;               // bytes of K per LDS stage (two 64-byte MFMA macro steps)
constexpr int MOE_LDSP = MOE_KB + 16;     // LDS row pitch in bytes (+16: rows 0..15 of a fragment read do not share a bank group)
constexpr int MOE_CH = 256;               // plan rows per histogram chunk
constexpr int MOE_EMAX = 1024;

struct PlanView {
    const int *cnt, *off, *toff, *perm, *inv;
    int* hist;
};
__host__ __device__ inline PlanView plan_view(const int* p, int R, int E) {
    PlanView v;
    v.cnt = p;
    v.off = p + E;
    v.toff = v.off + E + 1;
    v.perm = v.toff + E + 1;
    v.inv = v.perm + R;
    v.hist = const_cast<int*>(v.inv + R);
    return v;
}
inline int64_t plan_ints(int R, int E) { return 3 * (int64_t)E + 2 + 2 * (int64_t)R + (int64_t)((R + MOE_CH - 1) / MOE_CH) * E; }

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

// ---- grouped GEMM ------------------------------------------------------------------------------------------------------------------------
enum { A_ROWS = 0, A_GATHER = 1 };            // A row of plan row p: row p itself, or row perm[p] / k (its token) of a [T, K] tensor
enum { B_NT = 0, B_NT_GU = 1, B_NN = 2 };     // B[e] as [N, K] (K-contiguous), the same with the gate/up interleave, or as [K, N]
enum { EP_STORE = 0, EP_COEF = 1, EP_DGRAD = 2 };

struct MoeGemmArgs {
    const void* A;
    int64_t lda;
    const void* B;
    int64_t sB, ldb;       // expert stride, row pitch (elements)
    void* C;
    int64_t ldc;           // EP_STORE: out rows; EP_COEF: m; EP_DGRAD: Agu
    void* coef;
    int64_t ldcoef;        // EP_COEF writes, EP_DGRAD reads [R, 2 I]: cg at column j, cu at column I + j
    const void* m;
    int64_t ldm;           // EP_DGRAD: the stored m (for the routing-weight partials)
    const void* w;         // EP_DGRAD: routing weights [T, k]
    float* gwp;            // EP_DGRAD: partials [R][N / 128]
    const int* plan;
    int R, k, E, N, K, I;
};

// 16-byte load through an address_space(1) pointer: a generic pointer walked in the K loop becomes flat_load, which also counts on lgkmcnt --
// the ds_read waits of the MFMA phase would then drain the next stage's prefetch
typedef const __attribute__((address_space(1))) u32x4* gvec_ptr_t;
LRP_DEVICE u32x4 gload16(const void* p) { return *(gvec_ptr_t)p; }

template <typename T, int AMODE, int BMODE, int EPI, int ACT>
__global__ __launch_bounds__(256) void moe_gemm_kernel(MoeGemmArgs g) {
    __shared__ __attribute__((aligned(16))) char As[MOE_BM * MOE_LDSP];
    __shared__ __attribute__((aligned(16))) char Bs[MOE_BN * MOE_LDSP];
    constexpr int V = 16 / (int)sizeof(T);         // elements per 16-byte chunk
    constexpr int KE = MOE_KB / (int)sizeof(T);    // K elements per stage
    typedef typename Mma16<T>::frag frag;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const PlanView P = plan_view(g.plan, g.R, g.E);
    const int ntn = g.N / MOE_BN;
    const int total = P.toff[g.E] * ntn;
    const int xcd = blockIdx.x & 7, per = gridDim.x >> 3;
    const int lo = (int)((int64_t)total * xcd / 8), hi = (int)((int64_t)total * (xcd + 1) / 8);
    const T* A = reinterpret_cast<const T*>(g.A);
    const T* B = reinterpret_cast<const T*>(g.B);

    for (int wi = lo + (int)(blockIdx.x >> 3); wi < hi; wi += per) {
        const int mtg = wi / ntn, nt = wi - mtg * ntn;
        int a = 0, b = g.E;                          // toff[a] <= mtg < toff[b]
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (P.toff[mid] <= mtg) a = mid;
            else b = mid;
        }
        const int e = a, mt = mtg - P.toff[e];
        const int p0 = P.off[e] + mt * MOE_BM;
        const int nrows = min(MOE_BM, P.cnt[e] - mt * MOE_BM);

        // staging: chunk c = tid + 256 i (i < 4) of the 128 x 128-byte A tile is row c / 8, 16-byte column c % 8 -- a lane's rows (and so
        // its gathered source rows) are fixed over the K loop
        const T* ap[4];
        const T* bp[4];
        const int kc = tid & 7;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (tid >> 3) + 32 * i;
            const int p = p0 + min(row, nrows - 1);                 // rows past the expert's count re-read its last row (results dropped)
            const int64_t src = (AMODE == A_GATHER) ? (int64_t)(P.perm[p] / g.k) : (int64_t)p;
            ap[i] = A + src * g.lda + kc * V;
            if constexpr (BMODE == B_NN) {
                const int c = tid + 256 * i;                        // [K, N]: 16-byte chunk of N at K row c / (128 / V)
                const int kr = c / (MOE_BN / V), nc = c % (MOE_BN / V);
                bp[i] = B + (int64_t)e * g.sB + (int64_t)kr * g.ldb + (int64_t)nt * MOE_BN + nc * V;
            } else {
                int64_t nrow;
                if constexpr (BMODE == B_NT_GU) {
                    // tile columns in 16-blocks [gate 16 | up 16] x 4: the pair of 16 x 16 MFMA tiles ni = 2q, 2q + 1 of a wave holds gate and
                    // up of the SAME intermediate indices in the same lanes (the epilogue's m = act(g) u needs no exchange)
                    const int jb = nt * 64 + (row >> 5) * 16 + (row & 15);
                    nrow = ((row >> 4) & 1) ? (int64_t)g.I + jb : (int64_t)jb;
                } else {
                    nrow = (int64_t)nt * MOE_BN + row;
                }
                bp[i] = B + (int64_t)e * g.sB + nrow * g.ldb + kc * V;
            }
        }
        const int64_t bstep = (BMODE == B_NN) ? (int64_t)KE * g.ldb : KE;

        f32x4 acc[4][4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

        u32x4 ra[4], rb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ra[i] = gload16(ap[i]);
            rb[i] = gload16(bp[i]);
        }
        for (int k0 = 0; k0 < g.K; k0 += KE) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = (tid >> 3) + 32 * i;
                *reinterpret_cast<u32x4*>(As + row * MOE_LDSP + kc * 16) = ra[i];
                if constexpr (BMODE == B_NN) {
                    const int c = tid + 256 * i;
                    const int kr = c / (MOE_BN / V), nc = c % (MOE_BN / V);
                    const T* vals = reinterpret_cast<const T*>(&rb[i]);
#pragma unroll
                    for (int q = 0; q < V; ++q) *reinterpret_cast<T*>(Bs + (nc * V + q) * MOE_LDSP + kr * (int)sizeof(T)) = vals[q];
                } else {
                    *reinterpret_cast<u32x4*>(Bs + row * MOE_LDSP + kc * 16) = rb[i];
                }
            }
            __syncthreads();
            if (k0 + KE < g.K) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ap[i] += KE;
                    bp[i] += bstep;
                    ra[i] = gload16(ap[i]);
                    rb[i] = gload16(bp[i]);
                }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int ko = s * 64 + (lane >> 4) * 16;
                frag fa[4], fb[4];
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) fa[mi] = *reinterpret_cast<const frag*>(As + (wm * 64 + mi * 16 + (lane & 15)) * MOE_LDSP + ko);
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) fb[ni] = *reinterpret_cast<const frag*>(Bs + (wn * 64 + ni * 16 + (lane & 15)) * MOE_LDSP + ko);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = Mma16<T>::mma(fa[mi], fb[ni], acc[mi][ni]);
            }
        }

        // ---- epilogue: lane holds D[i = wm 64 + mi 16 + (lane >> 4) 4 + r][c = wn 64 + ni 16 + (lane & 15)]
        if constexpr (EPI == EP_STORE) {
            T* C = reinterpret_cast<T*>(g.C);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = wm * 64 + mi * 16 + (lane >> 4) * 4 + r;
                    if (i >= nrows) continue;
                    T* crow = C + (int64_t)(p0 + i) * g.ldc + (int64_t)nt * MOE_BN + wn * 64 + (lane & 15);
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) crow[ni * 16] = from_f32<T>(acc[mi][ni][r]);
                }
        } else if constexpr (EPI == EP_COEF) {
            T* M = reinterpret_cast<T*>(g.C);
            T* CO = reinterpret_cast<T*>(g.coef);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = wm * 64 + mi * 16 + (lane >> 4) * 4 + r;
                    if (i >= nrows) continue;
                    const int64_t p = p0 + i;
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const int j = nt * 64 + wn * 32 + q * 16 + (lane & 15);
                        const float gg = acc[mi][2 * q][r], uu = acc[mi][2 * q + 1][r];
                        float mv, cg, cu;
                        if constexpr (sizeof(T) == 2) {
                            gated_coef<true, ACT>(gg, uu, 1e-10f, 0.f, mv, cg, cu);
                        } else {
                            // fp32 parity path: the exact forms of lrp_gated_act_fwd / _bwd
                            const float y = act_apply(gg, ACT), den = gg + 1e-10f;
                            mv = y * uu;
                            cg = (den == 0.f) ? 0.f : 0.5f * uu * (y / den);
                            cu = 0.5f * y;
                        }
                        M[p * g.ldc + j] = from_f32<T>(mv);
                        CO[p * g.ldcoef + j] = from_f32<T>(cg);
                        CO[p * g.ldcoef + g.I + j] = from_f32<T>(cu);
                    }
                }
        } else {
            // down-projection dgrad D = G[t] Wd[e] (unscaled).  Agu = 1/2 w D {cg | cu} in HF's [gate | up] order; the routing-weight
            // partial sum_c m[p][c] D[p][c] over this tile's 128 columns (= sum_j y_j G_j restricted to them), reduced in a fixed order
            T* AG = reinterpret_cast<T*>(g.C);
            const T* CO = reinterpret_cast<const T*>(g.coef);
            const T* Mv = reinterpret_cast<const T*>(g.m);
            const T* W = reinterpret_cast<const T*>(g.w);
            float part[4][4];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = wm * 64 + mi * 16 + (lane >> 4) * 4 + r;
                    const int64_t p = p0 + min(i, nrows - 1);
                    const float hw = 0.5f * to_f32(W[P.perm[p]]);
                    float s = 0.f;
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) {
                        const int j = nt * MOE_BN + wn * 64 + ni * 16 + (lane & 15);
                        const float d = acc[mi][ni][r];
                        s += to_f32(Mv[p * g.ldm + j]) * d;
                        if (i < nrows) {
                            const float gm = hw * d;
                            AG[p * g.ldc + j] = from_f32<T>(gm * to_f32(CO[p * g.ldcoef + j]));
                            AG[p * g.ldc + g.I + j] = from_f32<T>(gm * to_f32(CO[p * g.ldcoef + g.I + j]));
                        }
                    }
                    part[mi][r] = s;
                }
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float s = part[mi][r];
                    s += __shfl_xor(s, 1, 64);
                    s += __shfl_xor(s, 2, 64);
                    s += __shfl_xor(s, 4, 64);
                    s += __shfl_xor(s, 8, 64);
                    part[mi][r] = s;
                }
            __syncthreads();                                    // the K loop's last LDS reads are done: As is free
            float* red = reinterpret_cast<float*>(As);          // [128 rows][2 column halves]
            if ((lane & 15) == 0) {
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int r = 0; r < 4; ++r) red[(wm * 64 + mi * 16 + (lane >> 4) * 4 + r) * 2 + wn] = part[mi][r];
            }
            __syncthreads();
            if (tid < nrows) g.gwp[(int64_t)(p0 + tid) * ntn + nt] = red[tid * 2] + red[tid * 2 + 1];
        }
        __syncthreads();                                        // LDS reuse by the next work item
    }
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

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int esz(int dtype) { return dtype == LRP_F32 ? 4 : 2; }

// common checks; returns LRP_OK or the error code
int check_dims(int T, int k, int E, int H, int I, int dtype) {
    if (T < 1 || k < 1 || E < 1 || H < 1 || I < 1) return LRP_EINVAL;
    if (dtype != LRP_F32 && dtype != LRP_BF16) return LRP_EINVAL;
    if (E > MOE_EMAX) return LRP_ESHAPE;
    if ((int64_t)T * k >= (1ll << 30)) return LRP_ESHAPE;
    if (H % MOE_BN != 0 || I % MOE_BN != 0) return LRP_ESHAPE;
    return LRP_OK;
}
// an operand of `cols` columns with row pitch ld, read or written with 16-byte vectors
int check_mat(const void* p, int64_t ld, int64_t cols, int dtype) {
    if (!p) return LRP_EINVAL;
    if (ld < cols) return LRP_ESHAPE;
    if (!al16(p) || (ld * esz(dtype)) % 16 != 0) return LRP_EALIGN;
    return LRP_OK;
}
#define MOE_CHECK(x)                     \
    do {                                 \
        const int rc_ = (x);             \
        if (rc_ != LRP_OK) return rc_;   \
    } while (0)

int grid_for(int R, int E, int N) {
    const int64_t bound = ((int64_t)(R + MOE_BM - 1) / MOE_BM + E) * (N / MOE_BN);
    int64_t g = std::min<int64_t>(bound, 2 * (int64_t)lrp_num_cus());
    g = (g + 7) / 8 * 8;
    return (int)std::max<int64_t>(g, 8);
}

template <typename T, int AMODE, int BMODE, int EPI, int ACT>
int launch_gemm(const MoeGemmArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((moe_gemm_kernel<T, AMODE, BMODE, EPI, ACT>), dim3(grid_for(a.R, a.E, a.N)), dim3(256), 0, st, a);
    return lrp_check_launch();
}

MoeGemmArgs base_args(const int* plan, int T, int k, int E, int H, int I) {
    MoeGemmArgs a = {};
    a.plan = plan;
    a.R = T * k;
    a.k = k;
    a.E = E;
    a.I = I;
    (void)H;
    return a;
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
