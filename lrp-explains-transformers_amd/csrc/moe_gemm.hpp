// moe_gemm.hpp -- the grouped expert GEMM of csrc/moe.hip (tile walk, staging, three epilogues) and its host-side checks, shared by the
// translation units that instantiate it: moe.hip (B read as stored, in the activation dtype) and moe_mxfp4.hip (QB: B held as MXFP4 codes +
// scales, decoded between the global load and the LDS write; include/lrp_hip_moe_mxfp4.h).  Plan layout and placement: see moe.hip.
#pragma once
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

// ---- grouped GEMM ------------------------------------------------------------------------------------------------------------------------
enum { A_ROWS = 0, A_GATHER = 1 };            // A row of plan row p: row p itself, or row perm[p] / k (its token) of a [T, K] tensor
enum { B_NT = 0, B_NT_GU = 1, B_NN = 2 };     // B[e] as [N, K] (K-contiguous), the same with the gate/up interleave, or as [K, N]
enum { EP_STORE = 0, EP_COEF = 1, EP_DGRAD = 2 };

struct MoeGemmArgs {
    const void* A;
    int64_t lda;
    const void* B;         // QB: the e2m1 codes [E, rows, ldb / 2] bytes
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
    const void* Bsc;       // QB: the e8m0 scales [E, rows, ldb / 32] bytes (last: the fields above keep their kernarg offsets)
};

// 16-byte load through an address_space(1) pointer: a generic pointer walked in the K loop becomes flat_load, which also counts on lgkmcnt --
// the ds_read waits of the MFMA phase would then drain the next stage's prefetch
typedef const __attribute__((address_space(1))) u32x4* gvec_ptr_t;
LRP_DEVICE u32x4 gload16(const void* p) { return *(gvec_ptr_t)p; }

// ---- QB: B held as MXFP4 (include/lrp_hip_mxfp4.h applied to [E rows, ldb]) ------------------------------------------------------------------
// Blocks of 32 run along the STORED row: along K in the NT forms, along N in B_NN.  Per stage a thread owns 8 MxStage<T>::NQ consecutive elements of
// one stored row -- a whole block in bf16 (128 x 64 NT / 64 x 128 NN elements = 256 blocks per stage), half a block in fp32 (128 blocks) --
// loads their codes with ONE vector load (16 / 8 bytes) and the block's scale byte, and decodes between the load's arrival and the LDS
// write: the values land in LDS exactly where the unquantised staging puts them, so every accumulator receives the same MFMAs on the same
// operand bits in the same order (each decoded value is exact in bf16 and fp32): bit-identical to lrp_mxfp4_dequant + the plain kernel.
typedef const __attribute__((address_space(1))) u32x2* gvec8_ptr_t;
typedef const __attribute__((address_space(1))) uint8_t* gbyte_ptr_t;
template <typename T> struct MxStage;                  // NQ: 32-bit code words (8 elements each) a thread decodes per stage
template <> struct MxStage<bf16_t> {
    static constexpr int NQ = 4;
    typedef u32x4 codes_t;
    static LRP_DEVICE codes_t load(const uint8_t* p) { return *(gvec_ptr_t)p; }
};
template <> struct MxStage<float> {
    static constexpr int NQ = 2;
    typedef u32x2 codes_t;
    static LRP_DEVICE codes_t load(const uint8_t* p) { return *(gvec8_ptr_t)p; }
};

// (the decode itself: mx_decode8 of common.hpp)

template <typename T, int AMODE, int BMODE, int EPI, int ACT, bool QB = false>
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
        // QB: one piece of EPT elements of one stored row per thread and stage
        constexpr int NQ = MxStage<T>::NQ, EPT = 8 * NQ;
        constexpr int PPR = (BMODE == B_NN) ? MOE_BN / EPT : KE / EPT;      // pieces per stored row in a stage: NN 4 / 8, NT 2
        const int qrow = tid / PPR, qpart = tid % PPR;                      // NT: tile row (N), piece along K; NN: K row, piece along N
        const uint8_t* qc = nullptr;
        const uint8_t* qs = nullptr;
        if constexpr (QB) {
            int64_t srow, col;                                              // the stored row and the piece's first column
            if constexpr (BMODE == B_NN) {
                srow = qrow;
                col = (int64_t)nt * MOE_BN + qpart * EPT;
            } else {
                if constexpr (BMODE == B_NT_GU) {
                    const int jb = nt * 64 + (qrow >> 5) * 16 + (qrow & 15);          // (the interleave of the plain staging below)
                    srow = ((qrow >> 4) & 1) ? (int64_t)g.I + jb : (int64_t)jb;
                } else {
                    srow = (int64_t)nt * MOE_BN + qrow;
                }
                col = qpart * EPT;
            }
            const int64_t el = (int64_t)e * g.sB + srow * g.ldb + col;
            qc = reinterpret_cast<const uint8_t*>(g.B) + el / 2;
            qs = reinterpret_cast<const uint8_t*>(g.Bsc) + el / 32;
        }
        const int64_t qstep = (BMODE == B_NN) ? (int64_t)KE * g.ldb : KE;   // elements per stage along the walk
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (tid >> 3) + 32 * i;
            const int p = p0 + min(row, nrows - 1);                 // rows past the expert's count re-read its last row (results dropped)
            const int64_t src = (AMODE == A_GATHER) ? (int64_t)(P.perm[p] / g.k) : (int64_t)p;
            ap[i] = A + src * g.lda + kc * V;
            if constexpr (QB) {
                bp[i] = nullptr;
            } else if constexpr (BMODE == B_NN) {
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
        typename MxStage<T>::codes_t rq = {};
        uint32_t rE = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ra[i] = gload16(ap[i]);
            if constexpr (!QB) rb[i] = gload16(bp[i]);
        }
        if constexpr (QB) {
            rq = MxStage<T>::load(qc);
            rE = *(gbyte_ptr_t)qs;
        }
        for (int k0 = 0; k0 < g.K; k0 += KE) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = (tid >> 3) + 32 * i;
                *reinterpret_cast<u32x4*>(As + row * MOE_LDSP + kc * 16) = ra[i];
                if constexpr (QB) {
                } else if constexpr (BMODE == B_NN) {
                    const int c = tid + 256 * i;
                    const int kr = c / (MOE_BN / V), nc = c % (MOE_BN / V);
                    const T* vals = reinterpret_cast<const T*>(&rb[i]);
#pragma unroll
                    for (int q = 0; q < V; ++q) *reinterpret_cast<T*>(Bs + (nc * V + q) * MOE_LDSP + kr * (int)sizeof(T)) = vals[q];
                } else {
                    *reinterpret_cast<u32x4*>(Bs + row * MOE_LDSP + kc * 16) = rb[i];
                }
            }
            if constexpr (QB) {
                __attribute__((aligned(16))) T vals[EPT];
#pragma unroll
                for (int q = 0; q < NQ; ++q) mx_decode8(rq[q], rE, vals + 8 * q);
                if constexpr (BMODE == B_NN) {
#pragma unroll
                    for (int q = 0; q < EPT; ++q) *reinterpret_cast<T*>(Bs + (qpart * EPT + q) * MOE_LDSP + qrow * (int)sizeof(T)) = vals[q];
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)          // EPT sizeof(T) = 64 bytes: four 16-byte stores
                        *reinterpret_cast<u32x4*>(Bs + qrow * MOE_LDSP + qpart * 64 + q * 16) = reinterpret_cast<const u32x4*>(vals)[q];
                }
            }
            __syncthreads();
            if (k0 + KE < g.K) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ap[i] += KE;
                    ra[i] = gload16(ap[i]);
                    if constexpr (!QB) {
                        bp[i] += bstep;
                        rb[i] = gload16(bp[i]);
                    }
                }
                if constexpr (QB) {
                    qc += qstep / 2;
                    qs += qstep / 32;
                    rq = MxStage<T>::load(qc);
                    rE = *(gbyte_ptr_t)qs;
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

template <typename T, int AMODE, int BMODE, int EPI, int ACT, bool QB = false>
int launch_gemm(const MoeGemmArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((moe_gemm_kernel<T, AMODE, BMODE, EPI, ACT, QB>), dim3(grid_for(a.R, a.E, a.N)), dim3(256), 0, st, a);
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
