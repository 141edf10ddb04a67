// attention_cp.hip -- the attention backward of the CP-LRP rule (ref lxt/efficient/patches.py:228-280): q and k are detached, so of the four
// contractions of the attention backward two remain -- S = Q K^T recomputed and dV = P^T G -- and there is no dQ, no dK, no D.
//
//   dv[b, j, hk, :] = sum_{h in group hk} sum_{i >= max(j, q_begin)} P_h[i, j] G[b, i, h, :],   P_h[i, j] = exp(scale q_h[i].k_hk[j] - lse[b, h, i])
//
// One workgroup owns (b, kv head, key block) and walks the group's query heads in ascending order with the dV^T accumulators in registers:
// the GQA sum needs no dv_h [M, Hq d] round trip, no reduce pass and no atomics, and its order is fixed.  Row side = keys (K fragments in
// registers, loaded once per workgroup -- every query head of the group scores against the same K rows), column side = the queries of one
// head after the other, streamed through LDS.
//   bf16, d in {64, 96, 128}: dkv_kernel<false, DH, IV> of attention32.hip without the Gho V^T contraction, the dS path, the dK accumulators
//   and the V block (32x32x16 MFMAs, G^T read out of the row-major G tile with ds_read_b64_tr_b16);
//   fp32, d in {16, 32, 64, 128}: attn_bwd_dkv_kernel<float, D> of attention.hip likewise (16x16x4 MFMAs, G^T from the head-transposed copy).
#include "attention_tiles.hpp"
#include "attention32_tiles.hpp"

namespace {

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- fp32: 4 waves x 16 keys; Q tile [32 queries][D] row-major and G^T tile [D][32 queries] per step ---------------------------------------
template <int D>
__global__ __launch_bounds__(ANT, 2) void attn_bwd_dv_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ gt, const float* __restrict__ lse,
    float* __restrict__ dv, int S, int Hq, int Hkv, int64_t ldq, int64_t ldk, int64_t ldt, int64_t lddv, float scale, int q_begin,
    const int* __restrict__ row_lo, const int* __restrict__ row_hi) {
    typedef float T;
    typedef AT<T> A;
    typedef typename Mma16<T>::frag frag_t;
    constexpr int SZ = A::SZ, CT = A::CT, NC16 = A::NC16, NDC = D * SZ / 64, ND16 = D / 16;
    constexpr int KP = D * SZ;
    constexpr int BK = 64;
    static_assert(NC16 == 2, "one register-resident P operand per 16-query sub-tile");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sQ = smem;                       // [CT][KP]
    char* sGt = sQ + CT * KP;              // [D][128]

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
    const int b = blockIdx.z, hk = blockIdx.y, rep = Hq / Hkv;
    const int k0 = blockIdx.x * BK, ki = k0 + wave * 16 + (lane & 15);

    frag_t kf[NDC];
    load_row_frags<T, D>(kf, k + (int64_t)b * S * ldk + (int64_t)hk * D, ldk, ki, S, lane);
    f32x4 dvacc[ND16];
#pragma unroll
    for (int dt = 0; dt < ND16; ++dt) dvacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int qbeg = (max(k0, q_begin) / CT) * CT;       // causal: no query before the block's first key sees it; none below q_begin counts
    for (int hh = 0; hh < rep; ++hh) {
        const int h = hk * rep + hh;
        const T* qb = q + (int64_t)b * S * ldq + (int64_t)h * D;
        const T* gtb = gt + ((int64_t)b * Hq + h) * D * ldt;
        const float* lse_b = lse + ((int64_t)b * Hq + h) * S;
        for (int qt0 = qbeg; qt0 < S; qt0 += CT) {
            __syncthreads();
            {
                TileStage<CT, KP> s1;
                s1.gload(reinterpret_cast<const char*>(qb + (int64_t)qt0 * ldq), ldq * SZ, S - qt0, KP);
                s1.swrite(sQ);
                TileStage<D, 128> s2;
                s2.gload(reinterpret_cast<const char*>(gtb + qt0), ldt * SZ, D, (int)min((int64_t)128, (ldt - qt0) * SZ));
                // columns past the sequence are zero whatever the copy's padding holds: P = 0 there, and 0 x NaN is not 0
#pragma unroll
                for (int p = 0; p < TileStage<D, 128>::NCH; ++p) {
                    const int c = (threadIdx.x + p * ANT) % 8;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (qt0 + c * 4 + e >= S) s2.r[p][e] = 0u;
                }
                s2.swrite(sGt);
            }
            __syncthreads();

            // st[t][r] = score(query qt0 + 16 t + 4 g + r, key ki)
            f32x4 st[NC16];
#pragma unroll
            for (int t = 0; t < NC16; ++t) st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < NC16; ++t)
#pragma unroll
                for (int c = 0; c < NDC; ++c) st[t] = Mma16<T>::mma(rm_frag<T, D>(sQ, t, c, lane), kf[c], st[t]);
#pragma unroll
            for (int t = 0; t < NC16; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int qi = qt0 + t * 16 + g * 4 + r;
                    const bool in = qi < S && qi >= q_begin;
                    int ivlo = 0, ivhi = S;
                    if (row_lo != nullptr && in) { ivlo = row_lo[(int64_t)b * S + qi]; ivhi = row_hi[(int64_t)b * S + qi]; }
                    const bool ok = in && visible(qi, ki, S, 1, 0, ivlo, ivhi);
                    const float lq = in ? lse_b[qi] : 0.f;
                    st[t][r] = ok ? __expf(st[t][r] * scale - lq) : 0.f;
                }
#pragma unroll
            for (int dt = 0; dt < ND16; ++dt)
#pragma unroll
                for (int kc = 0; kc < NC16; ++kc) dvacc[dt] = Mma16<T>::mma(tr_frag<T>(sGt, dt, kc, lane), PackCols<T>::pack(st, kc), dvacc[dt]);
        }
    }
    store_rows<T, D>(dv + (int64_t)b * S * lddv + (int64_t)hk * D, lddv, ki, S, dvacc, 1.f, lane);
}

}  // namespace

namespace attn32 {

// ---- bf16: NWV = 8 or 4 waves x 32 keys; per step a [64 queries][256 B] Q tile, the G tile of the same rows and their 64 lse values, two stages.
// The steps run over (query head of the group, query tile), heads outermost, as ONE pipelined sequence: the first tile of the next head is
// staged under the last tile of this one.
// Budget against dkv_kernel (d = 128): registers -- dV^T accumulators 64 + K fragments 32 + S^T 16 + operand rings and addresses, about 150
// where dkv_kernel needs 256; the dK accumulators (64) and the dP^T block (16) are gone.  LDS -- 2 x (2 x 16 KiB + 256 B) = 64.5 KiB where
// dkv_kernel holds 128.5 KiB: the per-wave V blocks (64 KiB) are gone.  Occupancy stays at two waves per SIMD (four would need <= 128 registers and the
// three register-resident blocks above are 112 before any operand is read); what the freed LDS buys is that those eight waves may be TWO
// 4-wave workgroups of 128 keys each (the host picks NWV, see lrp_attn_bwd_dv), which lets the item-major grid order level the causal 8 : 1.
template <int DH, bool IV, int NWV>
__global__ __launch_bounds__(NWV * 64, 2) void dv_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ gho, const float* __restrict__ lse,
    bf16_t* __restrict__ dv, int S, int Hq, int Hkv, int64_t ldq, int64_t ldk, int64_t ldg, int64_t lddv, float scale, int B, int q_begin,
    const int* __restrict__ row_lo, const int* __restrict__ row_hi) {
    constexpr int BK = NWV * 32, STAGE = 2 * TILE + 256, NK = DH / 16, ND32 = DH / 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int bhk, kblk;
    if (!xcd_item_major_decode(blockIdx.x, B * Hkv, (S + BK - 1) / BK, bhk, kblk)) return;
    const int b = bhk / Hkv, hk = bhk % Hkv, rep = Hq / Hkv;
    const int k0 = kblk * BK, kw = k0 + wave * 32, ki = kw + l31;
    const int* rlo_b = (IV && row_lo) ? row_lo + (int64_t)b * S : nullptr;
    const int* rhi_b = (IV && row_lo) ? row_hi + (int64_t)b * S : nullptr;
    int* const ivtab = reinterpret_cast<int*>(smem + 2 * STAGE);     // per-32-query-block interval bounds (only with row intervals)

    bf16x8 kf[NK];
    load_row_frags<DH>(kf, k + (int64_t)b * S * ldk + (int64_t)hk * DH, ldk, ki, S, hi);
    f32x16 dvacc[ND32];
#pragma unroll
    for (int db = 0; db < ND32; ++db) dvacc[db] = zero16();
    const float c1 = scale * LRP_LOG2E;
    int qbeg = (max(k0, q_begin) / CT) * CT, qend = S;               // causal; queries below q_begin carry no gradient
    if (rlo_b != nullptr) {
        int qlo, qhi;
        iv_block_table<NWV>(rlo_b, rhi_b, S, k0, BK, wave, lane, ivtab, reinterpret_cast<int*>(smem), qlo, qhi);
        qbeg = max(qbeg, (min(qlo, S) / CT) * CT);
        qend = min(qend, qhi);
    }
    const int ntile = qbeg < qend ? (qend - qbeg + CT - 1) / CT : 0, nstep = ntile * rep;

    auto stage = [&](int step, int buf) {
        const int hh = step / ntile, qt0 = qbeg + (step - hh * ntile) * CT, h = hk * rep + hh;
        char* sb = smem + buf * STAGE;
        stage_tile<NWV, DH>(q + (int64_t)b * S * ldq + (int64_t)h * DH, ldq, qt0, S, sb, wave, lane);
        stage_tile<NWV, DH>(gho + (int64_t)b * S * ldg + (int64_t)h * DH, ldg, qt0, S, sb + TILE, wave, lane);
        if (wave == 0) stage_stats(lse + ((int64_t)b * Hq + h) * S, qt0, S, sb + 2 * TILE, lane);
    };
    if (nstep > 0) stage(0, 0);
    __syncthreads();
    // absolute LDS addresses of the current stage (Q tile; G tile = + TILE; 32-row block qb = + qb * 8192; lse at + 2 TILE)
    uint32_t arm0, atr[ND32][2], ast;
    {
        const uint32_t sbase = lds_addr(smem);
        LaneAddr la;
        la.init(lane);
        arm0 = sbase + la.rm[0];
#pragma unroll
        for (int db = 0; db < ND32; ++db) { atr[db][0] = sbase + la.tr[db][0]; atr[db][1] = sbase + la.tr[db][1]; }
        ast = sbase + 2 * TILE + hi * 16;
    }
    int cur = 0, qt0 = qbeg, tile = 0;
    for (int step = 0; step < nstep; ++step) {
        if (step + 1 < nstep) stage(step + 1, cur ^ 1);
        sfor<0, 2>([&](auto qbc) {
            constexpr int qb = decltype(qbc)::value, QO = qb * 32 * KP, SO = qb * 128;
            const int qq0 = qt0 + qb * 32;
            bool live = !(qq0 + 31 < kw || qq0 >= S || qq0 + 31 < q_begin);   // false: no query of the block reaches a key of the wave
            bool iv_mask = false;
            if (live && rlo_b != nullptr) {
                int t0_, t1_, t2_, t3_;
                iv_row(ivtab, qq0 >> 5, t0_, t1_, t2_, t3_);
                if (t1_ <= kw || t0_ >= kw + 32) live = false;           // no query of the block sees a key of this wave
                iv_mask = !(t2_ <= kw && t3_ >= kw + 32);                // some row's interval ends inside the wave's keys
            }
            if (!live) return;
            // ---- S^T: Q fragments read PD steps ahead through a ring of PD + 1 slots (dkv_kernel's phase 1 with one read per step, not three)
            f32x16 st = zero16();
            f32x4 sl[2];                                                // lse of the queries 8 i + 4 hi + 0..3, double-buffered
            constexpr int PD = 2, RS = PD + 1;
            bf16x8 fq[RS];
            static_assert(PD < NK && PD == 2, "the prologue below issues the reads of steps 0 .. PD - 1");
            {
                const uint32_t a0 = frag_addr<0>(arm0), a1 = frag_addr<1>(arm0);
                A32_RD128(fq[0], a0, QO); A32_RD128(fq[1], a1, QO);
            }
            sfor<0, NK>([&](auto ksc) {
                constexpr int ks = decltype(ksc)::value, cu = ks % RS, nx = (ks + PD) % RS;
                // reads younger than step ks's at the wait: the steps ks + 1 .. min(ks + PD, NK - 1) and, from step NK - 2 on, the first lse read
                constexpr int ahead = (ks + PD < NK ? PD : NK - 1 - ks);
                if constexpr (ks + PD < NK) {
                    const uint32_t aq = frag_addr<ks + PD>(arm0);
                    A32_RD128(fq[nx], aq, QO);
                }
                if constexpr (ks == NK - 2) A32_RD128(sl[0], ast, SO);
                constexpr int nw = ahead + (ks >= NK - 2 ? 1 : 0);
                asm volatile("s_waitcnt lgkmcnt(%[n])" : "+v"(fq[cu]) : [n] "n"(nw));
                st = mfma32(fq[cu], kf[ks], st);
                A32_FENCE();
            });
            // ---- P of one 16-query group j (two 8-register halves i = 2 j, 2 j + 1), then dV^T += G^T P^T over the head-dim blocks.  Transpose-
            // read group n = (j, db) = (n / ND32, n % ND32) uses register slot n & 1 and is issued one group ahead; group (1, 0) is in flight
            // under the element-wise work of j = 1.  LDS reads return in order: every wait below names how many younger reads may stay out.
            u32x2 tg[2][2];
            bf16x8 pf[2];
            const bool masked = (qq0 + 32 > S) || (qq0 < kw + 31) || iv_mask || (qq0 < q_begin);
            auto trg = [&](auto nc) {
                constexpr int n = decltype(nc)::value, sl_ = n & 1, jj = n / ND32, dbb = n % ND32;
                auto& tgr = tg;                 // (named outside the asm operands: an operand alone does not make the lambda capture them)
                auto& adr = atr;
                A32_RDTR(tgr[sl_][0], adr[dbb][0], QO + TILE + jj * 16 * KP);
                A32_RDTR(tgr[sl_][1], adr[dbb][1], QO + TILE + jj * 16 * KP);
            };
            auto dv_step = [&](auto nc, auto wc) {
                constexpr int n = decltype(nc)::value, sl_ = n & 1, jj = n / ND32, dbb = n % ND32, w = decltype(wc)::value;
                if constexpr (w >= 0) asm volatile("s_waitcnt lgkmcnt(%[n])" : "+v"(tg[sl_][0]), "+v"(tg[sl_][1]) : [n] "n"(w));
                dvacc[dbb] = mfma32(join_tr(tg[sl_][0], tg[sl_][1]), pf[jj], dvacc[dbb]);
                A32_FENCE();
            };
            auto elementwise = [&](auto ic) {
                constexpr int i = decltype(ic)::value, cu = i & 1, nx = cu ^ 1, tsl = (i == 1 ? 0 : (ND32 & 1));
                // issue order: lse(0) [phase 1], group 0, lse(1), lse(2), groups 1 .. ND32, lse(3), groups ND32 + 1 ..
                if constexpr (i == 0) {
                    A32_RD128(sl[nx], ast, SO + 32);
                    A32_WAIT(3, "+v"(sl[cu]));                                        // younger: group 0 (2), lse(1)
                } else if constexpr (i == 1) {
                    A32_RD128(sl[nx], ast, SO + 64);
                    A32_WAIT(1, "+v"(sl[cu]), "+v"(tg[tsl][0]), "+v"(tg[tsl][1]));    // younger: lse(2); group 0 is older: landed
                } else if constexpr (i == 2) {
                    A32_RD128(sl[nx], ast, SO + 96);
                    A32_WAIT(3, "+v"(sl[cu]));                                        // younger (at least): group ND32 (2), lse(3)
                } else {
                    A32_WAIT(0, "+v"(sl[cu]), "+v"(tg[tsl][0]), "+v"(tg[tsl][1]));    // everything landed, group ND32 (slot ND32 & 1) included
                }
                float pe[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) pe[e] = fast_exp2(__builtin_fmaf(st[4 * i + e], c1, -(sl[cu][e] * LRP_LOG2E)));
                if (masked) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int qi = qq0 + 8 * i + 4 * hi + e;
                        int ivlo = 0, ivhi = S;
                        if constexpr (IV) { if (rlo_b != nullptr && qi < S) { ivlo = rlo_b[qi]; ivhi = rhi_b[qi]; } }
                        pe[e] = ((qi < S) & (qi >= q_begin) & visible(qi, ki, S, 1, 0, ivlo, ivhi)) ? pe[e] : 0.f;
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) pf[i >> 1][4 * (i & 1) + e] = (bf16_t)pe[e];
                A32_FENCE();
            };
            trg(IC<0>{});
            A32_FENCE();
            elementwise(IC<0>{});
            elementwise(IC<1>{});
            sfor<0, ND32>([&](auto dbc) {
                constexpr int n = decltype(dbc)::value;
                trg(IC<n + 1>{});
                dv_step(IC<n>{}, IC<(n == 0 ? -1 : 2)>{});                           // younger: group n + 1 (2)
            });
            elementwise(IC<2>{});
            elementwise(IC<3>{});
            sfor<0, ND32>([&](auto dbc) {
                constexpr int n = ND32 + decltype(dbc)::value, last = (n + 1 == 2 * ND32);
                if constexpr (!last) trg(IC<n + 1>{});
                dv_step(IC<n>{}, IC<(n == ND32 ? -1 : (last ? 0 : 2))>{});
            });
        });
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // the next step's tiles have landed (this wave's pieces)
        __syncthreads();
        {
            const uint32_t delta = cur ? (uint32_t)-STAGE : (uint32_t)STAGE;
            arm0 += delta;
#pragma unroll
            for (int db = 0; db < ND32; ++db) { atr[db][0] += delta; atr[db][1] += delta; }
            ast += delta;
        }
        cur ^= 1;
        qt0 += CT;
        if (++tile == ntile) { tile = 0; qt0 = qbeg; }
    }
    store_rows<DH>(dv + (int64_t)b * S * lddv + (int64_t)hk * DH, lddv, ki, S, dvacc, 1.f, hi);
}

constexpr size_t DV_LDS_MAX = 160 * 1024;          // gfx950: 160 KiB per workgroup (the interval table grows with S)

}  // namespace attn32

static inline bool dv_bf16_ok(int d) { return d == 64 || d == 96 || d == 128; }
static inline bool dv_f32_ok(int d) { return d == 16 || d == 32 || d == 64 || d == 128; }
extern "C" int lrp_attn_bwd_dv_ok(int dtype, int d) { return (dtype == LRP_BF16 && dv_bf16_ok(d)) || (dtype == LRP_F32 && dv_f32_ok(d)) ? 1 : 0; }

extern "C" int lrp_attn_bwd_dv(const void* q, const void* k, const void* G, const void* G_t, const float* lse, void* dv, int B, int S, int Hq,
                               int Hkv, int d, int64_t ldq, int64_t ldk, int64_t ldg, int64_t ldt, int64_t lddv, float scale, int q_begin,
                               const int* row_lo, const int* row_hi, int dtype, void* stream) {
    if ((row_lo == nullptr) != (row_hi == nullptr)) return LRP_EINVAL;
    if (!q || !k || !G || !lse || !dv) return LRP_EINVAL;
    if (!(scale > 0.f) || q_begin < 0) return LRP_EINVAL;
    if (B < 0 || S < 0 || Hq < 1 || Hkv < 1 || (Hq % Hkv) || d < 16) return LRP_EINVAL;
    if (dtype != LRP_F32 && dtype != LRP_BF16) return LRP_EINVAL;
    const bool need_t = lrp_attn_needs_transposed(dtype, d) != 0;
    if (need_t && !G_t) return LRP_EINVAL;
    if (B > 65535 || Hq > 65535) return LRP_ESHAPE;
    if (!lrp_attn_bwd_dv_ok(dtype, d)) return LRP_ESHAPE;
    const int epc = dtype == LRP_F32 ? 4 : 8;
    if (!al16(q) || !al16(k) || !al16(G) || !al16(dv) || (ldq % epc) || (ldk % epc) || (ldg % epc) || (lddv % 4)) return LRP_EALIGN;
    if (need_t && (!al16(G_t) || (ldt % epc) || ldt < S)) return LRP_EALIGN;
    if (B == 0 || S == 0) return LRP_OK;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == LRP_F32) {
        const dim3 grid((S + 63) / 64, Hkv, B);
#define DV_F32(DD)                                                                                                                            \
    lrp_launch_lds<attn_bwd_dv_kernel<DD>>(grid, dim3(ANT), (size_t)32 * DD * 4 + (size_t)DD * 128, (size_t)32 * DD * 4 + (size_t)DD * 128, st, \
                                           (const float*)q, (const float*)k, (const float*)G_t, lse, (float*)dv, S, Hq, Hkv, ldq, ldk, ldt,   \
                                           lddv, scale, q_begin, row_lo, row_hi)
        switch (d) {
            case 16: DV_F32(16); break;
            case 32: DV_F32(32); break;
            case 64: DV_F32(64); break;
            default: DV_F32(128); break;
        }
#undef DV_F32
        return lrp_check_launch();
    }
    using namespace attn32;
    const bool iv = row_lo != nullptr;
    const size_t lds = 2 * (2 * (size_t)TILE + 256) + (iv ? (size_t)((S + 31) / 32) * 16 : 0);   // + the interval table
    if (lds > DV_LDS_MAX) return LRP_ESHAPE;
    // Key blocks of 256 (8 waves) or 128 (4 waves, two workgroups per CU: 2 x 64.5 KiB of LDS).  A workgroup's chain is rep x tiles steps long and
    // the first key block's is 2 S / 256 times the last one's (causal): a grid of fewer than ~4 workgroups per CU cannot level that, so it is
    // cut finer -- the item-major order then pairs a heavy block with light ones on a CU.  A key's sum does not see the choice (same heads,
    // same tiles, same order): the result is bitwise the same either way.  DV_FORCE_NW: tools/cp_bench.py's A/B build.
#ifdef DV_FORCE_NW
    const int nwv = DV_FORCE_NW;
#else
    const int nwv = (int64_t)B * Hkv * ((S + 255) / 256) < 4 * (int64_t)lrp_num_cus() ? 4 : 8;
#endif
    const dim3 grid(xcd_group_grid(B * Hkv, (S + nwv * 32 - 1) / (nwv * 32)));
#define DV_BF16(DH)                                                                                                                          \
    lrp_with_bool(iv, [&](auto ivf) {                                                                                                        \
        lrp_with_bool(nwv == 4, [&](auto four) {                                                                                             \
            constexpr int NWV = decltype(four)::value ? 4 : 8;                                                                               \
            lrp_launch_lds<dv_kernel<DH, decltype(ivf)::value, NWV>>(grid, dim3(NWV * 64), lds, DV_LDS_MAX, st, (const bf16_t*)q,            \
                                                                     (const bf16_t*)k, (const bf16_t*)G, lse, (bf16_t*)dv, S, Hq, Hkv, ldq,  \
                                                                     ldk, ldg, lddv, scale, B, q_begin, row_lo, row_hi);                     \
        });                                                                                                                                  \
    })
    switch (d) {
        case 64: DV_BF16(64); break;
        case 96: DV_BF16(96); break;
        default: DV_BF16(128); break;
    }
#undef DV_BF16
    return lrp_check_launch();
}
