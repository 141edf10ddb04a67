// attention32_tiles.hpp -- what the 32x32x16 / transpose-read attention kernels share: tile geometry, staging, lane addresses, hand-issued
// LDS reads, stores and the row-interval tables.  Included by attention32.hip (forward, dQ, dK / dV) and attention_cp.hip (dV alone).
#pragma once
#include "common.hpp"

namespace attn32 {

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_t;
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;

constexpr int NW = 8;              // waves per workgroup of the dK/dV kernel (256 keys)
constexpr int NWQ = 4;             // waves per workgroup of the forward / dQ kernels: 128 queries, TWO workgroups per CU, so that
                                   // one workgroup's prologue / store tail and barrier waits run under the other's MFMAs
constexpr int CT = 64;             // column-side rows per tile
constexpr int KP = 256;            // bytes per LDS tile row: the head-dim-128 image for EVERY head dim DH in {64, 96, 128} (16-byte chunks
                                   // >= DH / 8 of a row are never staged and never read: one swizzle, one set of lane addresses)
constexpr int TILE = CT * KP;      // 16 KiB
constexpr int NKX = 8, NDX = 4;    // array bounds (DH = 128); an instantiation for DH runs NK = DH / 16 MFMA k-steps over the head dim and
                                   // ND32 = DH / 32 32-wide head-dim blocks per out^T accumulator
#define LRP_LOG2E 1.4426950408889634f

LRP_DEVICE int rot4(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }
LRP_DEVICE float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

LRP_DEVICE bool xcd_group_decode(int L, int ngroups, int per_group, int& group, int& item) {
    const int xcd = L & 7, i = L >> 3;
    item = i % per_group;
    group = xcd + 8 * (i / per_group);
    return group < ngroups;
}
// the same grid walked ITEM-major within a XCD: all groups' item 0 first, then item 1, ... -- for the dK / dV kernel, whose items (key blocks of a
// head) differ 8 : 1 in work (causal) and whose 128-KiB workgroups run ONE per CU: with the group-major order the last head's heaviest key
// block starts when the other CUs are already draining (list-scheduling simulation of 16 heads x 8 key blocks on a XCD's 32 CUs: makespan 88 tile
// steps against an ideal of 72; item-major -- heaviest first over ALL heads -- reaches 72).  Price: a head's key blocks no longer run at the same
// time on one XCD, so its Q / Gho tiles are re-read from the Infinity Cache instead of the XCD's L2.
LRP_DEVICE bool xcd_item_major_decode(int L, int ngroups, int per_group, int& group, int& item) {
    const int xcd = L & 7, i = L >> 3, gpx = (ngroups + 7) >> 3;
    item = i / gpx;
    group = xcd + 8 * (i % gpx);
    return group < ngroups;
}

// stage a [64 rows][256 B] tile of a token-major operand: 16 one-KiB groups of 4 rows, 16 / NWV per wave, each one
// buffer_load_dwordx4 .. lds -- ONE per-lane byte offset (row (l >> 4) of the group, swizzled chunk; the
// group index only enters the chunk through grp & 3 = wave & 3), the group's first row in the scalar offset, rows >= S read as zero
// through num_records (a zero K / V / Q / Gho row contributes nothing: masked keys, and dS^T Q = P^T Gho = 0 for a zero query row).
// A global_load_lds piece with its 64-bit per-lane address costs ~80-120 cycles at issue, a buffer piece ~35 (profiles/r03_gemm_experiments.txt).
// Head dims below 128: a lane whose source chunk lies past the head (chunk >= DH / 8) gets an offset beyond num_records -- the buffer
// unit returns zero without a memory request; its LDS slot is never read.
constexpr int A32_OOB = 0x40000000;
template <int NWV = NW, int DH = 128>
LRP_DEVICE void stage_tile(const bf16_t* base, int64_t ld, int row0, int S, char* lds, int wave, int lane) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)(((int64_t)(S - 1) * ld + DH) * 2), 0x00020000);
    const int rl = lane >> 4, slot = lane & 15;
    const int chunk_ = slot ^ ((rl << 2) | (wave & 3));
    const int voff = (DH == 128 || chunk_ < DH / 8) ? (int)(rl * ld * 2) + (chunk_ << 4) : A32_OOB;
#pragma unroll
    for (int g = 0; g < 16 / NWV; ++g) {
        const int grp = g * NWV + wave;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(lds + grp * 1024), 16, voff, (int)((int64_t)(row0 + grp * 4) * ld * 2), 0, 0);
    }
}
// 64 fp32 row statistics -> lds[0..63]
LRP_DEVICE void stage_stats(const float* base, int r0, int S, char* lds, int lane) {
    int r = r0 + lane;
    r = r < S ? r : S - 1;
    __builtin_amdgcn_global_load_lds((glb_ptr_t)(base + r), (lds_ptr_t)lds, 4, 0, 0);
}

// per-lane LDS byte offsets (relative to a tile base), hoisted out of the tile loops
struct LaneAddr {
    uint32_t rm[NKX];         // row fragment: row (lane & 31) of a 32-row block, head-dim chunk 2 ks + hi
    uint32_t tr[NDX][2];      // transpose read: head-dim block db, half (rows +0..3 / +8..11 of a 16-row group, + 4 hi)
    LRP_DEVICE void init(int lane) {
        const int l31 = lane & 31, hi = lane >> 5, i16 = lane & 15;
#pragma unroll
        for (int ks = 0; ks < NKX; ++ks) rm[ks] = l31 * KP + (((ks * 2 + hi) ^ rot4(l31)) << 4);
#pragma unroll
        for (int db = 0; db < NDX; ++db)
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int r = half * 8 + 4 * hi + (i16 >> 2);                       // row within its 16-row group
                const int chunk = db * 4 + ((l31 >> 4) << 1) + ((i16 & 3) >> 1);
                tr[db][half] = r * KP + ((chunk ^ rot4(r)) << 4) + 8 * (i16 & 1);
            }
    }
};

LRP_DEVICE bf16x8 lds_frag(const char* tile, uint32_t off) { return *reinterpret_cast<const bf16x8*>(tile + off); }
// 8 contraction slots of one head-dim column: rows {4hi..4hi+3} and {8+4hi..8+4hi+3} of the 16-row group at `tile`
LRP_DEVICE bf16x8 lds_frag_tr(const char* tile, uint32_t off0, uint32_t off1) {
    const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(tile + off0));
    const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(tile + off1));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    const s16x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(bf16x8, v);
}
LRP_DEVICE f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
LRP_DEVICE f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}
// accumulator registers 8j .. 8j+7 as the next MFMA's operand
LRP_DEVICE bf16x8 pack8(const f32x16& x, int j) {
    bf16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (bf16_t)x[8 * j + e];
    return r;
}
// column-side row of accumulator register r in lane-half hi
LRP_DEVICE int crow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// ---- hand-issued LDS reads ---------------------------------------------------------------------------------------------
// The compiler's own bookkeeping puts s_waitcnt lgkmcnt(0) behind every fresh fragment read, i.e. {read, wait the full LDS
// latency, MFMA} per contraction step.  The LDS returns in order, so "the fragment I need" = "all but the n younger reads":
// reads are issued a few steps ahead as inline asm and waited for with hand-counted s_waitcnt lgkmcnt(n); sched_barrier(0)
// keeps the groups in program order.  (Outstanding scalar loads or compiler-issued LDS operations can only make a counted
// wait more conservative.)  A side effect: the compiler no longer sees LDS reads that might alias the in-flight
// direct-to-LDS loads of the next tile and stops draining vmcnt in the middle of the tile.
#define A32_RD128(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(dst) : "v"(addr), "n"(off))
#define A32_RDTR(dst, addr, off) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=&v"(dst) : "v"(addr), "n"(off))
#define A32_WAIT(n, ...) asm volatile("s_waitcnt lgkmcnt(" #n ")" : __VA_ARGS__)
#define A32_FENCE() __builtin_amdgcn_sched_barrier(0)
// the 2 ND transpose reads (ND head-dim blocks x 2 halves) of one 16-row group, and the counted waits that name them as results
template <int ND, int OFF> LRP_DEVICE void tr_group(u32x2 (&dst)[NDX][2], const uint32_t (&adr)[NDX][2]) {
    A32_RDTR(dst[0][0], adr[0][0], OFF); A32_RDTR(dst[0][1], adr[0][1], OFF);
    A32_RDTR(dst[1][0], adr[1][0], OFF); A32_RDTR(dst[1][1], adr[1][1], OFF);
    if constexpr (ND > 2) { A32_RDTR(dst[2][0], adr[2][0], OFF); A32_RDTR(dst[2][1], adr[2][1], OFF); }
    if constexpr (ND > 3) { A32_RDTR(dst[3][0], adr[3][0], OFF); A32_RDTR(dst[3][1], adr[3][1], OFF); }
}
#define A32_TRV2(t) "+v"(t[0][0]), "+v"(t[0][1]), "+v"(t[1][0]), "+v"(t[1][1])
#define A32_TRV3(t) A32_TRV2(t), "+v"(t[2][0]), "+v"(t[2][1])
#define A32_TRV4(t) A32_TRV3(t), "+v"(t[3][0]), "+v"(t[3][1])
template <int ND, int N> LRP_DEVICE void wait_tr(u32x2 (&t)[NDX][2]) {
    if constexpr (ND == 4) asm volatile("s_waitcnt lgkmcnt(%[n])" : A32_TRV4(t) : [n] "n"(N));
    else if constexpr (ND == 3) asm volatile("s_waitcnt lgkmcnt(%[n])" : A32_TRV3(t) : [n] "n"(N));
    else asm volatile("s_waitcnt lgkmcnt(%[n])" : A32_TRV2(t) : [n] "n"(N));
}
template <int ND, int N> LRP_DEVICE void wait_tr2(u32x2 (&t)[NDX][2], u32x2 (&u)[NDX][2]) {
    if constexpr (ND == 4) asm volatile("s_waitcnt lgkmcnt(%[n])" : A32_TRV4(t), A32_TRV4(u) : [n] "n"(N));
    else if constexpr (ND == 3) asm volatile("s_waitcnt lgkmcnt(%[n])" : A32_TRV3(t), A32_TRV3(u) : [n] "n"(N));
    else asm volatile("s_waitcnt lgkmcnt(%[n])" : A32_TRV2(t), A32_TRV2(u) : [n] "n"(N));
}
// Measured and NOT adopted (profiles/r02_attention_experiments.txt): s_setprio schemes that favour one of the two waves of a
// SIMD (static, or high priority in the MFMA phases only) change nothing -- tools/attn_timeline.py shows the MFMA phases of a
// wave already running at close to their single-wave time, i.e. the two waves of a SIMD are complementary; what is left is the
// per-wave cost of the element-wise phase (VALU issue beside the other wave's MFMAs), the LDS-DMA issue cost of the staging
// loads and the per-workgroup prologue / store tail.
// A32_TIMELINE -- the one build switch of this file.  It is instrumentation, not a fork between two kernels: undefined (every shipped
// build) A32_TS and the #ifdef A32_TIMELINE blocks compile to nothing; with -DA32_TIMELINE the dQ and dK / dV (d <= 128) kernels add up
// per-wave shader-clock totals of their loop segments and write them over the first words of the wave's first output row.  Built only by
// tools/attn_timeline.py, tools/attn_dkv_timeline.py and tools/attn_dkv_only.py.
#ifdef A32_TIMELINE
#define A32_TS(slot)                                                          \
    {                                                                         \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                    \
        const uint32_t now_ = (uint32_t)__builtin_readcyclecounter();         \
        tl_acc[slot] += now_ - tl_prev;                                       \
        tl_prev = now_;                                                       \
    }
#else
#define A32_TS(slot)
#endif
template <int V> struct IC { static constexpr int value = V; };
template <int I, int N, typename F> LRP_DEVICE void sfor(F&& f) {
    if constexpr (I < N) {
        f(IC<I>{});
        sfor<I + 1, N>(static_cast<F&&>(f));
    }
}
// value of the other lane half (lane ^ 32) combined with one's own: v_permlane32_swap (upper 32 lanes of the first operand
// <-> lower 32 lanes of the second) instead of an LDS round trip.  Inline asm: the builtin's second result was folded away
// by the compiler when both operands are the same value; s_nop 1 = the VALU-write -> permlane-read wait states.
LRP_DEVICE void half_swap(float& a, float& b) { asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b)); }
LRP_DEVICE float half_max(float x) {
    float a = x, b = x;
    half_swap(a, b);
    return fmaxf(a, b);
}
LRP_DEVICE float half_sum(float x) {
    float a = x, b = x;
    half_swap(a, b);
    return a + b;
}
// row-fragment address of contraction step ks from the step-0 address: chunk (2 ks + hi) ^ rot = (2 ks) ^ (hi ^ rot), so the
// eight addresses differ by an XOR of ks << 5 (tile rows are 256-byte aligned).  Kept opaque (asm volatile) so that the
// compiler recomputes it next to the read instead of keeping eight address registers live across the kernel.
template <int KS> LRP_DEVICE uint32_t frag_addr(uint32_t a0) {
    if constexpr (KS == 0) return a0;
    else {
        uint32_t r;
        asm volatile("v_xor_b32 %0, %1, %2" : "=v"(r) : "n"(KS << 5), "v"(a0));
        return r;
    }
}
LRP_DEVICE uint32_t lds_addr(const void* p) { return (uint32_t)(uintptr_t)(lds_ptr_t)p; }
// the two halves of a transpose-read fragment as one MFMA operand
LRP_DEVICE bf16x8 join_tr(u32x2 a, u32x2 b) {
    const u32x4 v = {a[0], a[1], b[0], b[1]};
    return __builtin_bit_cast(bf16x8, v);
}

template <int DH>
LRP_DEVICE void load_row_frags(bf16x8* f, const bf16_t* base, int64_t ld, int row, int S, int hi) {
    const bool ok = row < S;
#pragma unroll
    for (int ks = 0; ks < DH / 16; ++ks) {
        if (ok) f[ks] = *reinterpret_cast<const bf16x8*>(base + (int64_t)row * ld + ks * 16 + hi * 8);
        else {
            u32x4 z = {0, 0, 0, 0};
            f[ks] = __builtin_bit_cast(bf16x8, z);
        }
    }
}
// out^T accumulators -> token-major rows: lane (row, hi) holds head-dim columns db*32 + 8 i + 4 hi + 0..3
// Round 5: 16-byte stores.  A row's 8-column groups are split between its two lanes (hi = 0: columns 8 i .. + 3, hi = 1: 8 i + 4 .. + 7), so the
// natural store is 4 x 8 bytes per 32-column block and lane -- 32 store instructions per lane for dK + dV, and the store tail of a workgroup is
// ISSUE-bound (MI355X_MICROARCH.md: ~9.3k cycles per 16 dwordx2 stores; cdna_hip_programming.md T21).  v_permlane32_swap between the packed
// registers of groups i and i + 1 gives the lower lane columns 8 i .. 8 i + 7 and the upper lane 8 (i + 1) .. + 7: one dwordx4 store per pair.
template <int DH>
LRP_DEVICE void store_rows(bf16_t* base, int64_t ld, int row, int S, const f32x16* acc, float mul, int hi) {
    const bool wide = (((reinterpret_cast<uintptr_t>(base) | (uintptr_t)(ld * 2)) & 15) == 0);        // wave-uniform (kernel arguments)
    if (!wide) {
        if (row >= S) return;
#pragma unroll
        for (int db = 0; db < DH / 32; ++db)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bf16x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (bf16_t)(acc[db][4 * i + e] * mul);
                *reinterpret_cast<bf16x4*>(base + (int64_t)row * ld + db * 32 + 8 * i + 4 * hi) = v;
            }
        return;
    }
    bf16_t* const rb = base + (int64_t)row * ld + 8 * hi;               // upper lane: the second 8-column half of a pair
#pragma unroll
    for (int db = 0; db < DH / 32; ++db)
#pragma unroll
        for (int i = 0; i < 4; i += 2) {
            bf16x4 va, vb;
#pragma unroll
            for (int e = 0; e < 4; ++e) { va[e] = (bf16_t)(acc[db][4 * i + e] * mul); vb[e] = (bf16_t)(acc[db][4 * (i + 1) + e] * mul); }
            u32x2 a = __builtin_bit_cast(u32x2, va), b = __builtin_bit_cast(u32x2, vb);
            auto r0 = __builtin_amdgcn_permlane32_swap(a[0], b[0], false, false);      // every lane takes part (rows >= S only skip the store)
            auto r1 = __builtin_amdgcn_permlane32_swap(a[1], b[1], false, false);
            const u32x4 o = {r0[0], r1[0], r0[1], r1[1]};
            if (row < S) *reinterpret_cast<u32x4*>(rb + db * 32 + 8 * i) = o;
        }
}

LRP_DEVICE bool visible(int q, int key, int S, int causal, int window, int lo, int hi) {
    return (key < S) & (!causal | (key <= q)) & ((window <= 0) | (key > q - window)) & (key >= lo) & (key < hi);   // no branches
}
// explicit stabilisers folded into ONE reciprocal (as attention.hip: lrp_ds2)
template <bool EXPL>
LRP_DEVICE float lrp_ds(float s_raw, float p, float dp, float Dq, float scale, float eps_mask, float eps_qk) {
    if constexpr (!EXPL) return p * (dp - Dq);                 // * scale / 2 folded into the final store
    else {
        const float s2 = s_raw * scale;
        return p * (dp - Dq) * scale * (s2 * s_raw) * __builtin_amdgcn_rcpf((s2 + eps_mask) * (2.f * s_raw + eps_qk));
    }
}

// ---- per-row key intervals: what a workgroup / a wave can see at all -------------------------------------------------------------------
// Callers that express their whole mask as intervals (causal = 0: Gemma-3 image + text prompts, packed sequences) would otherwise stream
// EVERY key tile past every query block and mask element by element.  The kernels derive the tile range from the intervals themselves:
// forward / dQ: the union [min lo, max hi) over the workgroup's query rows bounds the key loop, the wave's own union skips dead tiles, and a
// tile inside the INTERSECTION [max lo, min hi) of the wave's rows needs no per-element interval mask; dK / dV: the query rows whose interval
// meets the workgroup's keys bound the query loop.  No assumption on the intervals (monotone or not); one LDS round trip per workgroup.
struct IvWave { int lo_min, hi_max, lo_max, hi_min; };
LRP_DEVICE int wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
LRP_DEVICE int wave_max(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}
// lane's row interval [lo, hi) (rows >= S: in_range = false) -> the wave's bounds; sh[2 * wave], sh[2 * wave + 1] <- its union (the caller
// barriers and folds the waves' unions with iv_fold)
LRP_DEVICE IvWave iv_wave(int lo, int hi, bool in_range, int wave, int* sh) {
    const bool sees = in_range && hi > lo;
    IvWave w;
    w.lo_min = wave_min(sees ? lo : 0x7fffffff);
    w.hi_max = wave_max(sees ? hi : 0);
    w.lo_max = wave_max(in_range ? lo : 0);
    w.hi_min = wave_min(in_range ? hi : 0x7fffffff);
    sh[2 * wave] = w.lo_min;
    sh[2 * wave + 1] = w.hi_max;
    return w;
}
template <int NWAVES> LRP_DEVICE void iv_fold(const int* sh, int& lo, int& hi) {
    lo = sh[0];
    hi = sh[1];
#pragma unroll
    for (int w = 1; w < NWAVES; ++w) { lo = min(lo, sh[2 * w]); hi = max(hi, sh[2 * w + 1]); }
}
// dK / dV (the row side is keys; queries stream): a table [S / 32][4] = {lo_min, hi_max, lo_max, hi_min} of every 32-query block of batch entry b
// behind the kernel's tile buffers (host: + 16 bytes per block of dynamic LDS), built once per workgroup; from it the query range whose
// intervals meet the workgroup's keys [k0, k0 + BK), and per (query block, wave) "dead" / "no interval mask needed" as for forward / dQ
// one table row, read with a hand-issued ds_read_b128 (a compiler-visible LDS read in the tile loop would make the compiler drain the
// in-flight direct-to-LDS loads of the next tile first) and moved to scalar registers (wave-uniform branches)
LRP_DEVICE void iv_row(const int* tab, int blk, int& lo_min, int& hi_max, int& lo_max, int& hi_min) {
    u32x4 t;
    const uint32_t a = (uint32_t)(uintptr_t)(lds_ptr_t)tab + 16u * (uint32_t)blk;
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(t) : "v"(a));
    lo_min = __builtin_amdgcn_readfirstlane((int)t[0]);
    hi_max = __builtin_amdgcn_readfirstlane((int)t[1]);
    lo_max = __builtin_amdgcn_readfirstlane((int)t[2]);
    hi_min = __builtin_amdgcn_readfirstlane((int)t[3]);
}
template <int NWAVES> LRP_DEVICE void iv_block_table(const int* rlo, const int* rhi, int S, int k0, int BK, int wave, int lane, int* tab, int* sh,
                                                     int& qlo, int& qhi) {
    const int nblk = (S + 31) >> 5;
    for (int blk = wave; blk < nblk; blk += NWAVES) {
        const int r = blk * 32 + (lane & 31);
        const bool in = r < S;
        const int lo = in ? rlo[r] : 0, hi = in ? rhi[r] : 0;
        const bool sees = in && hi > lo;
        const int a = wave_min(sees ? lo : 0x7fffffff), e = wave_max(sees ? hi : 0), c = wave_max(in ? lo : 0), d_ = wave_min(in ? hi : 0x7fffffff);
        if (lane == 0) { tab[4 * blk] = a; tab[4 * blk + 1] = e; tab[4 * blk + 2] = c; tab[4 * blk + 3] = d_; }
    }
    __syncthreads();
    int a = 0x7fffffff, e = 0;
    for (int blk = threadIdx.x; blk < nblk; blk += NWAVES * 64)
        if (tab[4 * blk] < k0 + BK && tab[4 * blk + 1] > k0) { a = min(a, blk * 32); e = max(e, blk * 32 + 32); }
    a = wave_min(a);
    e = wave_max(e);
    sh[2 * wave] = a;
    sh[2 * wave + 1] = e;
    __syncthreads();
    iv_fold<NWAVES>(sh, qlo, qhi);
    __syncthreads();                                              // the scratch words are free again (they lie in the first tile buffer)
}

}  // namespace attn32
