// linear_stream.hpp -- the body the weight-streaming Linear kernels share: linear_stream.hip (W streamed as bf16 by LDS-DMA) and
// linear_stream_q.hip (W streamed as MXFP4 codes, decoded into the SAME wave-private LDS image) differ in how W travels and in nothing after
// it.  Here, once: the tile constants, the fragment addresses, one K tile's multiply, the last-arriver protocol of the split forms (the
// dgrad kernel of linear_stream.hip uses it too), the forward epilogue built from it, and the host policy.  The bit identity of
// lrp_linear_stream_fwd_q with lrp_mxfp4_dequant + lrp_linear_stream_fwd_tk (include/lrp_hip_mxfp4_stream.h) rests on both kernels running
// THIS code on the same LDS image; every decoded value is exact in bf16.  Two parts stand in both .hip files and MUST CHANGE TOGETHER:
//   * the x ring's stager (the kernels' stage_x lambdas; the MXFP4 one adds "past the range: LS_OOB");
//   * the epilogue: the plain forward kernel has ls_fwd_epilogue's statements written out, publish / ticket / slab sum included.
// Called as functions of this header they changed the plain kernel's code; written out, its six instantiations compile to the code they
// compiled to before this header existed (profiles/linear_stream_refactor_isa.txt, profiles/linear_stream_refactor_ab.txt).
#pragma once
#include "common.hpp"

namespace {

constexpr int LS_KT = 64;              // K elements per K tile
constexpr int LS_WD = 8;               // K tiles of W per wave-private LDS ring: [LS_WD tiles][16 rows][128 B], chunk c of row r at c ^ (r & 7)
constexpr int LS_OOB = 0x40000000;     // a buffer voffset beyond num_records: the load fetches nothing and returns zero
typedef __attribute__((address_space(3))) void* ls_lds_ptr_t;
extern __shared__ __attribute__((aligned(16))) char smem[];       // the workgroup's dynamic LDS

// MBMAX = 16-row blocks of x the instantiation has accumulators for, XD = x prefetch distance in K tiles
template <int MBMAX, int XD_> struct LSCfg {
    static constexpr int XD = XD_;
    static constexpr int NBUF = XD + 2;                            // LDS ring: tile t + XD is written while tiles t - 1, t may still be read
    static constexpr int P = MBMAX / 2;                            // 1-KiB staging pieces (8 rows x 128 B) per wave per K tile
    static constexpr int XTILE = MBMAX * 16 * 128;                 // bytes of one x tile
    static constexpr int BS = MBMAX < 4 ? MBMAX : 4;               // row blocks per LDS read batch
    static constexpr int NBATCH = MBMAX / BS;
};

template <int V> struct LSI { static constexpr int value = V; };
template <int I, int N, typename F> LRP_DEVICE void ls_for(F&& f) {
    if constexpr (I < N) {
        f(LSI<I>{});
        ls_for<I + 1, N>(static_cast<F&&>(f));
    }
}

#define LS_DSRD(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))

// ---- fragment addresses.  cX[ks] = ls_frag_x: row block i, k-step ks of an x tile = row 16 i + (l & 15), chunk (4 ks + (l >> 4)) ^ (row & 7)
// (+ i 2048 + the tile's base); cW[ks] = cX[ks] + ls_w_ring: ring slot s, k-step ks of the wave's W ring, the same image (row l & 15 of the
// wave's 16 rows; + s 2048)
LRP_DEVICE uint32_t ls_frag_x(int lane, int ks) {
    const uint32_t lds0 = (uint32_t)(uintptr_t)(ls_lds_ptr_t)smem;
    return lds0 + (uint32_t)((lane & 15) * 128) + (uint32_t)((((4 * ks + (lane >> 4)) ^ (lane & 7))) << 4);
}
template <typename C> LRP_DEVICE uint32_t ls_w_ring(int wave) { return (uint32_t)(C::NBUF * C::XTILE + wave * (LS_WD * 2048)); }

// ---- one K tile's multiply: W ring slot S against the x tile at byte xb of the x ring.  The callers keep what surrounds it (staging, the
// vmcnt wait, the s_barrier, the W refill).  D = mfma(Wfrag, xfrag), one v_mfma_f32_16x16x32_bf16 per accumulator and k-step in ascending K;
// blocks past nb are not multiplied.  Every LDS read is hand-counted: the wait that retires a read names its destination again ("+v")
template <typename C, int S, int MBMAX>
LRP_DEVICE void ls_tile_mma(const uint32_t (&cX)[2], const uint32_t (&cW)[2], uint32_t xb, LSI<S>, f32x4 (&acc)[MBMAX], int nb) {
    const uint32_t a0 = cX[0] + xb, a1 = cX[1] + xb;
    // this wave's W fragments of the tile: two reads, first in the LDS queue
    u32x4 wq0, wq1;
    LS_DSRD(wq0, cW[0], S * 2048);
    LS_DSRD(wq1, cW[1], S * 2048);
    // units u = (ks, batch): BS fragment reads each, read one unit ahead
    u32x4 xf[2][C::BS];
    constexpr int U = 2 * C::NBATCH;
    auto issue = [&](auto uc) {
        constexpr int u = decltype(uc)::value, ks = u / C::NBATCH, b = u % C::NBATCH;
        (void)&xf; (void)&a0; (void)&a1;
        ls_for<0, C::BS>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            (void)&xf; (void)&a0; (void)&a1;
            if constexpr (ks == 0) LS_DSRD(xf[u & 1][i], a0, (b * C::BS + i) * 2048);
            else LS_DSRD(xf[u & 1][i], a1, (b * C::BS + i) * 2048);
        });
    };
    issue(LSI<0>{});
    if constexpr (C::BS == 4) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(wq0), "+v"(wq1));
    else asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(wq0), "+v"(wq1));
    const bf16x8 w0 = __builtin_bit_cast(bf16x8, wq0), w1 = __builtin_bit_cast(bf16x8, wq1);
    ls_for<0, U>([&](auto uc) {
        constexpr int u = decltype(uc)::value, ks = u / C::NBATCH, b = u % C::NBATCH;
        (void)&xf;
        if constexpr (u + 1 < U) {
            issue(LSI<u + 1>{});
            if constexpr (C::BS == 4) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(xf[u & 1][0]), "+v"(xf[u & 1][1]), "+v"(xf[u & 1][2]), "+v"(xf[u & 1][3]));
            else asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(xf[u & 1][0]), "+v"(xf[u & 1][1]));
        } else {
            if constexpr (C::BS == 4) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xf[u & 1][0]), "+v"(xf[u & 1][1]), "+v"(xf[u & 1][2]), "+v"(xf[u & 1][3]));
            else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xf[u & 1][0]), "+v"(xf[u & 1][1]));
        }
        ls_for<0, C::BS>([&](auto ic) {
            constexpr int i = decltype(ic)::value, blk = b * C::BS + i;
            if (blk < nb)
                acc[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ks == 0 ? w0 : w1, __builtin_bit_cast(bf16x8, xf[u & 1][i]), acc[blk], 0, 0, 0);
        });
        __builtin_amdgcn_sched_barrier(0);
    });
}

// ---- the last-arriver protocol of the split forms: every split's workgroup publishes its fp32 partial quads into its slab, takes a ticket of
// its column block, and the LAST arriver sums the slabs in slab order -- its own from memory as well, so the result does not
// depend on who arrives last -- and writes the output.  One zero-initialised ticket word per column block, private to the stream.
// (1) publish: agent-scope stores are write-through (sc1): visible to the last arriver's agent-scope loads whatever XCD it runs on
LRP_DEVICE void ls_publish_quad(float* dst, f32x4 v) {
    uint64_t* d8 = reinterpret_cast<uint64_t*>(dst);
    const f32x2 lo = {v[0], v[1]}, hi2 = {v[2], v[3]};
    __hip_atomic_store(d8, __builtin_bit_cast(uint64_t, lo), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(d8 + 1, __builtin_bit_cast(uint64_t, hi2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// (2) ticket: is this workgroup the last of its column block's gridDim.y to arrive?  `ticket` is the block's word; the value passes through
// the first word of the LDS, which nothing reads any more.
// Ordering: the producers' side is the hardware path -- sc1 write-through stores, drained by vmcnt(0) and a workgroup barrier
// BEFORE the ticket atomic is issued, so the slabs are at the device coherence point when the ticket moves (a RELEASE on the ticket would add
// a whole-L2 write-back per workgroup: round 3 measured that at more than the second launch it replaces); the consumer's side is made
// explicit: an agent-scope ACQUIRE fence (one L2 / vector-cache invalidate per column block) ahead of the slab loads, which are agent-scope
// atomics the compiler may not hoist above it
LRP_DEVICE bool ls_last_arriver(unsigned* ticket) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                              // every wave's slab stores have left; the LDS is no longer read
    unsigned* tk = reinterpret_cast<unsigned*>(smem);
    if (threadIdx.x == 0) tk[0] = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (tk[0] != gridDim.y - 1) return false;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // all arrivals of this launch are in: re-arm
    return true;
}
// (3) sum the quad at src of slab 0 over the gridDim.y <= 8 slabs, in slab order.  Compiler-visible agent-scope loads, NOT inline asm: an asm
// load's destination registers are unprotected until one's own wait -- the register allocator re-used them for the next address while the
// load was in flight: a memory fault on the box
LRP_DEVICE f32x4 ls_sum_quad(const float* src, int64_t slab_stride) {
    const unsigned nsp = gridDim.y;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < (int)nsp) {
            uint64_t* s8 = reinterpret_cast<uint64_t*>(const_cast<float*>(src + (int64_t)k * slab_stride));
            const f32x2 lo = __builtin_bit_cast(f32x2, __hip_atomic_load(s8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const f32x2 hi2 = __builtin_bit_cast(f32x2, __hip_atomic_load(s8 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const f32x4 pk = {lo[0], lo[1], hi2[0], hi2[1]};
            v = (k == 0) ? pk : v + pk;
        }
    return v;
}
// ... and write a quad at element `at` of an fp32 or bf16 (RNE) matrix
LRP_DEVICE void ls_store_quad(void* out, int64_t at, int f32, f32x4 v) {
    if (f32) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + at) = v;
    else {
        bf16x4 o = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
        *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16_t*>(out) + at) = o;
    }
}

// ---- forward epilogue: lane holds z[16 i + (l & 15)][n0 + rw w + 4 (l >> 4) + e] (n0: the workgroup's first column, rw live columns per wave).
// tickets != NULL (TO = float, z = the slab workspace; the host guarantees whole, aligned quads: rw = 16, N % 64 == 0): split K, the sum
// (+ bias) goes to fin
template <typename TO, int MBMAX>
LRP_DEVICE void ls_fwd_epilogue(const f32x4 (&acc)[MBMAX], int wave, int n0, int rw, int nb, TO* z, const bf16_t* bias, int M, int N,
                                int64_t ldz, int64_t slab_stride, unsigned* tickets, void* fin, int64_t ldf, int fin_f32) {
    const int lane = threadIdx.x & 63;
    const int c16 = 4 * (lane >> 4);                                  // column of the wave's 16-row block: live while < rw
    const int ncol = n0 + rw * wave + c16;
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (bias) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c16 + e < rw && ncol + e < N) bv[e] = to_f32(bias[ncol + e]);
    }
    const bool vec = (c16 + 3 < rw) && (ncol + 3 < N) && ((ncol & 3) == 0) && ((ldz & 3) == 0) && ((reinterpret_cast<uintptr_t>(z) & 15) == 0);
    if constexpr (sizeof(TO) == 4) {
        if (tickets != nullptr) {
            float* const slab = reinterpret_cast<float*>(z) + (int64_t)blockIdx.y * slab_stride;
#pragma unroll
            for (int i = 0; i < MBMAX; ++i) {
                const int m = 16 * i + (lane & 15);
                if (i < nb && m < M) ls_publish_quad(slab + (int64_t)m * ldz + ncol, acc[i]);
            }
            if (!ls_last_arriver(tickets + blockIdx.x)) return;
#pragma unroll
            for (int i = 0; i < MBMAX; ++i) {
                const int m = 16 * i + (lane & 15);
                if (i < nb && m < M)
                    ls_store_quad(fin, (int64_t)m * ldf + ncol, fin_f32, ls_sum_quad(reinterpret_cast<const float*>(z) + (int64_t)m * ldz + ncol, slab_stride) + bv);
            }
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < MBMAX; ++i) {
        const int m = 16 * i + (lane & 15);
        if (i < nb && m < M) {
            const f32x4 v = acc[i] + bv;
            TO* dst = z + (int64_t)m * ldz + ncol;
            if (vec) ls_store_quad(dst, 0, sizeof(TO) == 4, v);
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c16 + e < rw && ncol + e < N) dst[e] = from_f32<TO>(v[e]);
            }
        }
    }
}

// ---- host policy
// rows of W per wave: the count in 8 .. 16 that covers N in the fewest whole rounds of the 256 CUs (cost = rounds x rows per workgroup; ties
// go to the larger block).  N = 14336: 14 (256 workgroups instead of 224); N = 28672: 14 (512 = two rounds instead of 448 = 1.75).
inline int stream_rows_per_wave(int N) {
    int best = 16, best_cost = ((((N + 63) / 64) + 255) / 256) * 16;
    for (int rw = 15; rw >= 8; --rw) {
        const int wgs = (N + 4 * rw - 1) / (4 * rw), cost = ((wgs + 255) / 256) * rw;
        if (cost < best_cost) { best = rw; best_cost = cost; }
    }
    return best;
}
// K splits of the forward for narrow weights: the smallest count in {2, 3, 4, 6, 8} that puts 192 ... 1024 workgroups of 64 rows on the chip with
// whole 8-tile rings per split (1: the full-K form applies; 0: neither does)
inline int fwd_splits(int N, int K) {
    if (N < 1 || K < 512 || (K % 512)) return 0;
    const int wgs = (N + 63) / 64;
    if (wgs >= 192) return wgs <= 1024 ? 1 : 0;
    if (N % 64) return 0;                                 // whole quads per lane in the slabs: 16 rows per wave
    for (int s_ : {2, 3, 4, 6, 8})
        if (wgs * s_ >= 192 && wgs * s_ <= 1024 && (K % (512 * s_)) == 0) return s_;
    return 0;
}
// dynamic LDS of a forward workgroup: the x ring + four wave-private W rings
template <typename C> constexpr size_t ls_fwd_lds() { return (size_t)C::NBUF * C::XTILE + 4 * (size_t)LS_WD * 2048; }
// the instantiation for M rows: f(LSI<MBMAX>{}) with the smallest MBMAX in {2, 4, 8} that holds ceil(M / 16) row blocks
template <typename F> int ls_with_row_blocks(int M, F&& f) {
    const int nb = (M + 15) / 16;
    if (nb <= 2) return f(LSI<2>{});
    if (nb <= 4) return f(LSI<4>{});
    return f(LSI<8>{});
}

}  // namespace
