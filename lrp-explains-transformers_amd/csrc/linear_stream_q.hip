// linear_stream_q.hip -- the weight-streaming Linear forward of linear_stream.hip with the weight held as MXFP4 (include/lrp_hip_mxfp4.h):
// z[M, N] = x[M, K] . D[N, K]^T (+ bias), D = what lrp_mxfp4_dequant makes of codes [N, K / 2] + scales [N, K / 32], read as 0.53 bytes per element
// instead of a bf16 matrix that a dequant launch wrote first (include/lrp_hip_mxfp4_stream.h).
//
// BIT IDENTITY with lrp_mxfp4_dequant + lrp_linear_stream_fwd_tk is the contract, and the construction is the one of moe_gemm.hpp: the codes are
// decoded between their global load and an LDS write, and the decoded W tile lands in the SAME wave-private LDS image the plain kernel's
// LDS-DMA staging produces ([8 slots][16 rows][128 B], 16-byte chunk c of row r at c ^ (r & 7)).  Everything after that image is
// linear_stream.hpp's, the code the plain kernel runs: the fragment addresses, a K tile's multiply (ls_tile_mma) and the policy
// (stream_rows_per_wave, fwd_splits, the row-block ladder).  Two parts the plain kernel has written out in linear_stream.hip, and bit identity
// holds only while they say the same there and here: the x stager (stage_x below) and the epilogue with its K splits (ls_fwd_epilogue: bias,
// slab order, tickets).  A CHANGE TO EITHER IS MADE IN BOTH PLACES; tests/test_mxfp4_stream_gpu.py compares the two kernels bit for bit.
//
// What differs is how W travels:
//   * a GROUP is 4 K tiles = 256 K elements = one 128-byte line of codes per row.  A wave instruction loads 8 rows x 8 lanes x 16 B: FULL lines
//     per row visit (the lesson of version 1 of the plain kernel), two instructions for the wave's 16 rows, plus one 4-byte load per lane for the
//     row's scale bytes of its half of the group (4 bytes = 128 K elements; never a byte load per block);
//   * the codes wait in REGISTERS: a ring of LQ_RD = 8 groups (16 x 1 KiB = 16 KiB of codes in flight per wave, the bytes the plain kernel keeps
//     in flight -- 4 x deeper in K), 80 VGPRs.  They are inline-asm buffer loads: beside the x ring's LDS-DMA hipcc would wait vmcnt(0) at the
//     first use of a load it counts, so these are counted by hand with the x stages (loads retire in order: "x(t) has landed" covers every older code load);
//   * x is staged 2 K tiles ahead at MBMAX = 2 (the plain kernel: 3), which makes the workgroup's LDS half a CU's: two workgroups per CU (LQCfg);
//   * the LDS ring's two halves (slots 0..3 / 4..7) alternate: while group g is multiplied out of one half, group g + 1 is decoded into the
//     other, a quarter per K tile (2 code words = 8 v_cvt_scalef32_pk_bf16_fp4 + 2 ds_write_b128 per lane and tile, behind the tile's MFMAs, where no
//     hand-counted ds_read is outstanding).  The ring is wave-private and a wave's LDS operations complete in order: no barrier guards it;
//   * nothing is peeled: a load past the split's K range, or of a row past rw / N (x: past M), goes out with a voffset beyond num_records -- it
//     fetches nothing and returns zero -- so every wait count is one constant.
#include "linear_stream.hpp"

extern "C" int lrp_linear_stream_ok(int M, int N, int K, int64_t ldx, int64_t ldw);

namespace {

constexpr int LQ_GT = 4;       // K tiles per group (one 128-byte line of codes per row); the LDS ring's LS_WD slots are two halves of one group each
constexpr int LQ_RD = 8;       // groups of codes in registers per wave

// x prefetch distance in K tiles: the plain kernel's 3, but 2 at MBMAX = 2 -- a ring of 4 x 4 KiB beside the 64 KiB of W rings is 80 KiB, HALF
// the CU's LDS, so two workgroups share a CU.  At a quarter of the plain kernel's bytes per tile the kernel is bound by the serial chain of a
// K tile (barrier, fragment reads, dependent MFMAs, decode) at one wave per SIMD, not by HBM; a second resident workgroup overlaps two chains
// (measured: [28672, 4096], 512 workgroups, 41.4 -> 33.5 us; staging x 11 tiles ahead instead moved nothing)
template <int MBMAX> struct LQCfg : LSCfg<MBMAX, MBMAX == 2 ? 2 : 3> {
    using B = LSCfg<MBMAX, MBMAX == 2 ? 2 : 3>;
    static constexpr int XD = B::XD, P = B::P;
    // is there a group end (its 4 loads: 2 codes, 2 scales) between the x stages of tiles u + XD and u + 1 + XD?  After tile u = 3 (mod 4)
    static constexpr bool group_end(int u) { return ((u % LQ_GT) + LQ_GT) % LQ_GT == LQ_GT - 1; }
    // VMEM operations younger than x(t) at the wait of tile t = s4 (mod 4): the x stages of tiles t - XD + 1 .. t, and the loads of the group
    // ends among tiles t - XD .. t - 1
    static constexpr int vmc(int s4) {
        int c = XD * P;
        for (int j = 1; j <= XD; ++j) c += group_end(s4 - j) ? 4 : 0;
        return c;
    }
    // the prologue stages x(0 .. XD - 1); the counts above hold from tile 0 on if it too has a group's 4 loads wherever the steady state has a
    // group end between two x stages: behind x(v) when group_end(v - XD).  ge_upto(v) = such places up to and including v; NGE = all of them
    static constexpr int ge_upto(int v) {
        int c = 0;
        for (int w = 0; w <= v; ++w) c += group_end(w - XD) ? 1 : 0;
        return c;
    }
    static constexpr int NGE = ge_upto(XD - 1);
};

// loads hipcc does not count (file header): the destination is named again, "+v", by the wait that retires it, before anything reads it
#define LQ_LD16(dst, vo, rs, so) asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen nt" : "=v"(dst) : "v"(vo), "s"(rs), "s"(so) : "memory")
#define LQ_LD4(dst, vo, rs, so) asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "=v"(dst) : "v"(vo), "s"(rs), "s"(so) : "memory")

LRP_DEVICE u32x4 lq_rsrc(const void* p, int64_t bytes) {
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    return u32x4{(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a), (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((a >> 32) & 0xffff)),
                 (uint32_t)__builtin_amdgcn_readfirstlane((int)bytes), 0x00020000u};
}

template <typename TO, int MBMAX>
__global__ __launch_bounds__(256, 1) void linear_stream_q_fwd_kernel(
    const bf16_t* __restrict__ x, const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, TO* __restrict__ z,
    const bf16_t* __restrict__ bias, int M, int N, int K, int64_t ldx, int64_t ldc, int64_t ldsc, int64_t ldz, int rw, int kt_per_split,
    int64_t slab_stride, unsigned* __restrict__ tickets, void* __restrict__ fin, int64_t ldf, int fin_f32) {
    using C = LQCfg<MBMAX>;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n0 = blockIdx.x * (4 * rw);
    const int kt0 = (int)blockIdx.y * kt_per_split;
    const int nkt = (gridDim.y > 1) ? kt_per_split : K / LS_KT;
    const int nG = nkt / LQ_GT;                                       // even: K (and a split's share) is a multiple of 512
    const int g0 = kt0 / LQ_GT;
    int nb = (M + 15) >> 4;
    nb = nb > MBMAX ? MBMAX : nb;

    // ---- W: piece p of a group = rows 8 p + (l >> 3) of the wave's 16, the 16 bytes (32 elements, one scale block) l & 7 of the row's line
    const u32x4 rsC = lq_rsrc(codes, (int64_t)(N - 1) * ldc + K / 2);
    const u32x4 rsS = lq_rsrc(scales, (int64_t)(N - 1) * ldsc + K / 32);
    const int prow = lane >> 3, pslot = lane & 7;
    const int wrow0 = n0 + rw * wave;
    int voC[2], voS[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const bool live = (8 * p + prow < rw) && (wrow0 + 8 * p + prow < N);         // rows rw .. 15 and rows past N: never fetched, never stored
        voC[p] = live ? (int)((int64_t)(wrow0 + 8 * p + prow) * ldc) + (pslot << 4) : LS_OOB;
        voS[p] = live ? (int)((int64_t)(wrow0 + 8 * p + prow) * ldsc) + ((pslot >> 2) << 2) : LS_OOB;
    }
    const uint32_t esh = (uint32_t)((pslot & 3) << 3);                 // the lane's scale byte inside its 4-byte load
    u32x4 cq[LQ_RD][2];
    uint32_t sq[LQ_RD][2];
    // codes and scales of group g (relative to the split) into register slot j; past the split's range: nothing is fetched
    auto load_g = [&](auto jc, int g) {
        constexpr int j = decltype(jc)::value;
        (void)&cq; (void)&sq; (void)&rsC; (void)&rsS;
        const bool in = g < nG;
        const int soc = (g0 + g) * 128, sos = (g0 + g) * 8;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int vc = in ? voC[p] : LS_OOB, vs = in ? voS[p] : LS_OOB;
            LQ_LD16(cq[j][p], vc, rsC, soc);
            LQ_LD4(sq[j][p], vs, rsS, sos);
        }
    };
    // ---- the decoded image: the lane's 32 elements are K tile (l & 7) >> 1 of the group, chunks 4 (l & 1) + d (d = code word) of row 8 p + prow
    char* const wring = smem + C::NBUF * C::XTILE + wave * (LS_WD * 2048);       // [LS_WD tiles][16 rows][128 B], wave-private
    const uint32_t wst = (uint32_t)((pslot >> 1) * 2048 + prow * 128) + (uint32_t)((((pslot & 1) << 2) ^ prow) << 4);
    // quarter d (code word d of both pieces) of register slot j into ring half `half`
    auto decode_q = [&](auto jc, auto dc, auto hc) {
        constexpr int j = decltype(jc)::value, d = decltype(dc)::value, half = decltype(hc)::value;
        (void)&cq; (void)&sq;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            __attribute__((aligned(16))) bf16_t vals[8];
            mx_decode8(cq[j][p][d], (sq[j][p] >> esh) & 0xffu, vals);
            *reinterpret_cast<u32x4*>(wring + half * (LQ_GT * 2048) + p * 1024 + (wst ^ (uint32_t)(d << 4))) = *reinterpret_cast<const u32x4*>(vals);
        }
    };

    // ---- x: past the split's K range nothing is fetched
    const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (int)(((int64_t)(M - 1) * ldx + K) * 2), 0x00020000);
    const int voX = (int)(prow * ldx * 2) + ((pslot ^ prow) << 4);
    // (linear_stream.hip's stage_x + the range test: they change together)
    auto stage_x = [&](int kt, int buf) {
        const int vo = kt < nkt ? voX : LS_OOB;
#pragma unroll
        for (int p = 0; p < C::P; ++p) {
            const int q = wave * C::P + p;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsX, (ls_lds_ptr_t)(smem + buf * C::XTILE + q * 1024), 16, vo,
                                                     (int)((int64_t)(8 * q) * ldx * 2) + (kt + kt0) * 128, 0, 0);
        }
    };
    uint32_t cX[2], cW[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) cX[ks] = ls_frag_x(lane, ks);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) cW[ks] = cX[ks] + ls_w_ring<C>(wave);
    f32x4 acc[MBMAX];
#pragma unroll
    for (int i = 0; i < MBMAX; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- prologue: codes(0 .. RD - NGE); group 0 decoded whole; x(0 .. XD - 1) with codes(RD - NGE + 1 .. RD) at the group-end places between
    // them (the last one, behind x(XD - 1), refills slot 0) -- the order the steady state continues
    ls_for<0, LQ_RD - C::NGE + 1>([&](auto jc) { load_g(jc, decltype(jc)::value); });
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(%[cnt])" : "+v"(cq[0][0]), "+v"(cq[0][1]), "+v"(sq[0][0]), "+v"(sq[0][1]) : [cnt] "n"(4 * (LQ_RD - C::NGE)) : "memory");
    __builtin_amdgcn_sched_barrier(0);
    ls_for<0, 4>([&](auto dc) { decode_q(LSI<0>{}, dc, LSI<0>{}); });
    __builtin_amdgcn_sched_barrier(0);
    ls_for<0, C::XD>([&](auto vc) {
        constexpr int v = decltype(vc)::value;
        stage_x(v, v);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (C::group_end(v - C::XD)) {
            constexpr int g = LQ_RD - C::NGE + C::ge_upto(v);
            load_g(LSI<g % LQ_RD>{}, g);
            __builtin_amdgcn_sched_barrier(0);
        }
    });

    // one K tile t = 4 g + s4 of the group in register slot j (ring half j & 1); behind its MFMAs, quarter s4 of group g + 1 is decoded
    auto tile = [&](auto jc, auto s4c, int t) {
        constexpr int j = decltype(jc)::value, s4 = decltype(s4c)::value, j1 = (j + 1) % LQ_RD, s = LQ_GT * (j & 1) + s4;
        (void)&cq; (void)&sq; (void)&cW;
        stage_x(t + C::XD, (t + C::XD) % C::NBUF);
        __builtin_amdgcn_sched_barrier(0);
        // x(t) has landed, and with it every older load: at a group's first tile that names the next group's codes and scales
        if constexpr (s4 == 0)
            asm volatile("s_waitcnt vmcnt(%[cnt])" : "+v"(cq[j1][0]), "+v"(cq[j1][1]), "+v"(sq[j1][0]), "+v"(sq[j1][1]) : [cnt] "n"(C::vmc(s4)) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(%[cnt])" :: [cnt] "n"(C::vmc(s4)) : "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        ls_tile_mma<C>(cX, cW, (uint32_t)((t % C::NBUF) * C::XTILE), LSI<s>{}, acc, nb);
        // no hand-counted ds_read is outstanding here (the last unit waited lgkmcnt(0)): the compiler's own ds_writes cannot disturb a count
        decode_q(LSI<j1>{}, s4c, LSI<(j1 & 1)>{});
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (s4 == LQ_GT - 1) {
            load_g(LSI<j1>{}, t / LQ_GT + 1 + LQ_RD);                 // slot j1 is decoded whole: refill it, LQ_RD groups ahead
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    for (int G = 0; G < nG; G += LQ_RD)
        ls_for<0, LQ_RD / 2>([&](auto hc) {
            constexpr int h = decltype(hc)::value;
            if (G + 2 * h < nG) {
                ls_for<0, LQ_GT>([&](auto s4c) { tile(LSI<2 * h>{}, s4c, (G + 2 * h) * LQ_GT + decltype(s4c)::value); });
                ls_for<0, LQ_GT>([&](auto s4c) { tile(LSI<2 * h + 1>{}, s4c, (G + 2 * h + 1) * LQ_GT + decltype(s4c)::value); });
            }
        });
    // the loads still outstanding fetched nothing (past the K range); they are retired before the registers and the LDS go back
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    ls_fwd_epilogue<TO, MBMAX>(acc, wave, n0, rw, nb, z, bias, M, N, ldz, slab_stride, tickets, fin, ldf, fin_f32);
}

template <typename TO, int MBMAX>
int launch_q(const void* x, const void* codes, const void* scales, const void* bias, void* z, int M, int N, int K, int64_t ldx, int64_t ldc,
             int64_t ldsc, int64_t ldz, hipStream_t st) {
    const size_t lds = ls_fwd_lds<LQCfg<MBMAX>>();
    auto kern = linear_stream_q_fwd_kernel<TO, MBMAX>;
    LRP_SET_MAX_LDS(kern, lds);
    const int rw = stream_rows_per_wave(N);
    hipLaunchKernelGGL(kern, dim3((N + 4 * rw - 1) / (4 * rw)), dim3(256), lds, st, (const bf16_t*)x, (const uint8_t*)codes, (const uint8_t*)scales,
                       (TO*)z, (const bf16_t*)bias, M, N, K, ldx, ldc, ldsc, ldz, rw, 0, (int64_t)0, (unsigned*)nullptr, (void*)nullptr, (int64_t)0, 0);
    return lrp_check_launch();
}

// split form: fp32 slabs [splits][M][N] in ws, summed in-kernel by the last arriver of each 64-row block into z
template <int MBMAX>
int launch_q_split(const void* x, const void* codes, const void* scales, const void* bias, void* z, int M, int N, int K, int64_t ldx, int64_t ldc,
                   int64_t ldsc, int64_t ldz, int out_f32, int splits, void* ws, unsigned* tickets, hipStream_t st) {
    const size_t lds = ls_fwd_lds<LQCfg<MBMAX>>();
    auto kern = linear_stream_q_fwd_kernel<float, MBMAX>;
    LRP_SET_MAX_LDS(kern, lds);
    hipLaunchKernelGGL(kern, dim3(N / 64, splits), dim3(256), lds, st, (const bf16_t*)x, (const uint8_t*)codes, (const uint8_t*)scales, (float*)ws,
                       (const bf16_t*)bias, M, N, K, ldx, ldc, ldsc, (int64_t)N, 16, K / LS_KT / splits, (int64_t)M * N, tickets, z, ldz, out_f32);
    return lrp_check_launch();
}

// the shape the kernel can address: the plain entry's domain on the dequantised matrix, the pitches at least a row, byte offsets inside 2^30
bool q_shape(int M, int N, int K, int64_t ldx, int64_t ldc, int64_t ldsc) {
    if (M < 1 || M > 128 || N < 1 || K < 512 || (K % 512) || ldx < K || ldc < K / 2 || ldsc < K / 32) return false;
    return (int64_t)N * K < (1ll << 30) && (int64_t)M * ldx < (1ll << 30) && (int64_t)N * ldc < (1ll << 30) && (int64_t)N * ldsc < (1ll << 30);
}

}  // namespace

extern "C" int lrp_linear_stream_q_ok(int M, int N, int K, int64_t ldx, int64_t ldc, int64_t ldsc) {
    if (!q_shape(M, N, K, ldx, ldc, ldsc) || (ldx % 8) || (ldc % 16) || (ldsc % 4)) return 0;
    return lrp_linear_stream_ok(M, N, K, ldx, K);
}

extern "C" int lrp_linear_stream_fwd_q(const void* x, const void* codes, const void* scales, const void* bias, void* z, int M, int N, int K,
                                       int64_t ldx, int64_t ldc, int64_t ldsc, int64_t ldz, int dtype, int out_dtype, void* ws, void* tickets,
                                       void* stream) {
    if (!x || !codes || !scales || !z || M < 0 || N < 0 || K < 0) return LRP_EINVAL;
    if ((dtype != LRP_BF16 && dtype != LRP_F32) || (out_dtype != LRP_BF16 && out_dtype != LRP_F32)) return LRP_EINVAL;
    if (M == 0 || N == 0) return LRP_OK;
    if (dtype != LRP_BF16 || !q_shape(M, N, K, ldx, ldc, ldsc)) return LRP_ESHAPE;
    if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(codes) & 15) || (ldx % 8) || (ldc % 16)) return LRP_EALIGN;
    if ((reinterpret_cast<uintptr_t>(scales) & 3) || (ldsc % 4)) return LRP_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int splits = (ws && tickets) ? fwd_splits(N, K) : 1;          // without the scratch: the full-K form, as in the plain entry
    if (splits > 1) {
        if ((reinterpret_cast<uintptr_t>(z) & 15) || (ldz % 4) || (reinterpret_cast<uintptr_t>(ws) & 15)) return LRP_EALIGN;
        const int f32o = out_dtype == LRP_F32 ? 1 : 0;
        return ls_with_row_blocks(M, [&](auto mb) {
            return launch_q_split<decltype(mb)::value>(x, codes, scales, bias, z, M, N, K, ldx, ldc, ldsc, ldz, f32o, splits, ws, (unsigned*)tickets, st);
        });
    }
    return ls_with_row_blocks(M, [&](auto mb) {
        constexpr int MB = decltype(mb)::value;
        if (out_dtype == LRP_F32) return launch_q<float, MB>(x, codes, scales, bias, z, M, N, K, ldx, ldc, ldsc, ldz, st);
        return launch_q<bf16_t, MB>(x, codes, scales, bias, z, M, N, K, ldx, ldc, ldsc, ldz, st);
    });
}
