// attnmap.hip -- token-to-token attention relevance maps (include/lrp_hip_latent.h: lrp_attn_relmap, lrp_attn_relmap_d256).
//
// out[b, i, j] = gscale sum_{h_lo <= h < h_hi} P_h[i, j] (g_h[i] . v_{h / rep}[j]),  P_h[i, j] = exp(scale q_h[i] . k_{h / rep}[j] - lse[b, h, i])
// for the (i, j) the mask lets through (causal, per-row key intervals), exactly 0 elsewhere: `attn_weights * attn_weights.grad` of eager
// attention, recomputed tile by tile from what the flash-style kernels keep (rotated q / k, v, the o projection's input gradient, lse).
//
// A workgroup owns one AM_T x AM_T tile of one prompt's [S, S] map, counted from the prompt's first row, and walks the heads of the range in
// ascending order; the tile's sum over heads lives in fp32 registers, goes through an LDS tile once and leaves as runs along j (plain vector
// stores, every element of out written exactly once: no atomics, no workspace, bitwise repeatable, batch invariant).  A tile that no row of
// it can see (above the diagonal, or outside the union of its rows' key intervals) is written as zeros without loading an operand.
// Both contractions run over d, the contiguous dimension of all four operands, so every MFMA fragment is a 16-byte run of a token-major row.
// Masked elements are SELECTED to 0, never multiplied: an invisible score may exponentiate to inf, and a row whose interval is empty
// (lse = -inf) must give 0, not NaN.
#include <limits.h>
#include "common.hpp"

namespace {

constexpr int AM_T = 64;                 // tile edge: 4 waves x 16 query rows, 4 blocks of 16 keys
constexpr float AM_LOG2E = 1.4426950408889634f;

// the rows' effective key intervals [lo, hi) of one tile (the causal bound folded in, empty -> [0, 0)) and whether any of them reaches
// the tile's keys [j0, j0 + AM_T).  Ends with a barrier: s_lo / s_hi are readable by every thread afterwards.
LRP_DEVICE bool am_tile_rows(int* s_lo, int* s_hi, const int* __restrict__ row_lo, const int* __restrict__ row_hi, int b, int S, int i0, int j0,
                             int causal) {
    const int t = threadIdx.x;
    if (t < AM_T) {
        const int i = i0 + t;
        int lo = 0, hi = 0;
        if (i < S) {
            hi = S;
            if (row_lo) {
                lo = max(row_lo[(int64_t)b * S + i], 0);
                hi = min(row_hi[(int64_t)b * S + i], S);
            }
            if (causal) hi = min(hi, i + 1);
        }
        if (hi <= lo) lo = hi = 0;
        s_lo[t] = lo;
        s_hi[t] = hi;
    }
    __syncthreads();
    int ulo = INT_MAX, uhi = 0;
    for (int r = 0; r < AM_T; ++r) {
        if (s_hi[r] > s_lo[r]) {
            ulo = min(ulo, s_lo[r]);
            uhi = max(uhi, s_hi[r]);
        }
    }
    return max(ulo, j0) < min(uhi, j0 + AM_T);
}

// the tile leaves as runs of AM_T floats along j; so == nullptr: zeros (a dead tile)
template <int NT = 256>
LRP_DEVICE void am_store_tile(float* __restrict__ out, const float (*so)[AM_T + 1], int b, int S, int i0, int j0) {
    for (int e = threadIdx.x; e < AM_T * AM_T; e += NT) {
        const int r = e / AM_T, c = e - r * AM_T;
        if (i0 + r < S && j0 + c < S) out[((int64_t)b * S + i0 + r) * S + j0 + c] = so ? so[r][c] : 0.f;
    }
}

// ---- bf16, d = D in {64, 128}: both contractions on v_mfma_f32_16x16x32_bf16, fp32 from the accumulators to the store (P and G_P are never
// rounded).  The K and V tiles of a kv head are staged in LDS once and serve the rep query heads of its group; the q and g fragments of a
// wave's 16 rows come straight from global memory (each wave reads its own rows only).  Keys are the MFMA's FIRST operand, so lane l ends up
// with keys (l >> 4) * 4 + r of query l & 15: one lse and one key interval per lane.
template <int D>
__global__ __launch_bounds__(256) void attn_relmap_bf16_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                               const bf16_t* __restrict__ v, const bf16_t* __restrict__ g,
                                                               const float* __restrict__ lse, float* __restrict__ out, int S, int Hq, int rep,
                                                               int h_lo, int h_hi, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldg,
                                                               float scale, float gscale, int causal, const int* __restrict__ row_lo,
                                                               const int* __restrict__ row_hi, int T) {
    constexpr int P = D + 8;            // LDS row pitch (elements): 16 more bytes, the 16 rows of a fragment read spread over the banks
    constexpr int KK = D / 32;          // MFMA steps of one contraction
    __shared__ __attribute__((aligned(16))) bf16_t sk[AM_T * P];
    __shared__ __attribute__((aligned(16))) bf16_t sv[AM_T * P];
    __shared__ float so[AM_T][AM_T + 1];
    __shared__ int s_lo[AM_T], s_hi[AM_T];
    const int b = blockIdx.y, ti = blockIdx.x / T, tj = blockIdx.x - ti * T;
    const int i0 = ti * AM_T, j0 = tj * AM_T;
    if (!am_tile_rows(s_lo, s_hi, row_lo, row_hi, b, S, i0, j0, causal)) {
        am_store_tile(out, nullptr, b, S, i0, j0);
        return;
    }
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, lr = lane & 15, lg = lane >> 4;
    const int il = wave * 16 + lr;                         // this lane's query row inside the tile
    const int64_t irow = (int64_t)b * S + min(i0 + il, S - 1);          // (rows past S: re-read the last one, masked by their empty interval)
    const int my_lo = s_lo[il], my_hi = s_hi[il];
    const float c1 = scale * AM_LOG2E;
    f32x4 tot[4];
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) tot[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
    int cur = -1;
    for (int h = h_lo; h < h_hi; ++h) {
        const int kvh = h / rep;
        if (kvh != cur) {
            __syncthreads();                               // (every wave is done with the previous group's tiles)
            for (int e = t; e < AM_T * (D / 8); e += 256) {
                const int r = e / (D / 8), c = (e - r * (D / 8)) * 8;
                const int64_t jrow = (int64_t)b * S + min(j0 + r, S - 1);
                *reinterpret_cast<bf16x8*>(&sk[r * P + c]) = *reinterpret_cast<const bf16x8*>(k + jrow * ldk + (int64_t)kvh * D + c);
                *reinterpret_cast<bf16x8*>(&sv[r * P + c]) = *reinterpret_cast<const bf16x8*>(v + jrow * ldv + (int64_t)kvh * D + c);
            }
            __syncthreads();
            cur = kvh;
        }
        bf16x8 qf[KK], gf[KK];
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            qf[kk] = *reinterpret_cast<const bf16x8*>(q + irow * ldq + (int64_t)h * D + kk * 32 + lg * 8);
            gf[kk] = *reinterpret_cast<const bf16x8*>(g + irow * ldg + (int64_t)h * D + kk * 32 + lg * 8);
        }
        const float l = lse[((int64_t)b * Hq + h) * S + min(i0 + il, S - 1)];
        const bool row_ok = l > -INFINITY;
        const float l2 = l * AM_LOG2E;
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, gp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const int off = (jb * 16 + lr) * P + kk * 32 + lg * 8;
                s = Mma16<bf16_t>::mma(*reinterpret_cast<const bf16x8*>(&sk[off]), qf[kk], s);
                gp = Mma16<bf16_t>::mma(*reinterpret_cast<const bf16x8*>(&sv[off]), gf[kk], gp);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + jb * 16 + lg * 4 + r;
                const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c1, -l2));
                tot[jb][r] += (row_ok && j >= my_lo && j < my_hi) ? p * gp[r] : 0.f;
            }
        }
    }
#pragma unroll
    for (int jb = 0; jb < 4; ++jb)
#pragma unroll
        for (int r = 0; r < 4; ++r) so[il][jb * 16 + lg * 4 + r] = tot[jb][r] * gscale;
    __syncthreads();
    am_store_tile(out, so, b, S, i0, j0);
}

// ---- bf16, d = 256 (Gemma-3): the contraction of the kernel above, with K and V staged in TWO panels of 128 columns.  A full-width pair of
// tiles (2 x 64 x 264 bf16) plus the output tile is ~84 KB of LDS: one workgroup per CU, one wave per SIMD, nothing to hide the q / g / lse
// loads behind.  A panel pair is 34 KB, and the output tile reuses it after the last head, so LDS admits four workgroups per CU.  The price
// is that the fp32 accumulators s and gp of the heads that share the staged panel live across the two panels: RC heads x 4 key blocks x
// (s, gp) x 4 registers.  A staging serves min(rep, RC) query heads of one kv group: all of them for rep <= 4 (Gemma-3: 2 and 4); a wider
// group is walked in chunks of RC heads and staged once per chunk.  To keep that register set small the tile is shared by EIGHT waves: wave
// w owns the 16 query rows (w & 3) * 16.. and the 32 keys (w >> 2) * 32.. (two key blocks, not four), which halves the accumulators per
// wave; the two waves of a row group read the same q / g fragments (the second read is a cache hit).  The MFMA steps of a head run in the
// order of d (panel 0: kk 0..3, panel 1: kk 4..7) and the heads are added to the tile in ascending order, so the sums are those of a
// single-pass kernel.
constexpr int AM_PD = 128;               // panel width (columns of d)
constexpr int AM_NT8 = 512;              // threads of the eight-wave workgroup

template <int RC>
__global__ __launch_bounds__(AM_NT8) void attn_relmap_bf16_d256_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                                    const bf16_t* __restrict__ v, const bf16_t* __restrict__ g,
                                                                    const float* __restrict__ lse, float* __restrict__ out, int S, int Hq,
                                                                    int rep, int h_lo, int h_hi, int64_t ldq, int64_t ldk, int64_t ldv,
                                                                    int64_t ldg, float scale, float gscale, int causal,
                                                                    const int* __restrict__ row_lo, const int* __restrict__ row_hi, int T) {
    constexpr int D = 256;
    constexpr int P = AM_PD + 8;        // LDS row pitch (elements), as above
    constexpr int KK = AM_PD / 32;      // MFMA steps of one panel
    constexpr int TILE = AM_T * P;      // elements of one staged panel
    static_assert(2 * TILE * sizeof(bf16_t) >= AM_T * (AM_T + 1) * sizeof(float), "the output tile reuses the panels' LDS");
    __shared__ __attribute__((aligned(16))) bf16_t skv[2 * TILE];
    __shared__ int s_lo[AM_T], s_hi[AM_T];
    bf16_t* sk = skv;
    bf16_t* sv = skv + TILE;
    float(*so)[AM_T + 1] = reinterpret_cast<float(*)[AM_T + 1]>(skv);
    const int b = blockIdx.y, ti = blockIdx.x / T, tj = blockIdx.x - ti * T;
    const int i0 = ti * AM_T, j0 = tj * AM_T;
    if (!am_tile_rows(s_lo, s_hi, row_lo, row_hi, b, S, i0, j0, causal)) {
        am_store_tile<AM_NT8>(out, nullptr, b, S, i0, j0);
        return;
    }
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, lr = lane & 15, lg = lane >> 4;
    const int il = (wave & 3) * 16 + lr;                   // this lane's query row inside the tile
    const int jw = (wave >> 2) * 2;                        // this wave's first key block
    const int64_t irow = (int64_t)b * S + min(i0 + il, S - 1);
    const int my_lo = s_lo[il], my_hi = s_hi[il];
    const float c1 = scale * AM_LOG2E;
    f32x4 tot[2];
#pragma unroll
    for (int jb = 0; jb < 2; ++jb) tot[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int h0 = h_lo; h0 < h_hi;) {
        const int kvh = h0 / rep;
        const int nh = min(min((kvh + 1) * rep, h_hi) - h0, RC);          // heads of this chunk: one kv head, uniform over the workgroup
        f32x4 s[RC][2], gp[RC][2];
#pragma unroll
        for (int c = 0; c < RC; ++c)
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) s[c][jb] = gp[c][jb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int pn = 0; pn < D / AM_PD; ++pn) {
            __syncthreads();                               // (every wave is done with the previous panel)
            for (int e = t; e < AM_T * (AM_PD / 8); e += AM_NT8) {
                const int r = e / (AM_PD / 8), c = (e - r * (AM_PD / 8)) * 8;
                const int64_t jrow = (int64_t)b * S + min(j0 + r, S - 1);
                *reinterpret_cast<bf16x8*>(&sk[r * P + c]) = *reinterpret_cast<const bf16x8*>(k + jrow * ldk + (int64_t)kvh * D + pn * AM_PD + c);
                *reinterpret_cast<bf16x8*>(&sv[r * P + c]) = *reinterpret_cast<const bf16x8*>(v + jrow * ldv + (int64_t)kvh * D + pn * AM_PD + c);
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < RC; ++c) {
                if (c < nh) {
                    bf16x8 qf[KK], gf[KK];
#pragma unroll
                    for (int kk = 0; kk < KK; ++kk) {
                        qf[kk] = *reinterpret_cast<const bf16x8*>(q + irow * ldq + (int64_t)(h0 + c) * D + pn * AM_PD + kk * 32 + lg * 8);
                        gf[kk] = *reinterpret_cast<const bf16x8*>(g + irow * ldg + (int64_t)(h0 + c) * D + pn * AM_PD + kk * 32 + lg * 8);
                    }
#pragma unroll
                    for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                        for (int kk = 0; kk < KK; ++kk) {
                            const int off = ((jw + jb) * 16 + lr) * P + kk * 32 + lg * 8;
                            s[c][jb] = Mma16<bf16_t>::mma(*reinterpret_cast<const bf16x8*>(&sk[off]), qf[kk], s[c][jb]);
                            gp[c][jb] = Mma16<bf16_t>::mma(*reinterpret_cast<const bf16x8*>(&sv[off]), gf[kk], gp[c][jb]);
                        }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < RC; ++c) {
            if (c < nh) {
                const float l = lse[((int64_t)b * Hq + h0 + c) * S + min(i0 + il, S - 1)];
                const bool row_ok = l > -INFINITY;
                const float l2 = l * AM_LOG2E;
#pragma unroll
                for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = j0 + (jw + jb) * 16 + lg * 4 + r;
                        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[c][jb][r], c1, -l2));
                        tot[jb][r] += (row_ok && j >= my_lo && j < my_hi) ? p * gp[c][jb][r] : 0.f;
                    }
            }
        }
        h0 += nh;
    }
    __syncthreads();                                       // (every wave is done with the last panel: its LDS becomes the output tile)
#pragma unroll
    for (int jb = 0; jb < 2; ++jb)
#pragma unroll
        for (int r = 0; r < 4; ++r) so[il][(jw + jb) * 16 + lg * 4 + r] = tot[jb][r] * gscale;
    __syncthreads();
    am_store_tile<AM_NT8>(out, so, b, S, i0, j0);
}

// ---- fp32, any d <= 256 that is a multiple of 4 (the parity path): LDS tiles of AM_DK columns of the four operands, a thread owns a 4 x 4
// sub-grid of the tile (rows ty + 16 a, keys tx + 16 c) and adds the products in the order of d; expf, not the hardware exp2.
constexpr int AM_DK = 32;

__global__ __launch_bounds__(256) void attn_relmap_f32_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                              const float* __restrict__ g, const float* __restrict__ lse, float* __restrict__ out,
                                                              int S, int Hq, int rep, int d, int h_lo, int h_hi, int64_t ldq, int64_t ldk,
                                                              int64_t ldv, int64_t ldg, float scale, float gscale, int causal,
                                                              const int* __restrict__ row_lo, const int* __restrict__ row_hi, int T) {
    constexpr int P = AM_DK + 1;
    __shared__ float sq[AM_T * P], sg[AM_T * P], sk[AM_T * P], sv[AM_T * P];
    __shared__ float so[AM_T][AM_T + 1];
    __shared__ int s_lo[AM_T], s_hi[AM_T];
    const int b = blockIdx.y, ti = blockIdx.x / T, tj = blockIdx.x - ti * T;
    const int i0 = ti * AM_T, j0 = tj * AM_T;
    if (!am_tile_rows(s_lo, s_hi, row_lo, row_hi, b, S, i0, j0, causal)) {
        am_store_tile(out, nullptr, b, S, i0, j0);
        return;
    }
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    float tot[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) tot[a][c] = 0.f;
    for (int h = h_lo; h < h_hi; ++h) {
        const int kvh = h / rep;
        float s[4][4], gp[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) s[a][c] = gp[a][c] = 0.f;
        for (int d0 = 0; d0 < d; d0 += AM_DK) {
            __syncthreads();
            for (int e = t; e < AM_T * (AM_DK / 4); e += 256) {
                const int r = e / (AM_DK / 4), c4 = (e - r * (AM_DK / 4)) * 4, col = d0 + c4;
                const int64_t irow = (int64_t)b * S + min(i0 + r, S - 1), jrow = (int64_t)b * S + min(j0 + r, S - 1);
                f32x4 xq = {0.f, 0.f, 0.f, 0.f}, xg = xq, xk = xq, xv = xq;
                if (col < d) {                             // (d is a multiple of 4: the whole vector is inside the head)
                    xq = *reinterpret_cast<const f32x4*>(q + irow * ldq + (int64_t)h * d + col);
                    xg = *reinterpret_cast<const f32x4*>(g + irow * ldg + (int64_t)h * d + col);
                    xk = *reinterpret_cast<const f32x4*>(k + jrow * ldk + (int64_t)kvh * d + col);
                    xv = *reinterpret_cast<const f32x4*>(v + jrow * ldv + (int64_t)kvh * d + col);
                }
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    sq[r * P + c4 + x] = xq[x];
                    sg[r * P + c4 + x] = xg[x];
                    sk[r * P + c4 + x] = xk[x];
                    sv[r * P + c4 + x] = xv[x];
                }
            }
            __syncthreads();
#pragma unroll 4
            for (int c = 0; c < AM_DK; ++c) {
                float qa[4], ga[4], kb[4], vb[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    qa[a] = sq[(ty + 16 * a) * P + c];
                    ga[a] = sg[(ty + 16 * a) * P + c];
                    kb[a] = sk[(tx + 16 * a) * P + c];
                    vb[a] = sv[(tx + 16 * a) * P + c];
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) {
                        s[a][cc] = __builtin_fmaf(qa[a], kb[cc], s[a][cc]);
                        gp[a][cc] = __builtin_fmaf(ga[a], vb[cc], gp[a][cc]);
                    }
            }
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int il = ty + 16 * a;
            const float l = lse[((int64_t)b * Hq + h) * S + min(i0 + il, S - 1)];
            const bool row_ok = l > -INFINITY;
            const int my_lo = s_lo[il], my_hi = s_hi[il];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                const int j = j0 + tx + 16 * cc;
                const float p = expf(s[a][cc] * scale - l);
                tot[a][cc] += (row_ok && j >= my_lo && j < my_hi) ? p * gp[a][cc] : 0.f;
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) so[ty + 16 * a][tx + 16 * cc] = tot[a][cc] * gscale;
    __syncthreads();
    am_store_tile(out, so, b, S, i0, j0);
}

}  // namespace

extern "C" int lrp_attn_relmap(const void* q, const void* k, const void* v, const void* g, const float* lse, float* out, int M, int B, int S,
                               int Hq, int Hkv, int d, int h_lo, int h_hi, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldg, float scale,
                               float gscale, int causal, const int* row_lo, const int* row_hi, int dtype, void* stream) {
    if (!q || !k || !v || !g || !lse || !out || (dtype != LRP_F32 && dtype != LRP_BF16)) return LRP_EINVAL;
    if (B < 1 || S < 1 || (int64_t)B * S != (int64_t)M || Hq < 1 || Hkv < 1 || Hq % Hkv != 0 || h_lo < 0 || h_hi > Hq || h_lo >= h_hi || d < 1 ||
        (dtype == LRP_BF16 ? (d != 64 && d != 128) : (d > 256 || d % 4 != 0)) || ldq < (int64_t)Hq * d || ldg < (int64_t)Hq * d ||
        ldk < (int64_t)Hkv * d || ldv < (int64_t)Hkv * d || (row_lo == nullptr) != (row_hi == nullptr) || B > 65535)
        return LRP_ESHAPE;
    const int64_t T = ((int64_t)S + AM_T - 1) / AM_T;
    if (T * T > INT_MAX) return LRP_ESHAPE;
    const int V = dtype == LRP_BF16 ? 8 : 4;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)g) % 16 || ldq % V || ldk % V || ldv % V || ldg % V ||
        ((uintptr_t)out | (uintptr_t)lse | (uintptr_t)row_lo | (uintptr_t)row_hi) % 4)
        return LRP_EALIGN;
    const dim3 grid((unsigned)(T * T), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    const int rep = Hq / Hkv;
    if (dtype == LRP_F32) {
        hipLaunchKernelGGL(attn_relmap_f32_kernel, grid, dim3(256), 0, st, (const float*)q, (const float*)k, (const float*)v, (const float*)g, lse,
                           out, S, Hq, rep, d, h_lo, h_hi, ldq, ldk, ldv, ldg, scale, gscale, causal, row_lo, row_hi, (int)T);
    } else if (d == 64) {
        hipLaunchKernelGGL(attn_relmap_bf16_kernel<64>, grid, dim3(256), 0, st, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v,
                           (const bf16_t*)g, lse, out, S, Hq, rep, h_lo, h_hi, ldq, ldk, ldv, ldg, scale, gscale, causal, row_lo, row_hi, (int)T);
    } else {
        hipLaunchKernelGGL(attn_relmap_bf16_kernel<128>, grid, dim3(256), 0, st, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v,
                           (const bf16_t*)g, lse, out, S, Hq, rep, h_lo, h_hi, ldq, ldk, ldv, ldg, scale, gscale, causal, row_lo, row_hi, (int)T);
    }
    return lrp_check_launch();
}

extern "C" int lrp_attn_relmap_d256(const void* q, const void* k, const void* v, const void* g, const float* lse, float* out, int M, int B, int S,
                                    int Hq, int Hkv, int d, int h_lo, int h_hi, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldg, float scale,
                                    float gscale, int causal, const int* row_lo, const int* row_hi, int dtype, void* stream) {
    if (!q || !k || !v || !g || !lse || !out || (dtype != LRP_F32 && dtype != LRP_BF16)) return LRP_EINVAL;
    if (B < 1 || S < 1 || (int64_t)B * S != (int64_t)M || Hq < 1 || Hkv < 1 || Hq % Hkv != 0 || h_lo < 0 || h_hi > Hq || h_lo >= h_hi ||
        dtype != LRP_BF16 || d != 256 || ldq < (int64_t)Hq * d || ldg < (int64_t)Hq * d || ldk < (int64_t)Hkv * d || ldv < (int64_t)Hkv * d ||
        (row_lo == nullptr) != (row_hi == nullptr) || B > 65535)
        return LRP_ESHAPE;
    const int64_t T = ((int64_t)S + AM_T - 1) / AM_T;
    if (T * T > INT_MAX) return LRP_ESHAPE;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)g) % 16 || ldq % 8 || ldk % 8 || ldv % 8 || ldg % 8 ||
        ((uintptr_t)out | (uintptr_t)lse | (uintptr_t)row_lo | (uintptr_t)row_hi) % 4)
        return LRP_EALIGN;
    const dim3 grid((unsigned)(T * T), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    const int rep = Hq / Hkv;
#define LRP_RELMAP_D256(RC)                                                                                                                   \
    hipLaunchKernelGGL(attn_relmap_bf16_d256_kernel<RC>, grid, dim3(AM_NT8), 0, st, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v,       \
                       (const bf16_t*)g, lse, out, S, Hq, rep, h_lo, h_hi, ldq, ldk, ldv, ldg, scale, gscale, causal, row_lo, row_hi, (int)T)
    // the heads one staging serves: a single head (rep 1, or a one-head range) needs no second set of accumulators
    const int width = min(rep, h_hi - h_lo);
    if (width == 1) LRP_RELMAP_D256(1);
    else if (width == 2) LRP_RELMAP_D256(2);
    else LRP_RELMAP_D256(4);
#undef LRP_RELMAP_D256
    return lrp_check_launch();
}
