// wgrad_tiles.hpp -- what the two token-contracting GEMMs share: wgrad.hip (dense: lrp_wgrad_rel, lrp_wgrad) and moe_wgrad.hip (grouped:
// lrp_moe_wgrad_rel[_q]).  Both form  acc[n, k] = sum_t s(t) G[row_g(t), n] X[row_x(t), k]  for one 128 x 128 (bf16) or 64 x 64 (fp32) tile of
// the result; they differ in how a token's rows and scale are FOUND (their global-load side and token-loop control flow stay in the .hip
// files) and in what their epilogues do with an accumulator.
// Who calls what.  Both files: the tile constants, the image layout (wg_off), the transposed fragment read (wg_frag_tr), the staging store
// (wg_stage), wf_clear and the host rule wg_shape_ok.  The grouped bf16 kernel alone: wg_clear, wg_mma_tile and wg_for_each.  The dense bf16
// kernel keeps those three written out: called as functions they moved its prologue's address arithmetic, and lrp_wgrad_rel without rs then
// measured 0.6 - 1.0 % over the previous build's own spread in three sessions (profiles/wgrad_tiles_refactor_ab.txt).  As it stands all five
// dense kernels compile to their previous text.  A change to the MFMA block or the lane mapping is made here AND in wgrad.hip.
//
// bf16: one workgroup of 4 waves owns the tile and walks the tokens in tiles of 64.  G and X are token-major, so the contraction index is
// the ROW of both operand tiles: both MFMA operands (8 consecutive tokens of one column) are gathered out of row-major LDS images by two
// ds_read_b64_tr_b16 each (4 token rows per read).
//   LDS (32 KiB, dynamic, nothing static in front of it): [G image][X image], each 64 token rows x 256 B; the 16-byte chunk ch of row r sits
//   at 256 r + 16 (ch ^ (((r & 3) << 2) | ((r >> 2) & 3))).  A 16-lane group of a transposed read takes 4 rows x 32 B, the two groups of a
//   32-lane half are 8 rows apart in the same columns: by the bank rule (bank = (addr / 4) % 64) the xor maps those 8 rows to 64 distinct banks --
//   worked out on paper, not confirmed with a bank-conflict counter.  Every lane's address is 8-byte
//   aligned (chunk base + 0 / 8) and the reads run under a full EXEC mask: rows past M and chunks past N / K are staged as ZEROS, never
//   masked out.
//   Wave w: n rows 64 (w >> 1) .., k columns 64 (w & 1) ..: 4 x 4 tiles of v_mfma_f32_16x16x32_bf16, acc = mfma(X fragment, G fragment), so
//   lane l holds acc[n = .. + (l & 15)][k = .. + 4 (l >> 4) + 0..3] of each 16 x 16 tile.
// fp32 (the parity path): a plain LDS-tiled form, 64 x 64 outputs per workgroup, 4 x 4 per thread, tokens in tiles of 16.  s G X is formed
// exactly and summed in fp64 (the sum carries 2^-53 per step).
#pragma once
#include "common.hpp"

namespace {

typedef __attribute__((ext_vector_type(4))) short wg_s16x4;
typedef __attribute__((ext_vector_type(8))) short wg_s16x8;
typedef __attribute__((address_space(3))) wg_s16x4* wg_lds_s16x4_t;

constexpr int WG_TILE = 128;                      // output rows (n) and columns (k) of a workgroup's tile
constexpr int WG_TT = 64;                         // tokens per staging tile
constexpr int WG_OPND = WG_TT * 256;              // bytes of one operand image
constexpr int WG_LDS = 2 * WG_OPND;
constexpr int WF_TILE = 64, WF_TT = 16;           // the fp32 path's output tile and tokens per staging tile

LRP_DEVICE uint32_t wg_off(int row, int ch) { return 256u * (uint32_t)row + 16u * (uint32_t)(ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

// 8 consecutive tokens (rows r0 .. r0 + 7 of this lane's 16-lane group) of one column, as the MFMA operand
LRP_DEVICE bf16x8 wg_frag_tr(const char* img, uint32_t off0, uint32_t off1) {
    const wg_s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s16x4_t)(img + off0));
    const wg_s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s16x4_t)(img + off1));
    const wg_s16x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(bf16x8, v);
}

// where a thread stands in its wave's 64 x 64 part of the tile: the wave's n / k half, the lane's row of a 16 x 16 tile and its group of 4 columns.
// Passed BY VALUE: taken by reference the token loops compiled to another schedule and 8 - 14 more VGPRs (profiles/wgrad_tiles_refactor_isa.txt)
struct WgLane {
    int wn, wk, i16, hi;
};
LRP_DEVICE WgLane wg_lane(int tid) { return WgLane{tid >> 7, (tid >> 6) & 1, tid & 15, (tid & 63) >> 4}; }

// staging store: thread -> the 16-byte chunk sch of the token rows srow + 16 i of both images, from the registers its loads filled.
// SCALE: the token's scale is folded into G here, G' = bf16(float(G) s[i]) -- one extra rounding.
template <bool SCALE>
LRP_DEVICE void wg_stage(char* smem, int srow, int sch, const u32x4 (&gr)[4], const u32x4 (&xr)[4], const float (&s)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t o = wg_off(srow + 16 * i, sch);
        u32x4 g = gr[i];
        if constexpr (SCALE) {
            bf16x8 v = __builtin_bit_cast(bf16x8, g);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (bf16_t)((float)v[e] * s[i]);
            g = __builtin_bit_cast(u32x4, v);
        }
        *reinterpret_cast<u32x4*>(smem + o) = g;
        *reinterpret_cast<u32x4*>(smem + WG_OPND + o) = xr[i];
    }
}

LRP_DEVICE void wg_clear(f32x4 (&acc)[4][4]) {                         // acc[k tile jx][n tile jg]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// one staged 64-token tile: 2 x (8 transposed fragment reads + 16 MFMAs).  Lane 4 q + p of a 16-lane group supplies row q, columns
// 4 p .. 4 p + 3 of the group's 4 x 16 block
LRP_DEVICE void wg_mma_tile(const char* smem, const WgLane L, f32x4 (&acc)[4][4]) {
    const int q = L.i16 >> 2, p = L.i16 & 3;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int r0 = 32 * ks + 8 * L.hi + q, r1 = r0 + 4;
        bf16x8 fg[4], fx[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cg = 8 * L.wn + 2 * j + (p >> 1), cx = 8 * L.wk + 2 * j + (p >> 1);
            fg[j] = wg_frag_tr(smem, wg_off(r0, cg) + 8 * (p & 1), wg_off(r1, cg) + 8 * (p & 1));
            fx[j] = wg_frag_tr(smem + WG_OPND, wg_off(r0, cx) + 8 * (p & 1), wg_off(r1, cx) + 8 * (p & 1));
        }
#pragma unroll
        for (int jx = 0; jx < 4; ++jx)
#pragma unroll
            for (int jg = 0; jg < 4; ++jg) acc[jx][jg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fx[jx], fg[jg], acc[jx][jg], 0, 0, 0);
    }
}

// the lane's 16 accumulator fragments inside the result: cell(r, k, acc[n, k .. k + 3]) for every one with n < N and k < K, r = row(n) being
// whatever the epilogue needs once per output row (its row pointers).  (K is a multiple of 8: k < K means k + 3 < K)
template <typename Row, typename Cell>
LRP_DEVICE void wg_for_each(int n0, int k0, const WgLane L, int N, int K, const f32x4 (&acc)[4][4], Row&& row, Cell&& cell) {
#pragma unroll
    for (int jg = 0; jg < 4; ++jg) {
        const int n = n0 + 64 * L.wn + 16 * jg + L.i16;
        if (n >= N) continue;
        const auto r = row(n);
#pragma unroll
        for (int jx = 0; jx < 4; ++jx) {
            const int k = k0 + 64 * L.wk + 16 * jx + 4 * L.hi;
            if (k < K) cell(r, k, acc[jx][jg]);
        }
    }
}

// ---- fp32: thread (tx, ty) = (tid & 15, tid >> 4) owns outputs n = n0 + 4 ty + a, k = k0 + 4 tx + b.  The fp64 FMA block over a staged tile and the
// 4 x 4 output walk stay written out in the four fp32 kernels: as functions they did not compile to the kernels' previous text
// (profiles/wgrad_tiles_refactor_isa.txt), and nothing had timed the parity path against its spread a second time
LRP_DEVICE void wf_clear(double (&acc)[4][4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
}

// ---- host: the rules of every entry's predicate -- the dtype, the tiles of N within gridDim.y, and for bf16 whole 16-byte chunks of the
// G and X rows (inside or outside the tile as a whole).  1, or the LRP_E* code
inline int wg_shape_ok(int N, int K, int dtype) {
    if (dtype != LRP_F32 && dtype != LRP_BF16) return LRP_EINVAL;
    const int tile = dtype == LRP_BF16 ? WG_TILE : WF_TILE;
    if (((int64_t)N + tile - 1) / tile > 65535) return LRP_ESHAPE;
    if (dtype == LRP_BF16 && (N % 8 || K % 8)) return LRP_ESHAPE;
    return 1;
}

}  // namespace
