// attention_tiles.hpp -- what the 16x16 attention kernels share: LDS tile staging and fragments, row-side loads, out^T stores, the mask.
// Included by attention.hip and attention_cp.hip.
#pragma once
#include "common.hpp"
#include <type_traits>

namespace {

constexpr int ANT = 256;      // 4 waves

template <typename T> struct AT {
    static constexpr int SZ = sizeof(T);
    static constexpr int EPC = 16 / SZ;
    static constexpr int CT = 128 / SZ;       // column-side tile: 64 bf16 / 32 fp32 elements = 128 B
    static constexpr int NC16 = CT / 16;      // 16-wide sub-tiles per column tile (4 / 2)
};

LRP_DEVICE int swz_mask(int pitch_bytes) {
    const int cpr = pitch_bytes >> 4;
    return (cpr >= 16 ? 16 : cpr) - 1;
}

// cooperative global->register fetch of a [ROWS x PITCH bytes] tile; NCH 16-byte chunks per thread
template <int ROWS, int PITCH>
struct TileStage {
    static constexpr int CPR = PITCH / 16;
    static constexpr int NCHUNK = ROWS * CPR;
    static constexpr int NCH = (NCHUNK + ANT - 1) / ANT;
    u32x4 r[NCH];
    // gbase: address of (row 0, byte 0); row_stride in bytes; rows_valid / bytes_valid bound the read
    LRP_DEVICE void gload(const char* gbase, int64_t row_stride, int rows_valid, int bytes_valid) {
#pragma unroll
        for (int p = 0; p < NCH; ++p) {
            const int id = threadIdx.x + p * ANT;
            const int row = id / CPR, c = id % CPR;
            const bool ok = (id < NCHUNK) && (row < rows_valid) && (c * 16 < bytes_valid);
            r[p] = ok ? *reinterpret_cast<const u32x4*>(gbase + (int64_t)row * row_stride + c * 16) : u32x4{0, 0, 0, 0};
        }
    }
    LRP_DEVICE void swrite(char* lds) const {
        constexpr int SW = (CPR >= 16 ? 16 : CPR) - 1;
#pragma unroll
        for (int p = 0; p < NCH; ++p) {
            const int id = threadIdx.x + p * ANT;
            const int row = id / CPR, c = id % CPR;
            if (id < NCHUNK) *reinterpret_cast<u32x4*>(lds + row * PITCH + ((c ^ (row & SW)) << 4)) = r[p];
        }
    }
};

template <int PITCH> LRP_DEVICE const char* lds_chunk(const char* lds, int row, int chunk) {
    constexpr int CPR = PITCH / 16;
    constexpr int SW = (CPR >= 16 ? 16 : CPR) - 1;
    return lds + row * PITCH + ((chunk ^ (row & SW)) << 4);
}

// row-major tile [rows][D]: operand fragment of row (r16*16 + l&15), 64-byte K chunk c
template <typename T, int D> LRP_DEVICE typename Mma16<T>::frag rm_frag(const char* lds, int r16, int c, int lane) {
    constexpr int PITCH = D * (int)sizeof(T);
    const int row = r16 * 16 + (lane & 15);
    return *reinterpret_cast<const typename Mma16<T>::frag*>(lds_chunk<PITCH>(lds, row, c * 4 + (lane >> 4)));
}
// transposed tile [D rows][128 B]: fragment of head-dim row (dt*16 + l&15) for macro k-step kc (64 B
// of columns).  Slot order must match the register-resident operand built by pack_cols():
//   bf16: e<4 -> column 32kc + 4g + e ; e>=4 -> column 32kc + 16 + 4g + (e-4)   (two 8-byte reads)
//   fp32: e   -> column 16kc + 4g + e                                           (one 16-byte read)
template <typename T> LRP_DEVICE typename Mma16<T>::frag tr_frag(const char* lds, int dt, int kc, int lane);
template <> LRP_DEVICE bf16x8 tr_frag<bf16_t>(const char* lds, int dt, int kc, int lane) {
    const int row = dt * 16 + (lane & 15), g = lane >> 4;
    const char* p0 = lds_chunk<128>(lds, row, 4 * kc + (g >> 1)) + (g & 1) * 8;
    const char* p1 = lds_chunk<128>(lds, row, 4 * kc + 2 + (g >> 1)) + (g & 1) * 8;
    const u32x2 a = *reinterpret_cast<const u32x2*>(p0);
    const u32x2 b = *reinterpret_cast<const u32x2*>(p1);
    u32x4 v = {a[0], a[1], b[0], b[1]};
    return __builtin_bit_cast(bf16x8, v);
}
template <> LRP_DEVICE f32x4 tr_frag<float>(const char* lds, int dt, int kc, int lane) {
    const int row = dt * 16 + (lane & 15), g = lane >> 4;
    return *reinterpret_cast<const f32x4*>(lds_chunk<128>(lds, row, 4 * kc + g));
}
// register-resident second operand from the D registers of the column sub-tiles of macro step kc
template <typename T> struct PackCols;
template <> struct PackCols<bf16_t> {   // sub-tiles 2kc, 2kc+1
    static LRP_DEVICE bf16x8 pack(const f32x4* x, int kc) {
        bf16x8 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) { r[e] = (bf16_t)x[2 * kc][e]; r[4 + e] = (bf16_t)x[2 * kc + 1][e]; }
        return r;
    }
};
template <> struct PackCols<float> {    // sub-tile kc
    static LRP_DEVICE f32x4 pack(const f32x4* x, int kc) { return x[kc]; }
};

// row-side operand fragments straight from global memory (token-major [rows, H, D], one head)
template <typename T, int D>
LRP_DEVICE void load_row_frags(typename Mma16<T>::frag* f, const T* base, int64_t ld, int row, int rows_valid, int lane) {
    constexpr int NDC = D * (int)sizeof(T) / 64;
    constexpr int EPC = 16 / (int)sizeof(T);
    const bool ok = row < rows_valid;
#pragma unroll
    for (int c = 0; c < NDC; ++c) {
        if (ok) f[c] = *reinterpret_cast<const typename Mma16<T>::frag*>(base + (int64_t)row * ld + (c * 4 + (lane >> 4)) * EPC);
        else {
            u32x4 z = {0, 0, 0, 0};
            f[c] = __builtin_bit_cast(typename Mma16<T>::frag, z);
        }
    }
}

// store out^T accumulators: lane holds out[row = l&15][col = dt*16 + (l>>4)*4 + r]
template <typename T, int D>
LRP_DEVICE void store_rows(T* base, int64_t ld, int row, int rows_valid, const f32x4* acc, float mul, int lane) {
    if (row >= rows_valid) return;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
        T* dst = base + (int64_t)row * ld + dt * 16 + (lane >> 4) * 4;
        if constexpr (sizeof(T) == 4) {
            f32x4 v = acc[dt] * mul;
            *reinterpret_cast<f32x4*>(dst) = v;
        } else {
            bf16x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (bf16_t)(acc[dt][r] * mul);
            *reinterpret_cast<bf16x4*>(dst) = v;
        }
    }
}

// (causal, window) describe the STRUCTURE of the mask (they also bound which tiles are visited); [lo, hi) is the optional
// per-query-row key interval (padding, packed sequences, bidirectional blocks) that refines it element-wise
LRP_DEVICE bool visible(int q, int key, int S, int causal, int window, int lo, int hi) {
    return key < S && (!causal || key <= q) && (window <= 0 || key > q - window) && key >= lo && key < hi;
}

}  // namespace
