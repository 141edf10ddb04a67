// decode.hip -- the two kernels of a KV-cached decode step (include/lrp_hip_decode.h): lrp_decode_rope_append, lrp_attn_decode.
//
// Both read the step's column from device memory (pos), so a captured step is the same launch sequence at every column, and both check that
// column on the device before an address is formed from it: no value of *pos makes either kernel touch memory outside the caches.
//
// lrp_attn_decode is HBM-bound (a step reads every live K / V row once and does 4 flops per element and query head): K / V go straight to
// registers in 16-byte loads, 16 lanes per key (a row of d = 128 bf16 is one load instruction of a 16-lane group), and the rep query heads of a
// kv head are all served from those registers.  At most 8 live query rows: no MFMA (a 16-row tile would be half empty at best and wants its
// operand through LDS), no LDS for operands.  The score of a key is reduced over its 16 lanes by four DPP row operations (VALU, not the LDS
// pipe); what crosses the LDS is the slab's maximum and, once per slab, the accumulators of the 16 key groups.
//
// Order of the sums (the result depends on a key's index only, never on B, cap or *pos): a lane adds its elements in column order; the 16
// lanes of a key by the xor-1, xor-2, half-mirror, mirror butterfly; a key group its keys j0 + g, j0 + g + 16, ... in that order; the four
// groups of a wave by the xor-16, xor-32 butterfly; the four waves in wave order; the slabs in ascending order (second launch).
#include "common.hpp"

namespace {

constexpr int DEC_SLAB = 64;                         // keys per slab (lrp_attn_decode_slab)
constexpr int DEC_NT = 256;                          // threads per workgroup
constexpr int DEC_LPK = 16;                          // lanes per key
constexpr int DEC_NP = DEC_SLAB / (DEC_NT / DEC_LPK);  // keys per 16-lane group and slab

inline bool on16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool on4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// element e of a 16-byte vector of T held as four words
template <typename T> LRP_DEVICE float vec_elem(const u32x4& v, int e);
template <> LRP_DEVICE float vec_elem<float>(const u32x4& v, int e) {
    const uint32_t w = v[e];          // (a copy first: __builtin_bit_cast on the element lvalue itself reads element 0 whatever e is)
    return __builtin_bit_cast(float, w);
}
template <> LRP_DEVICE float vec_elem<bf16_t>(const u32x4& v, int e) { return (e & 1) ? bf16_hi(v[e >> 1]) : bf16_lo(v[e >> 1]); }

template <int CTRL> LRP_DEVICE float dpp_move(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}
// sum over the 16 lanes of a DPP row, the same bits in every lane: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror
LRP_DEVICE float row16_sum(float x) {
    x += dpp_move<0xB1>(x);
    x += dpp_move<0x4E>(x);
    x += dpp_move<0x141>(x);
    x += dpp_move<0x140>(x);
    return x;
}

// ---- RoPE of the new token's q | k, append of k and v at column *pos -------------------------------------------------------------------
// a thread per 16-byte vector of a (prompt, head) row; heads [0, nq): q, [nq, nq + nk): k, [nq + nk, nq + 2 nk): v.  VECP: d / 2 is a whole
// number of vectors, the rotate-half partner is then ONE aligned vector
template <typename T, bool VECP>
__global__ __launch_bounds__(256) void decode_rope_append_kernel(const T* __restrict__ qk, int64_t ldqk, const T* __restrict__ v, int64_t ldv,
                                                                 const float* __restrict__ cs, const float* __restrict__ sn, int table_rows,
                                                                 const int* __restrict__ pos, T* __restrict__ q_rot, int64_t ldq,
                                                                 T* __restrict__ kc, T* __restrict__ vc, int64_t ldc, int B, int cap, int nq,
                                                                 int nk, int d) {
    constexpr int E = 16 / sizeof(T);
    const int p = *pos;
    if (p < 0 || p >= cap || p >= table_rows) return;
    const int vph = d / E, nh = nq + 2 * nk, hd = d / 2;
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * nh * vph) return;
    const int c0 = (int)(i % vph) * E;
    const int h = (int)((i / vph) % nh);
    const int64_t b = i / ((int64_t)vph * nh);
    const int64_t crow = (b * cap + p) * ldc;
    if (h >= nq + nk) {
        const int hv = h - nq - nk;
        st16(vc + crow + (int64_t)hv * d + c0, ld16(v + b * ldv + (int64_t)hv * d + c0));
        return;
    }
    const T* src = qk + b * ldqk + (int64_t)h * d;
    const Vec16<T> x = ld16(src + c0);
    float part[E], ct[E], st[E];
    if constexpr (VECP) {
        const Vec16<T> y = ld16(src + (c0 < hd ? c0 + hd : c0 - hd));
#pragma unroll
        for (int e = 0; e < E; ++e) part[e] = y.get(e);
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) part[e] = to_f32(src[c0 + e < hd ? c0 + e + hd : c0 + e - hd]);
    }
#pragma unroll
    for (int e4 = 0; e4 < E / 4; ++e4) {
        const f32x4 c = *reinterpret_cast<const f32x4*>(cs + (int64_t)p * d + c0 + 4 * e4);
        const f32x4 s = *reinterpret_cast<const f32x4*>(sn + (int64_t)p * d + c0 + 4 * e4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { ct[4 * e4 + e] = c[e]; st[4 * e4 + e] = s[e]; }
    }
    Vec16<T> out;
#pragma unroll
    for (int e = 0; e < E; ++e) {          // lrp_rope_fwd's two lines: the first half of a head takes the minus sign
        const float xc = x.get(e) * ct[e], ps = part[e] * st[e];
        out.set(e, c0 + e < hd ? xc - ps : xc + ps);
    }
    T* dst = h < nq ? q_rot + b * ldq + (int64_t)h * d : kc + crow + (int64_t)(h - nq) * d;
    st16(dst + c0, out);
}

// ---- single-query attention, launch 1: one workgroup per (slab, kv head x head tile, prompt) --------------------------------------------
// NC: 16-byte vectors of a key row per lane (vector lane16 + 16 c); RT: query heads of the kv head served from one load of the slab
template <typename T, int NC, int RT>
__global__ __launch_bounds__(DEC_NT) void attn_decode_kernel(const T* __restrict__ q, int64_t ldq, const T* __restrict__ kc,
                                                             const T* __restrict__ vc, int64_t ldc, const int* __restrict__ lo,
                                                             const int* __restrict__ pos, float* __restrict__ ws, int cap, int Hq, int Hkv,
                                                             int d, float scale, int ntile) {
    constexpr int E = 16 / sizeof(T);
    constexpr int DP = NC * DEC_LPK * E;             // columns the lanes of a key cover (>= d)
    __shared__ __attribute__((aligned(16))) float red[4 * RT * DP];
    __shared__ float redm[4 * RT], redl[4 * RT];
    const int p = *pos;
    if (p < 0 || p >= cap) return;
    const int b = blockIdx.z, kvh = blockIdx.y / ntile, tile = blockIdx.y % ntile, s = blockIdx.x;
    const int l0 = min(max(lo[b], 0), p);
    const int j0 = s * DEC_SLAB;
    if (j0 > p || j0 + DEC_SLAB <= l0) return;       // (uniform over the workgroup: ahead of every load and barrier)
    const int rep = Hq / Hkv, nch = d / E;
    const int lane16 = threadIdx.x & 15, g = threadIdx.x >> 4, wave = threadIdx.x >> 6;
    const int h0 = kvh * rep + tile * RT, nlive = min(RT, rep - tile * RT);

    u32x4 kr[DEC_NP][NC], vr[DEC_NP][NC];
    bool ok[DEC_NP];
#pragma unroll
    for (int pi = 0; pi < DEC_NP; ++pi) {
        const int j = j0 + pi * (DEC_NT / DEC_LPK) + g;
        ok[pi] = j >= l0 && j <= p;
        const int64_t off = ((int64_t)b * cap + j) * ldc + (int64_t)kvh * d;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int ch = lane16 + DEC_LPK * c;
            const bool ld = ok[pi] && ch < nch;
            kr[pi][c] = ld ? *reinterpret_cast<const u32x4*>(kc + off + ch * E) : u32x4{0u, 0u, 0u, 0u};
            vr[pi][c] = ld ? *reinterpret_cast<const u32x4*>(vc + off + ch * E) : u32x4{0u, 0u, 0u, 0u};
        }
    }
    float qf[RT][NC][E];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int ch = lane16 + DEC_LPK * c;
            const bool ld = r < nlive && ch < nch;
            const u32x4 x = ld ? *reinterpret_cast<const u32x4*>(q + (int64_t)b * ldq + (int64_t)(h0 + r) * d + ch * E) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
            for (int e = 0; e < E; ++e) qf[r][c][e] = vec_elem<T>(x, e);
        }

    // scores of this group's keys, every lane of the group holding the same bits; the slab's maximum per head
    float sc[DEC_NP][RT], m[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) m[r] = -INFINITY;
#pragma unroll
    for (int pi = 0; pi < DEC_NP; ++pi)
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            float a = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int e = 0; e < E; ++e) a = fmaf(qf[r][c][e], vec_elem<T>(kr[pi][c], e), a);
            a = row16_sum(a);
            sc[pi][r] = ok[pi] ? a * scale : -INFINITY;
            m[r] = fmaxf(m[r], sc[pi][r]);
        }
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        m[r] = fmaxf(m[r], __shfl_xor(m[r], 16, 64));
        m[r] = fmaxf(m[r], __shfl_xor(m[r], 32, 64));
        if ((threadIdx.x & 63) == 0) redm[wave * RT + r] = m[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RT; ++r) m[r] = fmaxf(fmaxf(redm[r], redm[RT + r]), fmaxf(redm[2 * RT + r], redm[3 * RT + r]));

    // p = exp(s - m) (a masked key: exp(-inf) = 0 on a V vector that was never loaded), l and P V of this group's keys
    float acc[RT][NC][E], ls[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        ls[r] = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int e = 0; e < E; ++e) acc[r][c][e] = 0.f;
    }
#pragma unroll
    for (int pi = 0; pi < DEC_NP; ++pi)
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const float pr = ok[pi] ? expf(sc[pi][r] - m[r]) : 0.f;
            ls[r] += pr;
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int e = 0; e < E; ++e) acc[r][c][e] = fmaf(pr, vec_elem<T>(vr[pi][c], e), acc[r][c][e]);
        }
    // the four key groups of a wave, then the four waves through LDS
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        ls[r] += __shfl_xor(ls[r], 16, 64);
        ls[r] += __shfl_xor(ls[r], 32, 64);
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                float a = acc[r][c][e];
                a += __shfl_xor(a, 16, 64);
                a += __shfl_xor(a, 32, 64);
                acc[r][c][e] = a;
            }
    }
    if ((threadIdx.x & 63) < DEC_LPK) {
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            if (lane16 == 0) redl[wave * RT + r] = ls[r];
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int e4 = 0; e4 < E / 4; ++e4) {
                    const f32x4 a = {acc[r][c][4 * e4], acc[r][c][4 * e4 + 1], acc[r][c][4 * e4 + 2], acc[r][c][4 * e4 + 3]};
                    *reinterpret_cast<f32x4*>(&red[(wave * RT + r) * DP + (lane16 + DEC_LPK * c) * E + 4 * e4]) = a;
                }
        }
    }
    __syncthreads();
    // the slab's partial of head h: acc at ws[((b Hq + h) NS + s) d], (m, l) behind all the accs
    const int NS = (cap + DEC_SLAB - 1) / DEC_SLAB, d4 = d / 4;
    float* ws_ml = ws + (int64_t)gridDim.z * Hq * NS * d;
    for (int i = threadIdx.x; i < nlive * d4; i += DEC_NT) {
        const int r = i / d4, c4 = i - r * d4;
        f32x4 a = *reinterpret_cast<const f32x4*>(&red[r * DP + 4 * c4]);
#pragma unroll
        for (int w = 1; w < 4; ++w) a += *reinterpret_cast<const f32x4*>(&red[(w * RT + r) * DP + 4 * c4]);
        *reinterpret_cast<f32x4*>(ws + (((int64_t)b * Hq + h0 + r) * NS + s) * d + 4 * c4) = a;
    }
    if ((int)threadIdx.x < nlive) {
        const int r = threadIdx.x;
        float* ml = ws_ml + (((int64_t)b * Hq + h0 + r) * NS + s) * 2;
        ml[0] = fmaxf(fmaxf(redm[r], redm[RT + r]), fmaxf(redm[2 * RT + r], redm[3 * RT + r]));      // (m[r], without a register index)
        ml[1] =((redl[r] + redl[RT + r]) + redl[2 * RT + r]) + redl[3 * RT + r];
    }
}

// ---- launch 2: the live slabs of a (prompt, head) in ascending order; thread t owns columns 4 t .. 4 t + 3 ------------------------------
template <typename T>
__global__ __launch_bounds__(64) void attn_decode_combine_kernel(const float* __restrict__ ws, const int* __restrict__ lo,
                                                                 const int* __restrict__ pos, T* __restrict__ o, int64_t ldo, int cap,
                                                                 int Hq, int d) {
    const int p = *pos;
    if (p < 0 || p >= cap) return;
    // one wave: the slabs' (m, l) are fetched 64 at a time, a slab per lane, and turned into the weights exp(m - M), exp(m - M) l in LDS; the
    // accumulator rows are then fetched eight at a time (independent loads, one round trip) and added in ascending slab order
    __shared__ float wsh[64], lsh[64];
    const int h = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const bool live = 4 * t < d;
    const int l0 = min(max(lo[b], 0), p);
    const int s0 = l0 / DEC_SLAB, s1 = p / DEC_SLAB, NS = (cap + DEC_SLAB - 1) / DEC_SLAB;
    const int64_t base = ((int64_t)b * Hq + h) * NS;
    const float* ml = ws + (int64_t)gridDim.y * Hq * NS * d + base * 2;
    float M = -INFINITY;
    for (int s = s0 + t; s <= s1; s += 64) M = fmaxf(M, ml[2 * s]);
    M = wave_max(M);
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    float L = 0.f;
    for (int c0 = s0; c0 <= s1; c0 += 64) {
        const int cnt = min(64, s1 - c0 + 1);
        __syncthreads();
        if (t < cnt) {
            const f32x2 v = *reinterpret_cast<const f32x2*>(ml + 2 * (c0 + t));
            const float w = expf(v[0] - M);
            wsh[t] = w;
            lsh[t] = v[1];
        }
        __syncthreads();
        for (int i0 = 0; i0 < cnt; i0 += 8) {
            f32x4 x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                x[u] = (live && i0 + u < cnt) ? *reinterpret_cast<const f32x4*>(ws + (base + c0 + i0 + u) * d + 4 * t) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (i0 + u < cnt) {
                    const float w = wsh[i0 + u];
                    L = fmaf(w, lsh[i0 + u], L);
#pragma unroll
                    for (int e = 0; e < 4; ++e) a[e] = fmaf(w, x[u][e], a[e]);
                }
        }
    }
    if (!live) return;
    T* dst = o + (int64_t)b * ldo + (int64_t)h * d + 4 * t;
    if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<f32x4*>(dst) = f32x4{a[0] / L, a[1] / L, a[2] / L, a[3] / L};
    } else {
        const bf16x4 r = {(bf16_t)(a[0] / L), (bf16_t)(a[1] / L), (bf16_t)(a[2] / L), (bf16_t)(a[3] / L)};
        *reinterpret_cast<bf16x4*>(dst) = r;
    }
}

struct DecodeArgs {
    const void *q, *kc, *vc;
    const int *lo, *pos;
    float* ws;
    int64_t ldq, ldc;
    int B, cap, Hq, Hkv, d, ntile;
    float scale;
};

template <typename T, int NC, int RT> void attn_decode_launch(const DecodeArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)((a.cap + DEC_SLAB - 1) / DEC_SLAB), (unsigned)(a.Hkv * a.ntile), (unsigned)a.B);
    hipLaunchKernelGGL((attn_decode_kernel<T, NC, RT>), grid, dim3(DEC_NT), 0, st, (const T*)a.q, a.ldq, (const T*)a.kc, (const T*)a.vc, a.ldc,
                       a.lo, a.pos, a.ws, a.cap, a.Hq, a.Hkv, a.d, a.scale, a.ntile);
}
template <typename T, int NC> void attn_decode_rt(const DecodeArgs& a, int rt, hipStream_t st) {
    if (rt == 1) attn_decode_launch<T, NC, 1>(a, st);
    else if (rt == 2) attn_decode_launch<T, NC, 2>(a, st);
    else if (rt == 4) attn_decode_launch<T, NC, 4>(a, st);
    else attn_decode_launch<T, NC, 8>(a, st);
}

}  // namespace

extern "C" int lrp_decode_rope_append(const void* qk, int64_t ldqk, const void* v, int64_t ldv, const float* cos_t, const float* sin_t,
                                      int table_rows, const int* pos, void* q_rot, int64_t ldq, void* kc, void* vc, int64_t ldc, int B, int cap,
                                      int nq, int nk, int d, int dtype, void* stream) {
    if (!qk || !v || !cos_t || !sin_t || !pos || !q_rot || !kc || !vc || B < 0 || nq < 1 || nk < 1 || cap < 1 || table_rows < 1 ||
        (dtype != LRP_F32 && dtype != LRP_BF16))
        return LRP_EINVAL;
    const int64_t es = dtype == LRP_F32 ? 4 : 2, epc = 16 / es;
    if (d < 2 || (d & 1) || d > 256 || (d * es) % 16) return LRP_ESHAPE;
    if (ldqk < (int64_t)(nq + nk) * d || ldv < (int64_t)nk * d || ldq < (int64_t)nq * d || ldc < (int64_t)nk * d) return LRP_ESHAPE;
    const int64_t work = (int64_t)B * (nq + 2 * nk) * (d / epc);
    if ((work + 255) / 256 > 0x7fffffff) return LRP_ESHAPE;
    if (!on16(qk) || !on16(v) || !on16(q_rot) || !on16(kc) || !on16(vc) || !on16(cos_t) || !on16(sin_t) || !on4(pos)) return LRP_EALIGN;
    if (ldqk % epc || ldv % epc || ldq % epc || ldc % epc) return LRP_EALIGN;
    if (B == 0) return LRP_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((work + 255) / 256));
    const bool vecp = (d / 2) % epc == 0;
#define LRP_APPEND(T, VP)                                                                                                                   \
    hipLaunchKernelGGL((decode_rope_append_kernel<T, VP>), grid, dim3(256), 0, st, (const T*)qk, ldqk, (const T*)v, ldv, cos_t, sin_t,     \
                       table_rows, pos, (T*)q_rot, ldq, (T*)kc, (T*)vc, ldc, B, cap, nq, nk, d)
    if (dtype == LRP_F32) { if (vecp) LRP_APPEND(float, true); else LRP_APPEND(float, false); }
    else { if (vecp) LRP_APPEND(bf16_t, true); else LRP_APPEND(bf16_t, false); }
#undef LRP_APPEND
    return lrp_check_launch();
}

extern "C" int lrp_attn_decode_slab(void) { return DEC_SLAB; }

extern "C" int64_t lrp_attn_decode_ws(int B, int Hq, int d, int cap) {
    if (B < 1 || Hq < 1 || d < 8 || d > 256 || (d % 8) || cap < 1) return -1;
    const int64_t ns = (cap + DEC_SLAB - 1) / DEC_SLAB;
    return ((int64_t)B * Hq * ns * (d + 2) * 4 + 15) / 16 * 16;
}

extern "C" int lrp_attn_decode(const void* q, int64_t ldq, const void* kc, const void* vc, int64_t ldc, const int* lo, const int* pos, void* o,
                               int64_t ldo, void* ws, int64_t ws_bytes, int B, int cap, int Hq, int Hkv, int d, float scale, int dtype,
                               void* stream) {
    if (!q || !kc || !vc || !lo || !pos || !o || !ws || B < 0 || Hq < 1 || Hkv < 1 || cap < 1 || (dtype != LRP_F32 && dtype != LRP_BF16))
        return LRP_EINVAL;
    if (Hq % Hkv || d < 8 || d > 256 || (d % 8)) return LRP_ESHAPE;
    if (ldq < (int64_t)Hq * d || ldo < (int64_t)Hq * d || ldc < (int64_t)Hkv * d) return LRP_ESHAPE;
    const int rep = Hq / Hkv, rt = rep >= 5 ? 8 : rep >= 3 ? 4 : rep, ntile = (rep + rt - 1) / rt;
    if (B > 65535 || (int64_t)Hkv * ntile > 65535) return LRP_ESHAPE;          // (grid dimensions y, z)
    if (B > 0 && ws_bytes < lrp_attn_decode_ws(B, Hq, d, cap)) return LRP_ESHAPE;
    const int64_t epc = dtype == LRP_F32 ? 4 : 8;
    if (!on16(q) || !on16(kc) || !on16(vc) || !on16(o) || !on16(ws) || !on4(lo) || !on4(pos)) return LRP_EALIGN;
    if (ldq % epc || ldo % epc || ldc % epc) return LRP_EALIGN;
    if (B == 0) return LRP_OK;
    hipStream_t st = (hipStream_t)stream;
    const DecodeArgs a{q, kc, vc, lo, pos, (float*)ws, ldq, ldc, B, cap, Hq, Hkv, d, ntile, scale};
    const int nch = d / (int)epc;                     // 16-byte vectors of a key row; a lane takes every 16th
    if (dtype == LRP_F32) {
        if (nch <= 16) attn_decode_rt<float, 1>(a, rt, st);
        else if (nch <= 32) attn_decode_rt<float, 2>(a, rt, st);
        else attn_decode_rt<float, 4>(a, rt, st);
        hipLaunchKernelGGL((attn_decode_combine_kernel<float>), dim3((unsigned)Hq, (unsigned)B), dim3(64), 0, st, (const float*)ws, lo, pos,
                           (float*)o, ldo, cap, Hq, d);
    } else {
        if (nch <= 16) attn_decode_rt<bf16_t, 1>(a, rt, st);
        else attn_decode_rt<bf16_t, 2>(a, rt, st);
        hipLaunchKernelGGL((attn_decode_combine_kernel<bf16_t>), dim3((unsigned)Hq, (unsigned)B), dim3(64), 0, st, (const float*)ws, lo, pos,
                           (bf16_t*)o, ldo, cap, Hq, d);
    }
    return lrp_check_launch();
}
