// decode_site.hip -- the site kernel of a Gemma-3 decode step (include/lrp_hip_decode_site.h): lrp_decode_qknorm_rope_append.
//
// Between the QKV projection and the cache a Gemma-3 / Qwen3 step has a per-head RMSNorm on q and on k, then RoPE and the append: three
// launches (2 x lrp_head_rmsnorm_fwd, lrp_decode_rope_append) and two round trips of [B, (nq + nk) d] through memory.  This is the one-pass
// form, as lrp_qk_norm_rope_fwd (sandwich.hip) is for the prefill: a lane group of d / W lanes per (prompt, head), the head in registers.
//
// Bit identity with the three launches: the sum of squares is head_rmsnorm_fwd_kernel's (a lane adds its W squares in column order, the lanes
// by the xor butterfly lpg/2 .. 1), rstd = rsqrtf(ss / d + eps), the normed value is rounded to the storage type where that kernel stored it,
// and the rotation is decode_rope_append_kernel's two products and one sum in fp32 (no contraction: -ffp-contract=off), rounded once.
// The step's column comes from device memory and is checked before any address is formed from it, as in decode.hip.
#include "common.hpp"

namespace {

inline bool on16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool on4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

constexpr int SITE_NT = 64;                          // one wave per workgroup: 64 / (d / W) heads

// heads [0, nq): q, [nq, nq + nk): k, [nq + nk, nq + 2 nk): v.  Lane lg of a group holds columns lg W .. lg W + W - 1; the rotate-half partner
// column c +- d/2 sits lpg / 2 lanes away (lpg >= 2), or W / 2 elements away in the same lane (lpg == 1: d is one 16-byte vector)
template <typename T, int W>
__global__ __launch_bounds__(SITE_NT) void decode_qknorm_rope_append_kernel(const T* __restrict__ qk, int64_t ldqk, const T* __restrict__ v,
                                                                            int64_t ldv, const T* __restrict__ wq, const T* __restrict__ wk,
                                                                            const float* __restrict__ cs, const float* __restrict__ sn,
                                                                            int table_rows, const int* __restrict__ pos, T* __restrict__ q_rot,
                                                                            int64_t ldq, T* __restrict__ kc, T* __restrict__ vc, int64_t ldc,
                                                                            int B, int cap, int nq, int nk, int d, float eps, float w_off) {
    const int p = *pos;
    if (p < 0 || p >= cap || p >= table_rows) return;
    const int lpg = d / W, gpb = SITE_NT / lpg, lg = threadIdx.x % lpg, nh = nq + 2 * nk;
    const int64_t gidx = (int64_t)blockIdx.x * gpb + threadIdx.x / lpg;
    if (gidx >= (int64_t)B * nh) return;             // (a whole lane group retires: the shuffles below stay inside a group)
    const int h = (int)(gidx % nh), c0 = lg * W;
    const int64_t b = gidx / nh;
    const int64_t crow = (b * cap + p) * ldc;
    if (h >= nq + nk) {
        const int hv = h - nq - nk;
        st16(vc + crow + (int64_t)hv * d + c0, ld16(v + b * ldv + (int64_t)hv * d + c0));
        return;
    }
    const bool isq = h < nq;
    const Vec16<T> x = ld16(qk + b * ldqk + (int64_t)h * d + c0);
    const Vec16<T> ww = ld16((isq ? wq : wk) + c0);
    float a[W], ct[W], st[W];
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        a[k] = x.get(k);
        ss += a[k] * a[k];
    }
    for (int off = lpg >> 1; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    const float rs = rsqrtf(ss / (float)d + eps);
#pragma unroll
    for (int k4 = 0; k4 < W / 4; ++k4) {
        const f32x4 c = *reinterpret_cast<const f32x4*>(cs + (int64_t)p * d + c0 + 4 * k4);
        const f32x4 s = *reinterpret_cast<const f32x4*>(sn + (int64_t)p * d + c0 + 4 * k4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { ct[4 * k4 + e] = c[e]; st[4 * k4 + e] = s[e]; }
    }
    float n[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {                    // head_rmsnorm_fwd_kernel's two conventions, then its store's rounding
        const float y = (w_off == 0.f) ? ww.get(k) * to_f32(from_f32<T>(a[k] * rs)) : (a[k] * rs) * (w_off + ww.get(k));
        n[k] = to_f32(from_f32<T>(y));
    }
    Vec16<T> out;
    if (lpg > 1) {
        const bool first = lg < (lpg >> 1);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const float part = __shfl_xor(n[k], lpg >> 1, 64);
            const float xc = n[k] * ct[k], ps = part * st[k];
            out.set(k, first ? xc - ps : xc + ps);
        }
    } else {
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const float xc = n[k] * ct[k], ps = n[(k + W / 2) % W] * st[k];
            out.set(k, k < W / 2 ? xc - ps : xc + ps);
        }
    }
    T* dst = isq ? q_rot + b * ldq + (int64_t)h * d : kc + crow + (int64_t)(h - nq) * d;
    st16(dst + c0, out);
}

}  // namespace

extern "C" int lrp_decode_qknorm_rope_append(const void* qk, int64_t ldqk, const void* v, int64_t ldv, const void* wq, const void* wk, float eps,
                                             float w_offset, const float* cos_t, const float* sin_t, int table_rows, const int* pos,
                                             void* q_rot, int64_t ldq, void* kc, void* vc, int64_t ldc, int B, int cap, int nq, int nk, int d,
                                             int dtype, void* stream) {
    if (!qk || !v || !wq || !wk || !cos_t || !sin_t || !pos || !q_rot || !kc || !vc || B < 0 || nq < 1 || nk < 1 || cap < 1 || table_rows < 1 ||
        (dtype != LRP_F32 && dtype != LRP_BF16))
        return LRP_EINVAL;
    const int64_t es = dtype == LRP_F32 ? 4 : 2, epc = 16 / es;
    // lrp_decode_rope_append's head dims (even, <= 256, whole 16-byte vectors) that lrp_head_rmsnorm_fwd takes too (d / epc a power of two)
    const int lpg = d > 0 ? d / (int)epc : 0;
    if (d < 2 || (d & 1) || d > 256 || (d * es) % 16 || lpg < 1 || lpg > 64 || (lpg & (lpg - 1))) return LRP_ESHAPE;
    if (ldqk < (int64_t)(nq + nk) * d || ldv < (int64_t)nk * d || ldq < (int64_t)nq * d || ldc < (int64_t)nk * d) return LRP_ESHAPE;
    const int gpb = SITE_NT / lpg;
    const int64_t nb = ((int64_t)B * (nq + 2 * nk) + gpb - 1) / gpb;
    if (nb > 0x7fffffff) return LRP_ESHAPE;
    if (!on16(qk) || !on16(v) || !on16(wq) || !on16(wk) || !on16(q_rot) || !on16(kc) || !on16(vc) || !on16(cos_t) || !on16(sin_t) || !on4(pos))
        return LRP_EALIGN;
    if (ldqk % epc || ldv % epc || ldq % epc || ldc % epc) return LRP_EALIGN;
    if (B == 0) return LRP_OK;
    hipStream_t st = (hipStream_t)stream;
#define LRP_SITE(T)                                                                                                                           \
    hipLaunchKernelGGL((decode_qknorm_rope_append_kernel<T, 16 / sizeof(T)>), dim3((unsigned)nb), dim3(SITE_NT), 0, st, (const T*)qk, ldqk,   \
                       (const T*)v, ldv, (const T*)wq, (const T*)wk, cos_t, sin_t, table_rows, pos, (T*)q_rot, ldq, (T*)kc, (T*)vc, ldc, B,  \
                       cap, nq, nk, d, eps, w_offset)
    if (dtype == LRP_F32) LRP_SITE(float);
    else LRP_SITE(bf16_t);
#undef LRP_SITE
    return lrp_check_launch();
}
