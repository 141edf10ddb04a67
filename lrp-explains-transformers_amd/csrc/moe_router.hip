// moe_router.hip -- the top-k router of a sparse MoE layer (HF Qwen3MoeTopKRouter) on the device, forward and exact backward, and the
// per-expert relevance read-out (C ABI: include/lrp_hip_moe_router.h).  All three are small row kernels, HBM / latency bound:
//   * forward / backward: ONE wave64 per token row, lane l holds the experts l, l + 64, ... (<= 16 per lane: E <= 1024) in registers;
//     sums and the arg-max are xor butterflies, so a row's result is a fixed function of that row alone (bitwise repeatable, batch invariant);
//   * expert relevance: a workgroup owns 64 experts of ONE prompt, stages the prompt's (index, w G_w) pairs through LDS in chunks and each
//     of its sixteen waves walks a fixed sixteenth of every chunk in order; the sixteen partial sums are added in wave order.
// Plain vector loads and stores only: no atomics, no workspace, every output element is written.
#include "common.hpp"

#include <math.h>

#include <algorithm>

namespace {

constexpr int RT_EMAX = 1024;      // the routing plan's limit (csrc/moe.hip)
constexpr int RT_KMAX = 16;
constexpr int RT_PER_LANE = RT_EMAX / 64;
constexpr int RT_ROWS = 4;         // token rows (waves) per workgroup
constexpr int ER_CHUNK = 2048;     // (token, slot) pairs staged per step of the expert read-out
constexpr int ER_STRIPS = 16;      // waves per workgroup of the expert read-out: each walks a fixed 1/16 of every chunk

LRP_DEVICE float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
LRP_DEVICE float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// (value, index) key: the larger value wins, equal values go to the LOWER index (torch.topk on the device, and the all-tie rows of a
// zero-initialised router)
LRP_DEVICE bool key_before(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

// NJ: experts per lane, ceil(E / 64) rounded up to a power of two (E = 128: 2 -- the k arg-max rounds scan NJ registers each)
template <typename T, int NJ>
__global__ __launch_bounds__(64 * RT_ROWS) void moe_router_fwd_kernel(const T* __restrict__ logits, long long* __restrict__ idx,
                                                                      T* __restrict__ w, float* __restrict__ lse, int Tn, int E, int k,
                                                                      int64_t ldl, int norm_topk) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * RT_ROWS + (threadIdx.x >> 6);
    if (row >= Tn) return;          // (whole waves: no barrier below)
    const T* x = logits + (int64_t)row * ldl;
    float p[NJ];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int e = lane + 64 * j;
        p[j] = e < E ? to_f32(x[e]) : -INFINITY;
        mx = fmaxf(mx, p[j]);
    }
    mx = wave_max(mx);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        p[j] = lane + 64 * j < E ? expf(p[j] - mx) : 0.f;
        s += p[j];
    }
    s = wave_sum(s);
#pragma unroll
    for (int j = 0; j < NJ; ++j) p[j] = lane + 64 * j < E ? p[j] / s : -1.f;      // probabilities are >= 0: -1 never wins
    if (lane == 0) lse[row] = mx + logf(s);
    // k rounds of a wave arg-max; slot r's winner is parked in lane r
    float my_v = 0.f, V = 0.f;
    int my_i = 0;
    for (int r = 0; r < k; ++r) {
        float bv = p[0];
        int bi = lane;
#pragma unroll
        for (int j = 1; j < NJ; ++j)
            if (p[j] > bv) { bv = p[j]; bi = lane + 64 * j; }          // (ascending j: a tie keeps the lower index)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (key_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == r) { my_v = bv; my_i = bi; }
        V += bv;                                                       // fp32 sum in slot order
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (bi == lane + 64 * j) p[j] = -1.f;
    }
    if (lane < k) {
        idx[(int64_t)row * k + lane] = my_i;
        w[(int64_t)row * k + lane] = from_f32<T>(norm_topk ? my_v / V : my_v);      // the ONE rounding to the activation dtype
    }
}

template <typename T>
__global__ __launch_bounds__(64 * RT_ROWS) void moe_router_bwd_kernel(const T* __restrict__ logits, const float* __restrict__ lse,
                                                                      const long long* __restrict__ idx, const T* __restrict__ gw,
                                                                      T* __restrict__ gl, int Tn, int E, int k, int64_t ldl, int64_t ldg,
                                                                      int norm_topk) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * RT_ROWS + (threadIdx.x >> 6);
    if (row >= Tn) return;
    const T* x = logits + (int64_t)row * ldl;
    const float l = lse[row];
    // lane s < k: slot s (a slot whose index is outside [0, E) carries nothing)
    int my_i = -1;
    float ps = 0.f, g = 0.f;
    if (lane < k) {
        const long long ix = idx[(int64_t)row * k + lane];
        if (ix >= 0 && ix < E) {
            my_i = (int)ix;
            ps = expf(to_f32(x[my_i]) - l);
            g = to_f32(gw[(int64_t)row * k + lane]);
        }
    }
    float gv = g, dot = 0.f;
    if (norm_topk) {
        // w_s = p_s / V in fp32, as autograd holds it (the rounding to the activation dtype comes after the division and passes the
        // gradient through); sum_s G_v[s] p_s = 0 analytically, so only the selected experts receive a gradient
        const float V = wave_sum(ps);
        const float c = wave_sum(g * (ps / V));
        gv = my_i >= 0 ? (g - c) / V : 0.f;
    } else {
        dot = wave_sum(g * ps);
    }
    T* y = gl + (int64_t)row * ldg;
#pragma unroll
    for (int j = 0; j < RT_PER_LANE; ++j) {
        const int e = lane + 64 * j;
        if (j * 64 >= E) break;          // (wave-uniform)
        float sel = 0.f;
        for (int s = 0; s < k; ++s) {
            const int is = __shfl(my_i, s);
            const float gs = __shfl(gv, s);
            if (is == e) sel += gs;
        }
        if (e < E) {
            const float pe = expf(to_f32(x[e]) - l);
            y[e] = from_f32<T>(norm_topk ? pe * sel : pe * (sel - dot));
        }
    }
}

template <typename T>
__global__ __launch_bounds__(64 * ER_STRIPS) void moe_expert_relevance_kernel(const long long* __restrict__ idx, const T* __restrict__ w,
                                                                             const T* __restrict__ gw, float* __restrict__ out, int S, int k,
                                                                             int E) {
    __shared__ __attribute__((aligned(16))) int s_e[ER_CHUNK];
    __shared__ __attribute__((aligned(16))) float s_v[ER_CHUNK];
    __shared__ float s_part[ER_STRIPS][64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, strip = threadIdx.x >> 6;
    const int e = blockIdx.y * 64 + lane;
    const int64_t n = (int64_t)S * k, base = (int64_t)b * n;
    float acc = 0.f;
    for (int64_t c0 = 0; c0 < n; c0 += ER_CHUNK) {
        const int len = (int)(n - c0 < ER_CHUNK ? n - c0 : ER_CHUNK);
        __syncthreads();
        for (int i = threadIdx.x; i < ER_CHUNK; i += 64 * ER_STRIPS) {
            int ei = -1;
            float v = 0.f;
            if (i < len) {
                const long long ix = idx[base + c0 + i];
                if (ix >= 0 && ix < E) { ei = (int)ix; v = to_f32(w[base + c0 + i]) * to_f32(gw[base + c0 + i]); }
            }
            s_e[i] = ei;
            s_v[i] = v;
        }
        __syncthreads();
        // wave `strip` walks its fixed slice of the chunk in order; every lane reads the same 16 bytes (LDS broadcast), no branch
        constexpr int Q = ER_CHUNK / ER_STRIPS;
#pragma unroll 4
        for (int i = strip * Q; i < (strip + 1) * Q; i += 4) {
            const int4 ee = *reinterpret_cast<const int4*>(&s_e[i]);
            const float4 vv = *reinterpret_cast<const float4*>(&s_v[i]);
            acc += ee.x == e ? vv.x : 0.f;
            acc += ee.y == e ? vv.y : 0.f;
            acc += ee.z == e ? vv.z : 0.f;
            acc += ee.w == e ? vv.w : 0.f;
        }
    }
    s_part[strip][lane] = acc;
    __syncthreads();
    if (strip == 0 && e < E) {
        float t = s_part[0][lane];
#pragma unroll
        for (int r = 1; r < ER_STRIPS; ++r) t += s_part[r][lane];
        out[(int64_t)b * E + e] = t;
    }
}

inline bool al(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline int esz(int dtype) { return dtype == LRP_F32 ? 4 : 2; }

int check_router(int T, int E, int k, int dtype) {
    if (T < 1 || E < 1 || k < 1 || (dtype != LRP_F32 && dtype != LRP_BF16)) return LRP_EINVAL;
    if (E > RT_EMAX || k > RT_KMAX || k > E || (int64_t)T * k >= (1ll << 30)) return LRP_ESHAPE;
    return LRP_OK;
}
// a [T, E] operand with row pitch ld, read and written element by element: every row starts on the 4-byte grid (bf16: an even pitch;
// E = 60 experts in bf16 are 120-byte rows, which a 16-byte rule would refuse for no reason of the kernel's)
int check_rows(const void* p, int64_t ld, int E, int dtype) {
    if (ld < E) return LRP_ESHAPE;
    if (!al(p, 4) || (ld * esz(dtype)) % 4 != 0) return LRP_EALIGN;
    return LRP_OK;
}

template <typename T>
void launch_fwd(int nj, dim3 grid, dim3 block, hipStream_t st, const T* logits, long long* idx, T* w, float* lse, int Tn, int E, int k,
                int64_t ldl, int norm_topk) {
#define RT_FWD(NJ) hipLaunchKernelGGL((moe_router_fwd_kernel<T, NJ>), grid, block, 0, st, logits, idx, w, lse, Tn, E, k, ldl, norm_topk)
    if (nj <= 1) RT_FWD(1);
    else if (nj <= 2) RT_FWD(2);
    else if (nj <= 4) RT_FWD(4);
    else if (nj <= 8) RT_FWD(8);
    else RT_FWD(RT_PER_LANE);
#undef RT_FWD
}

}  // namespace

extern "C" int lrp_moe_router_fwd(const void* logits, void* idx, void* w, float* lse, int T, int E, int k, int64_t ldl, int norm_topk,
                                  int dtype, void* stream) {
    if (!logits || !idx || !w || !lse) return LRP_EINVAL;
    int rc = check_router(T, E, k, dtype);
    if (rc != LRP_OK) return rc;
    if ((rc = check_rows(logits, ldl, E, dtype)) != LRP_OK) return rc;
    if (!al(idx, 8) || !al(w, esz(dtype)) || !al(lse, 4)) return LRP_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((T + RT_ROWS - 1) / RT_ROWS), block(64 * RT_ROWS);
    const int nj = (E + 63) / 64;
    if (dtype == LRP_BF16)
        launch_fwd<bf16_t>(nj, grid, block, st, (const bf16_t*)logits, (long long*)idx, (bf16_t*)w, lse, T, E, k, ldl, norm_topk);
    else
        launch_fwd<float>(nj, grid, block, st, (const float*)logits, (long long*)idx, (float*)w, lse, T, E, k, ldl, norm_topk);
    return lrp_check_launch();
}

extern "C" int lrp_moe_router_bwd(const void* logits, const float* lse, const void* idx, const void* w, const void* gw, void* g_logits,
                                  int T, int E, int k, int64_t ldl, int64_t ldg, int norm_topk, int dtype, void* stream) {
    if (!logits || !lse || !idx || !w || !gw || !g_logits) return LRP_EINVAL;
    int rc = check_router(T, E, k, dtype);
    if (rc != LRP_OK) return rc;
    if ((rc = check_rows(logits, ldl, E, dtype)) != LRP_OK) return rc;
    if ((rc = check_rows(g_logits, ldg, E, dtype)) != LRP_OK) return rc;
    if (!al(idx, 8) || !al(w, esz(dtype)) || !al(gw, esz(dtype)) || !al(lse, 4)) return LRP_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((T + RT_ROWS - 1) / RT_ROWS), block(64 * RT_ROWS);
    if (dtype == LRP_BF16)
        hipLaunchKernelGGL(moe_router_bwd_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)logits, lse, (const long long*)idx,
                           (const bf16_t*)gw, (bf16_t*)g_logits, T, E, k, ldl, ldg, norm_topk);
    else
        hipLaunchKernelGGL(moe_router_bwd_kernel<float>, grid, block, 0, st, (const float*)logits, lse, (const long long*)idx,
                           (const float*)gw, (float*)g_logits, T, E, k, ldl, ldg, norm_topk);
    return lrp_check_launch();
}

extern "C" int lrp_moe_expert_relevance(const void* idx, const void* w, const void* gw, float* out, int B, int S, int k, int E, int dtype,
                                        void* stream) {
    if (!idx || !w || !gw || !out || B < 1 || S < 1) return LRP_EINVAL;
    const int rc = check_router((int)std::min<int64_t>((int64_t)B * S, INT32_MAX), E, k, dtype);
    if (rc != LRP_OK) return rc;
    if ((int64_t)B * S * k >= (1ll << 30) || B > 65535) return LRP_ESHAPE;
    if (!al(idx, 8) || !al(w, esz(dtype)) || !al(gw, esz(dtype)) || !al(out, 4)) return LRP_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(B, (E + 63) / 64), block(64 * ER_STRIPS);
    if (dtype == LRP_BF16)
        hipLaunchKernelGGL(moe_expert_relevance_kernel<bf16_t>, grid, block, 0, st, (const long long*)idx, (const bf16_t*)w, (const bf16_t*)gw,
                           out, S, k, E);
    else
        hipLaunchKernelGGL(moe_expert_relevance_kernel<float>, grid, block, 0, st, (const long long*)idx, (const float*)w, (const float*)gw,
                           out, S, k, E);
    return lrp_check_launch();
}
