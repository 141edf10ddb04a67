// span.hip -- the head seed of an answer-span explanation (include/lrp_hip_span.h: lrp_span_seed).
//
// One workgroup per explained row of fp32 logits [R, V].  HBM / L2-bound: pass 1 (max) streams the row from HBM, pass 2 (sum of exp) and
// pass 3 (the dense seed of the log-probability objective) re-read it from L2 -- a row of V = 128256 is 513 KB.  16-byte loads (four in
// flight per thread in the two reduction passes) and 16-byte stores of the seed where bases and pitches allow, element by element
// otherwise and on the row's tail.  No LDS beyond the cross-wave reduction of common.hpp.
//
// Order of the sums (bitwise repeatable, independent of the other rows): a thread adds the elements of its vectors in index order, lane e of
// a vector into accumulator e, then (s0 + s1) + (s2 + s3), then its tail elements; wave_sum's butterfly; the waves in wave order.
#include "common.hpp"

namespace {

// f(x, c) over the row p[0 .. V): the first 4 nv elements as 16-byte vectors (nv = 0: an unaligned row), the rest element by element
template <int NT, typename F>
LRP_DEVICE void span_row_pass(const float* __restrict__ p, int V, int nv, F f) {
    int q = threadIdx.x;
    for (; q + 3 * NT < nv; q += 4 * NT) {
        f32x4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const f32x4*>(p + 4 * (q + u * NT));
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) f(x[u][e], e);
    }
    for (; q < nv; q += NT) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(p + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) f(x[e], e);
    }
    for (int c = 4 * nv + threadIdx.x; c < V; c += NT) f(p[c], 4);
}

template <typename ST, int NT>
__global__ __launch_bounds__(NT) void span_seed_kernel(const float* __restrict__ logits, int64_t ldl, const int* __restrict__ idx,
                                                       const float* __restrict__ w, const float* __restrict__ rstd, int V,
                                                       ST* __restrict__ seed, int64_t lds, float* __restrict__ logit,
                                                       float* __restrict__ logprob, float* __restrict__ rs, int vec_l, int vec_s) {
    constexpr int SW = 16 / sizeof(ST);          // seed elements of one 16-byte store
    __shared__ float red[NT / 64];
    const int64_t r = blockIdx.x;
    const float* p = logits + r * ldl;
    const int nv = vec_l ? V / 4 : 0;
    float m = -INFINITY;
    span_row_pass<NT>(p, V, nv, [&](float x, int) { m = fmaxf(m, x); });
    m = block_max(m, red);
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    span_row_pass<NT>(p, V, nv, [&](float x, int e) { acc[e] += expf(x - m); });
    const float s = block_sum(((acc[0] + acc[1]) + (acc[2] + acc[3])) + acc[4], red);
    const int i = idx[r];
    const bool in = (unsigned)i < (unsigned)V;
    const float wr = w ? w[r] : 1.f;
    if (threadIdx.x == 0) {
        const float li = in ? p[i] : NAN;
        logit[r] = li;
        logprob[r] = (li - m) - logf(s);
        if (rs) rs[r] = wr * rstd[r];
    }
    if (!seed) return;
    ST* o = seed + r * lds;
    auto val = [&](float x, int c) { return wr * ((c == i ? 1.f : 0.f) - expf(x - m) / s); };
    const int nvs = vec_s ? V / SW : 0;
#pragma unroll 2
    for (int q = threadIdx.x; q < nvs; q += NT) {
        const int c0 = q * SW;
        Vec16<ST> out;
#pragma unroll
        for (int h = 0; h < SW / 4; ++h) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(p + c0 + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) out.set(4 * h + e, val(x[e], c0 + 4 * h + e));
        }
        st16(o + c0, out);
    }
    for (int c = nvs * SW + threadIdx.x; c < V; c += NT) o[c] = from_f32<ST>(val(p[c], c));
}

inline bool on16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool on4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

template <typename ST>
void span_launch(const float* logits, int64_t ldl, const int* idx, const float* w, const float* rstd, int R, int V, ST* seed, int64_t lds,
                 float* logit, float* logprob, float* rs, hipStream_t st) {
    constexpr int SW = 16 / sizeof(ST);
    const int vec_l = on16(logits) && ldl % 4 == 0;
    const int vec_s = seed && vec_l && on16(seed) && lds % SW == 0;
    if (V > 8192)
        hipLaunchKernelGGL((span_seed_kernel<ST, 1024>), dim3((unsigned)R), dim3(1024), 0, st, logits, ldl, idx, w, rstd, V, seed, lds, logit,
                           logprob, rs, vec_l, vec_s);
    else
        hipLaunchKernelGGL((span_seed_kernel<ST, 256>), dim3((unsigned)R), dim3(256), 0, st, logits, ldl, idx, w, rstd, V, seed, lds, logit,
                           logprob, rs, vec_l, vec_s);
}

}  // namespace

extern "C" int lrp_span_seed(const float* logits, int64_t ld_logits, const int* idx, const float* w, const float* rstd, int R, int V,
                             int objective, void* seed, int64_t ld_seed, int seed_dtype, float* logit, float* logprob, float* rs,
                             void* stream) {
    if (!logits || !idx || !logit || !logprob || R < 0 || V < 1 || (objective != LRP_SPAN_LOGIT && objective != LRP_SPAN_LOGPROB))
        return LRP_EINVAL;
    const bool dense = objective == LRP_SPAN_LOGPROB;
    if (dense && (!seed || (seed_dtype != LRP_F32 && seed_dtype != LRP_BF16))) return LRP_EINVAL;
    if (rs && !rstd) return LRP_EINVAL;
    if (ld_logits < V || (dense && ld_seed < V)) return LRP_ESHAPE;
    if (!on4(logits) || !on4(idx) || !on4(w) || !on4(rstd) || !on4(logit) || !on4(logprob) || !on4(rs)) return LRP_EALIGN;
    if (dense && (reinterpret_cast<uintptr_t>(seed) % (seed_dtype == LRP_BF16 ? 2 : 4))) return LRP_EALIGN;
    if (R == 0) return LRP_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!dense)
        span_launch<float>(logits, ld_logits, idx, w, rstd, R, V, nullptr, 0, logit, logprob, rs, st);
    else if (seed_dtype == LRP_F32)
        span_launch<float>(logits, ld_logits, idx, w, rstd, R, V, (float*)seed, ld_seed, logit, logprob, rs, st);
    else
        span_launch<bf16_t>(logits, ld_logits, idx, w, rstd, R, V, (bf16_t*)seed, ld_seed, logit, logprob, rs, st);
    return lrp_check_launch();
}
