// sample.hip -- the next token of a sampled continuation (include/lrp_hip_sample.h: lrp_sample_rows).
//
// One workgroup per row of fp32 logits [B, V] (256 threads; 1024 for V > 8192).  The row is never sorted.  Passes over the row (the first
// streams it from HBM, the later ones are L2 hits -- a row of V = 262208 is 1 MB, more than the LDS):
//   1      max
//   2..5   top-k: radix select of the k-th largest value over the order-preserving 32-bit image of the logits, four 8-bit digits from the top,
//          a 256-bin histogram of COUNTS per digit
//   6..9   top-p: the same select on MASS (q = exp((l - max) / T) of the rows inside the top-k set); the first digit's total is Z_k
//   10     the draw: kept mass per chunk of the row in index order, a scan of the chunk totals, then the chosen chunk element by element
// A filter that is off costs no pass (all off: 1 and 10 only).  16-byte loads where base and pitch are on the 16-byte grid, element by element
// otherwise and on the row's tail.
//
// Determinism: every mass is a FIXED-POINT integer (44 fractional bits in 64, q <= 1 so a row of 2^18 entries cannot overflow); integer sums
// are associative, so LDS atomics on the histograms, the 16 histogram copies, the wave scans and the chunk order all give one result whatever
// the arrival order, the vector width or the row pitch -- bitwise repeatable, no global atomics, a row does not see the other rows.  The price:
// a mass below 2^-44 of the maximum's counts as 0 (such a token is kept and counted but never drawn), and 64-bit LDS adds.
#include "common.hpp"

namespace {

constexpr int NCOPY = 16;           // histogram copies, lane & 15 picks one: a hot bin (most of a row shares its top digit) is hit 4 lanes deep, not 64
constexpr int HPITCH = 257;         // bins of one copy + 1: the copies of one bin lie in different banks
constexpr int MAXCHUNK = 1024;      // chunks of the draw pass (<= threads of the workgroup: one thread per chunk in the scan)
constexpr float FIX_HALF = 4194304.f;          // 2^22: a mass is taken to 44 fractional bits in two exact halves

struct SampleShared {
    unsigned long long hist[NCOPY * HPITCH];
    unsigned long long tot[MAXCHUNK];
    unsigned long long wtot[16];
    unsigned long long sel_excl;
    int sel;
    int ired[2][16];
    float red[16];
};

// f(x, c) over the row p[0 .. V), c the column: the first 4 nv elements as 16-byte vectors (nv = 0: an unaligned row), the rest one by one
template <int NT, typename F>
LRP_DEVICE void sample_row_pass(const float* __restrict__ p, int V, int nv, F f) {
    int q = threadIdx.x;
    for (; q + 3 * NT < nv; q += 4 * NT) {
        f32x4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const f32x4*>(p + 4 * (q + u * NT));
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) f(x[u][e], 4 * (q + u * NT) + e);
    }
    for (; q < nv; q += NT) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(p + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) f(x[e], 4 * q + e);
    }
    for (int c = 4 * nv + threadIdx.x; c < V; c += NT) f(p[c], c);
}

// the order-preserving image: a >= b as floats <=> okey(a) >= okey(b) as unsigned (x + 0 takes -0 to +0: the two compare equal)
LRP_DEVICE uint32_t okey(float x) {
    const uint32_t b = __float_as_uint(x + 0.0f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// q = exp((x - m) / T) in [0, 1] as a fixed-point integer, 2^44 = 1
LRP_DEVICE unsigned long long qfix(float x, float m, float T) {
    float q = expf((x - m) / T);
    q = q >= 0.f ? fminf(q, 1.f) : 0.f;          // (NaN -> 0)
    const float s = q * FIX_HALF;
    const uint32_t hi = (uint32_t)s;
    const uint32_t lo = (uint32_t)((s - (float)hi) * FIX_HALF);
    return ((unsigned long long)hi << 22) | lo;
}

LRP_DEVICE unsigned long long wave_sum_u64(unsigned long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
LRP_DEVICE unsigned long long wave_scan_u64(unsigned long long x) {          // inclusive, in lane order
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(x, o, 64);
        if (lane >= o) x += t;
    }
    return x;
}
// inclusive scan in thread order over the workgroup; total to every thread
template <int NT>
LRP_DEVICE unsigned long long block_scan_u64(unsigned long long v, unsigned long long* wtot, unsigned long long& total) {
    const int w = threadIdx.x >> 6;
    const unsigned long long incl = wave_scan_u64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 63) wtot[w] = incl;
    __syncthreads();
    unsigned long long off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) {
        const unsigned long long x = wtot[i];
        if (i < w) off += x;
        tot += x;
    }
    total = tot;
    return incl + off;
}

// Radix select from the top over the keys of the row's elements with in_set(key), each weighing wt(x) (1: a count; qfix: a mass).
// target(total) of the first digit's histogram gives the rank sought; -> the key K with  weight(keys > K) < rank <= weight(keys >= K):
// a key of the row (the last digit's bin is not empty).
template <int NT, typename InSet, typename Wt, typename Tgt>
LRP_DEVICE uint32_t radix_select(const float* __restrict__ p, int V, int nv, SampleShared& sh, InSet in_set, Wt wt, Tgt target) {
    const int tid = threadIdx.x;
    uint32_t prefix = 0;
    unsigned long long rank = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < NCOPY * HPITCH; i += NT) sh.hist[i] = 0;
        if (tid == 0) { sh.sel = 0; sh.sel_excl = 0; }
        __syncthreads();
        const uint32_t himask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        unsigned long long* mine = sh.hist + (tid & (NCOPY - 1)) * HPITCH;
        sample_row_pass<NT>(p, V, nv, [&](float x, int) {
            const uint32_t k = okey(x);
            if (((k ^ prefix) & himask) == 0 && in_set(k)) {
                const unsigned long long w = wt(x);
                if (w) atomicAdd(mine + ((k >> shift) & 255), w);
            }
        });
        __syncthreads();
        unsigned long long v = 0;          // thread t holds bin 255 - t: the scan runs from the largest digit down
        if (tid < 256)
#pragma unroll
            for (int c = 0; c < NCOPY; ++c) v += sh.hist[c * HPITCH + 255 - tid];
        unsigned long long total;
        const unsigned long long incl = block_scan_u64<NT>(v, sh.wtot, total);
        if (shift == 24) rank = target(total);
        if (tid < 256 && incl - v < rank && rank <= incl) { sh.sel = 255 - tid; sh.sel_excl = incl - v; }
        __syncthreads();
        prefix |= (uint32_t)sh.sel << shift;
        rank -= sh.sel_excl;
        __syncthreads();
    }
    return prefix;
}

// Philox4x32-10: key (k0, k1), counter (c0, c1, 0, 0) -> word 0
LRP_DEVICE uint32_t philox_word0(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1) {
    uint32_t c2 = 0, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

template <int NT>
__global__ __launch_bounds__(NT) void sample_rows_kernel(const float* __restrict__ logits, int64_t ldl, int V, float T, int top_k, float top_p,
                                                         float min_p, const int64_t* __restrict__ seeds, const int* __restrict__ streams,
                                                         int step, const float* __restrict__ u_in, int* __restrict__ idx,
                                                         float* __restrict__ slp, int* __restrict__ n_kept, float* __restrict__ u_out, int vec) {
    __shared__ SampleShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = NT / 64;
    const int64_t r = blockIdx.x;
    const float* p = logits + r * ldl;
    const int nv = vec ? V / 4 : 0;

    float u;
    if (u_in) {
        u = u_in[r];
        u = u >= 0.f ? fminf(u, 0.99999994f) : 0.f;          // (the caller's contract is [0, 1); NaN -> 0)
    } else {
        const uint64_t s = (uint64_t)seeds[r];
        u = (float)(philox_word0((uint32_t)s, (uint32_t)(s >> 32), (uint32_t)step, streams ? (uint32_t)streams[r] : 0u) >> 8) * 5.9604644775390625e-8f;
    }

    float m = -INFINITY;
    sample_row_pass<NT>(p, V, nv, [&](float x, int) { m = fmaxf(m, x); });
    m = block_max(m, sh.red);
    __syncthreads();

    // the kept set is { j : okey(l_j) >= tau }: the largest of the filters' thresholds
    uint32_t tau = 0;
    if (top_k >= 1 && top_k < V)
        tau = radix_select<NT>(p, V, nv, sh, [](uint32_t) { return true; }, [](float) { return 1ull; },
                               [&](unsigned long long) { return (unsigned long long)top_k; });
    if (top_p < 1.f) {
        // keep j iff the mass of the kept tokens with a larger logit is < top_p Z_k: the key at which the mass from the top reaches ceil(top_p Z_k)
        const uint32_t tau_k = tau;
        const uint32_t tau_p = radix_select<NT>(p, V, nv, sh, [&](uint32_t k) { return k >= tau_k; }, [&](float x) { return qfix(x, m, T); },
                                                [&](unsigned long long zk) {
                                                    unsigned long long P = (unsigned long long)ceil((double)top_p * (double)zk);
                                                    P = P < zk ? P : zk;
                                                    return P > 0 ? P : 1ull;
                                                });
        tau = tau_p > tau ? tau_p : tau;
    }
    if (min_p > 0.f) {
        // l_j >= m + T log(min_p), the threshold formed in fp64 and rounded UP to a float: the comparison on floats is then the fp64 one
        const double thr = (double)m + (double)T * log((double)min_p);
        float f = (float)thr;
        if ((double)f < thr) f = nextafterf(f, INFINITY);
        const uint32_t tau_m = okey(f);
        tau = tau_m > tau ? tau_m : tau;
    }

    // the draw.  Chunk c is the columns [c CL, (c + 1) CL), CL a multiple of 256, at most MAXCHUNK (<= NT) chunks; a wave takes a chunk 256
    // columns at a time, lane L the 4 columns from 4 L
    constexpr int CMAX = NT < MAXCHUNK ? NT : MAXCHUNK;
    const int64_t CLu = (((int64_t)V + CMAX - 1) / CMAX + 255) / 256 * 256;          // (V >= 1: at least 256)
    const int NC = (int)(((int64_t)V + CLu - 1) / CLu);
    int kept = 0, last = -1;
    auto lane4 = [&](int64_t i0, unsigned long long* qf) {          // the lane's four columns from i0 -> their kept masses, in column order
        float x[4];
        if (nv > 0 && i0 + 3 < 4 * (int64_t)nv) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(p + i0);
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = t[e];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = i0 + e < V ? p[i0 + e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = i0 + e < V && okey(x[e]) >= tau;
            qf[e] = in ? qfix(x[e], m, T) : 0ull;
            if (in) { ++kept; last = (int)(i0 + e); }
        }
    };
    for (int c = wave; c < NC; c += NW) {
        const int64_t end = (c + 1) * CLu < V ? (c + 1) * CLu : V;
        unsigned long long s = 0;
        for (int64_t base = c * CLu; base < end; base += 256) {
            unsigned long long qf[4];
            lane4(base + 4 * lane, qf);
            s += ((qf[0] + qf[1]) + qf[2]) + qf[3];
        }
        s = wave_sum_u64(s);
        if (lane == 0) sh.tot[c] = s;
    }
    const int kept_mine = kept;
    if (tid == 0) { sh.sel = -1; sh.sel_excl = 0; }
    __syncthreads();
    const unsigned long long v = tid < NC ? sh.tot[tid] : 0ull;
    unsigned long long Z;
    const unsigned long long incl = block_scan_u64<NT>(v, sh.wtot, Z);
    // the first kept j whose running mass exceeds u Z (top_k = 1 is the arg-max: the first of the tied maxima whatever u)
    unsigned long long goal = top_k == 1 ? 0ull : (unsigned long long)((double)u * (double)Z);
    if (Z && goal >= Z) goal = Z - 1;
    if (tid < NC && incl - v <= goal && goal < incl) { sh.sel = tid; sh.sel_excl = incl - v; }
    // kept count and the last kept column
    int ks = kept_mine, lm = last;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ks += __shfl_xor(ks, o, 64);
        const int t = __shfl_xor(lm, o, 64);
        lm = t > lm ? t : lm;
    }
    if (lane == 0) { sh.ired[0][wave] = ks; sh.ired[1][wave] = lm; }
    __syncthreads();
    if (wave != 0) return;
    int nk = 0, lk = -1;
    for (int i = 0; i < NW; ++i) {
        nk += sh.ired[0][i];
        lk = sh.ired[1][i] > lk ? sh.ired[1][i] : lk;
    }
    int tok = -1;
    const int c = sh.sel;
    if (c >= 0) {
        unsigned long long run = sh.sel_excl;
        const int64_t end = (c + 1) * CLu < V ? (c + 1) * CLu : V;
        for (int64_t base = c * CLu; base < end && tok < 0; base += 256) {
            unsigned long long qf[4];
            lane4(base + 4 * lane, qf);
            const unsigned long long s = ((qf[0] + qf[1]) + qf[2]) + qf[3];
            const unsigned long long inc = wave_scan_u64(s);
            const unsigned long long hit = __ballot(run + inc > goal);
            if (hit) {
                const int L = __ffsll((long long)hit) - 1;
                int t = -1;
                unsigned long long a = run + inc - s;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a += qf[e];
                    if (t < 0 && a > goal) t = (int)(base + 4 * lane + e);
                }
                tok = __shfl(t, L, 64);
            } else {
                run += __shfl(inc, 63, 64);
            }
        }
    }
    if (tok < 0) tok = lk;          // (no mass anywhere -- not a row of the caller's contract: the last kept column)
    tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
    if (lane == 0) {
        idx[r] = tok;
        if (slp) slp[r] = (p[tok] - m) / T - logf((float)((double)Z * (1.0 / 17592186044416.0)));
        if (n_kept) n_kept[r] = nk;
        if (u_out) u_out[r] = u;
    }
}

inline bool on16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool onN(const void* p, int n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

}  // namespace

extern "C" int lrp_sample_rows(const float* logits, int64_t ld_logits, int B, int V, float temperature, int top_k, float top_p, float min_p,
                               const int64_t* seeds, const int* streams, int step, const float* u_in, int* idx, float* sample_logprob,
                               int* n_kept, float* u_out, void* stream) {
    if (!logits || !idx || (!seeds && !u_in) || B < 0 || V < 1) return LRP_EINVAL;
    if (!(temperature > 0.f) || !(temperature <= 3.4028234663852886e38f)) return LRP_EINVAL;
    if (top_k < 0 || !(top_p > 0.f) || !(min_p >= 0.f) || !(min_p <= 1.f) || step < 0) return LRP_EINVAL;
    if (ld_logits < V) return LRP_ESHAPE;
    if (!onN(logits, 4) || !onN(seeds, 8) || !onN(streams, 4) || !onN(u_in, 4) || !onN(idx, 4) || !onN(sample_logprob, 4) || !onN(n_kept, 4) ||
        !onN(u_out, 4))
        return LRP_EALIGN;
    if (B == 0) return LRP_OK;
    hipStream_t st = (hipStream_t)stream;
    const int vec = on16(logits) && ld_logits % 4 == 0;
    if (V > 8192)
        hipLaunchKernelGGL((sample_rows_kernel<1024>), dim3((unsigned)B), dim3(1024), 0, st, logits, ld_logits, V, temperature, top_k, top_p, min_p,
                           seeds, streams, step, u_in, idx, sample_logprob, n_kept, u_out, vec);
    else
        hipLaunchKernelGGL((sample_rows_kernel<256>), dim3((unsigned)B), dim3(256), 0, st, logits, ld_logits, V, temperature, top_k, top_p, min_p,
                           seeds, streams, step, u_in, idx, sample_logprob, n_kept, u_out, vec);
    return lrp_check_launch();
}
