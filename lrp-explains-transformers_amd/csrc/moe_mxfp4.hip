// moe_mxfp4.hip -- the four grouped expert GEMMs of moe.hip with the expert weights held as MXFP4 (include/lrp_hip_moe_mxfp4.h): the same
// kernel template (moe_gemm.hpp) instantiated with QB, which loads codes + scale bytes in place of the bf16 / fp32 B tile and decodes them
// between the global load and the LDS write.  No scratch copy of the weights, no extra launch; plans, A gathers, placement and epilogues are
// moe.hip's.  A separate translation unit so that the unquantised instantiations of moe.hip compile exactly as they did.
#include "moe_gemm.hpp"

namespace {

// codes on the 16-byte grid (one 16 / 8-byte vector load per thread and stage), scales on the 4-byte grid (the format's own rule)
int check_q(const void* codes, const void* scales) {
    if (!codes || !scales) return LRP_EINVAL;
    if (!al16(codes) || (reinterpret_cast<uintptr_t>(scales) & 3)) return LRP_EALIGN;
    return LRP_OK;
}

}  // namespace

extern "C" int lrp_moe_gate_up_fwd_q(const void* x, const void* codes, const void* scales, const int* plan, void* coef, void* m, int T, int k,
                                     int E, int H, int I, int64_t ldx, int64_t ldcoef, int64_t ldm, int act, int dtype, void* stream) {
    MOE_CHECK(check_dims(T, k, E, H, I, dtype));
    if (!plan) return LRP_EINVAL;
    if (act != LRP_ACT_SILU && act != LRP_ACT_GELU_TANH) return LRP_EINVAL;
    MOE_CHECK(check_mat(x, ldx, H, dtype));
    MOE_CHECK(check_q(codes, scales));
    MOE_CHECK(check_mat(coef, ldcoef, 2 * (int64_t)I, dtype));
    MOE_CHECK(check_mat(m, ldm, I, dtype));
    MoeGemmArgs a = base_args(plan, T, k, E, H, I);
    a.A = x; a.lda = ldx;
    a.B = codes; a.Bsc = scales; a.sB = 2 * (int64_t)I * H; a.ldb = H;
    a.C = m; a.ldc = ldm; a.coef = coef; a.ldcoef = ldcoef;
    a.N = 2 * I; a.K = H;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == LRP_BF16)
        return act == LRP_ACT_SILU ? launch_gemm<bf16_t, A_GATHER, B_NT_GU, EP_COEF, LRP_ACT_SILU, true>(a, st)
                                   : launch_gemm<bf16_t, A_GATHER, B_NT_GU, EP_COEF, LRP_ACT_GELU_TANH, true>(a, st);
    return act == LRP_ACT_SILU ? launch_gemm<float, A_GATHER, B_NT_GU, EP_COEF, LRP_ACT_SILU, true>(a, st)
                               : launch_gemm<float, A_GATHER, B_NT_GU, EP_COEF, LRP_ACT_GELU_TANH, true>(a, st);
}

extern "C" int lrp_moe_down_fwd_q(const void* m, const void* codes, const void* scales, const int* plan, void* y, int T, int k, int E, int H,
                                  int I, int64_t ldm, int64_t ldy, int dtype, void* stream) {
    MOE_CHECK(check_dims(T, k, E, H, I, dtype));
    if (!plan) return LRP_EINVAL;
    MOE_CHECK(check_mat(m, ldm, I, dtype));
    MOE_CHECK(check_q(codes, scales));
    MOE_CHECK(check_mat(y, ldy, H, dtype));
    MoeGemmArgs a = base_args(plan, T, k, E, H, I);
    a.A = m; a.lda = ldm;
    a.B = codes; a.Bsc = scales; a.sB = (int64_t)H * I; a.ldb = I;
    a.C = y; a.ldc = ldy;
    a.N = H; a.K = I;
    hipStream_t st = (hipStream_t)stream;
    return dtype == LRP_BF16 ? launch_gemm<bf16_t, A_ROWS, B_NT, EP_STORE, 0, true>(a, st)
                             : launch_gemm<float, A_ROWS, B_NT, EP_STORE, 0, true>(a, st);
}

extern "C" int lrp_moe_down_dgrad_q(const void* G, const void* codes, const void* scales, const void* coef, const void* m, const void* w,
                                    const int* plan, void* Agu, float* gw_part, int T, int k, int E, int H, int I, int64_t ldg, int64_t ldcoef,
                                    int64_t ldm, int64_t ldagu, int dtype, void* stream) {
    MOE_CHECK(check_dims(T, k, E, H, I, dtype));
    if (!plan || !w || !gw_part) return LRP_EINVAL;
    if ((reinterpret_cast<uintptr_t>(w) % esz(dtype)) || (reinterpret_cast<uintptr_t>(gw_part) & 3)) return LRP_EALIGN;
    MOE_CHECK(check_mat(G, ldg, H, dtype));
    MOE_CHECK(check_q(codes, scales));
    MOE_CHECK(check_mat(coef, ldcoef, 2 * (int64_t)I, dtype));
    MOE_CHECK(check_mat(m, ldm, I, dtype));
    MOE_CHECK(check_mat(Agu, ldagu, 2 * (int64_t)I, dtype));
    MoeGemmArgs a = base_args(plan, T, k, E, H, I);
    a.A = G; a.lda = ldg;
    a.B = codes; a.Bsc = scales; a.sB = (int64_t)H * I; a.ldb = I;
    a.C = Agu; a.ldc = ldagu; a.coef = const_cast<void*>(coef); a.ldcoef = ldcoef;
    a.m = m; a.ldm = ldm; a.w = w; a.gwp = gw_part;
    a.N = I; a.K = H;
    hipStream_t st = (hipStream_t)stream;
    return dtype == LRP_BF16 ? launch_gemm<bf16_t, A_GATHER, B_NN, EP_DGRAD, 0, true>(a, st)
                             : launch_gemm<float, A_GATHER, B_NN, EP_DGRAD, 0, true>(a, st);
}

extern "C" int lrp_moe_gate_up_dgrad_q(const void* Agu, const void* codes, const void* scales, const int* plan, void* gx_rows, int T, int k,
                                       int E, int H, int I, int64_t ldagu, int64_t ldgx, int dtype, void* stream) {
    MOE_CHECK(check_dims(T, k, E, H, I, dtype));
    if (!plan) return LRP_EINVAL;
    MOE_CHECK(check_mat(Agu, ldagu, 2 * (int64_t)I, dtype));
    MOE_CHECK(check_q(codes, scales));
    MOE_CHECK(check_mat(gx_rows, ldgx, H, dtype));
    MoeGemmArgs a = base_args(plan, T, k, E, H, I);
    a.A = Agu; a.lda = ldagu;
    a.B = codes; a.Bsc = scales; a.sB = 2 * (int64_t)I * H; a.ldb = H;
    a.C = gx_rows; a.ldc = ldgx;
    a.N = H; a.K = 2 * I;
    hipStream_t st = (hipStream_t)stream;
    return dtype == LRP_BF16 ? launch_gemm<bf16_t, A_ROWS, B_NN, EP_STORE, 0, true>(a, st)
                             : launch_gemm<float, A_ROWS, B_NN, EP_STORE, 0, true>(a, st);
}
