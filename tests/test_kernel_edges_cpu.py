"""CPU: argument checks that guard vector accesses and table reads of the HIP kernels -- every call below is rejected before anything is
launched (C ABI: return codes on a dummy host buffer; ops wrappers: an exception ahead of the first pointer hand-over)."""
import ctypes

import pytest
import torch

BF = torch.bfloat16


def _aligned():
    """a 16-byte aligned address inside a live host buffer (never dereferenced: the calls are refused first)"""
    buf = (ctypes.c_char * 256)()
    return buf, (ctypes.addressof(buf) + 15) // 16 * 16


def test_gated_coef_gemms_check_stash_and_output_alignment():
    """lrp_gemm_gated_fwd_coef / _bwd_coef store the coefficient stash, m and Agu (and load the stash) 16 bytes at a time: LRP_EALIGN unless
    coef, m, Agu are 16-byte aligned and ldcoef, ldm, ldagu are multiples of 8 -- as lrp_gemm_res_ssq asks of raw / ldraw"""
    import lxt_amd._lib as L
    lib, BF16 = L.lib, L.BF16
    keep, A = _aligned()
    M, I, H = 8192, 14336, 4096
    assert lib.lrp_gemm_gated_coef_ok(M, I, H, H, 4224, H, 14400, 0, BF16) == 1
    # (x, Wgu, rs, coef, m, M, I, K, ldx, ldw, ldcoef, ldm, eps_g, eps_lin, act, dtype, stream)
    fwd = lambda x=A, w=A, coef=A, m=A, ldcoef=2 * I, ldm=I: lib.lrp_gemm_gated_fwd_coef(      # noqa: E731
        x, w, None, coef, m, M, I, H, H, 4224, ldcoef, ldm, 1e-10, 0.0, 0, BF16, None)
    assert fwd(x=A + 2) == -2 and fwd(w=A + 8) == -2                       # (the operand checks that were there)
    assert fwd(coef=A + 8) == -2 and fwd(coef=A + 2) == -2
    assert fwd(m=A + 8) == -2 and fwd(m=A + 4) == -2
    assert fwd(ldcoef=2 * I + 4) == -2 and fwd(ldcoef=2 * I + 1) == -2
    assert fwd(ldm=I + 4) == -2 and fwd(ldm=I + 7) == -2
    assert fwd(coef=None) == -1 and fwd(m=None) == -1                       # LRP_EINVAL ahead of everything
    assert lib.lrp_gemm_gated_fwd_coef(A, A, None, A + 8, A, 256, I, H, H, 4224, 2 * I, I, 1e-10, 0.0, 0, BF16, None) == -3      # shape first
    # (Adn, Wdn, coef, Agu, M, I, K, lda, ldw, ldcoef, ldagu, dtype, stream)
    bwd = lambda a=A, w=A, coef=A, agu=A, ldcoef=2 * I, ldagu=2 * I: lib.lrp_gemm_gated_bwd_coef(      # noqa: E731
        a, w, coef, agu, M, I, H, H, 14400, ldcoef, ldagu, BF16, None)
    assert bwd(a=A + 2) == -2 and bwd(w=A + 8) == -2
    assert bwd(coef=A + 8) == -2 and bwd(agu=A + 8) == -2 and bwd(agu=A + 2) == -2
    assert bwd(ldcoef=2 * I + 4) == -2 and bwd(ldagu=2 * I + 4) == -2 and bwd(ldagu=2 * I + 1) == -2
    assert bwd(coef=None) == -1 and bwd(agu=None) == -1
    assert lib.lrp_gemm_gated_bwd_coef(A, A, A + 8, A, 256, 512, H, H, 520, 1024, 1024, BF16, None) == -3
    del keep


def test_rope_gemm_predicates_on_an_odd_head_count():
    """rope_cols % 256 == 128 at head_dim 128 (an odd nq + nk): the un-biased fused QKV + RoPE GEMM takes it (the kernel decides per head), the
    biased one keeps its refusal; rope_cols must still be whole heads"""
    import lxt_amd._lib as L
    lib, BF16 = L.lib, L.BF16
    assert lib.lrp_gemm_nt_rs_rope_ok(3072, 4352, 128, 128, 128, 4352, 192, 4224, 128, BF16) == 1
    assert lib.lrp_gemm_nt_rs_rope_ok(9728, 1280, 192, 192, 192, 1280, 2432, 1152, 128, BF16) == 1
    assert lib.lrp_gemm_nt_rs_rope_ok(6144, 2304, 2048, 2048, 2048, 2304, 2048, 2176, 128, BF16) == 1
    assert lib.lrp_gemm_nt_rs_bias_rope_ok(3072, 4352, 128, 128, 128, 4352, 192, 4224, 128, BF16) == 0
    assert lib.lrp_gemm_nt_rs_rope_ok(3072, 4352, 128, 128, 128, 4352, 192, 4224 - 64, 128, BF16) == 0
    assert lib.lrp_gemm_nt_rs_rope_ok(3072, 4352, 128, 128, 128, 4352, 192, 4352 + 128, 128, BF16) == 0


def test_fused_row_chunk_shapes_are_taken():
    """the shapes of test_kernels_gpu.test_gemm_fused_epilogues_row_chunks: 512 rows at a row pitch of 2^21 elements (two row chunks of 256), K = 128,
    24320 columns = 190 tiles.  Every predicate says yes, and every entry point gets past LRP_ESHAPE: with a misaligned row operand it answers
    LRP_EALIGN, the check that follows the shape check (nothing is launched)"""
    import lxt_amd._lib as L
    lib, BF16 = L.lib, L.BF16
    keep, A = _aligned()
    M, K, N, P, seq = 512, 128, 24320, 2 ** 21, 512
    assert lib.lrp_gemm_norm_fused_ok(M, N, K, P, K, 0, BF16) == 1 and lib.lrp_gemm_norm_fused_ok(M, N, K, P, N, 1, BF16) == 1
    assert lib.lrp_gemm_norm_fused_ok(256, N, K, P, K, 0, BF16) == 0                                   # (one chunk alone is 95 tiles)
    assert lib.lrp_gemm_nt_rs_rope_ok(M, N, K, P, K, N, seq, 24064, 128, BF16) == 1
    assert lib.lrp_gemm_nt_rs_bias_rope_ok(M, N, K, P, K, N, seq, 23552, 128, BF16) == 1
    assert lib.lrp_gemm_nt_rs_rope_ok(M, N, K, P, K, N, 384, 24064, 128, BF16) == 0                    # (256-row chunks against prompts of 384)
    assert lib.lrp_gemm_gated_coef_ok(M, N, K, P, K, P, N, 0, BF16) == 1
    x = A + 2
    assert lib.lrp_gemm_gated_fwd_coef(x, A, A, A, A, M, N // 2, K, P, K, N, N // 2, 1e-10, 0.0, 0, BF16, None) == -2
    assert lib.lrp_gemm_gated_bwd_coef(x, A, A, A, M, N, K, P, N, 2 * N, 2 * N, BF16, None) == -2
    assert lib.lrp_gemm_res_ssq(x, A, A, A, A, M, N, K, P, K, N, N, M, A, N, BF16, None) == -2
    assert lib.lrp_gemm_nt_rs(x, A, A, A, M, N, K, P, K, N, BF16, None) == -2
    assert lib.lrp_gemm_nt_rs_rope(x, A, A, A, A, A, M, N, K, P, K, N, seq, 24064, 128, BF16, None) == -2
    assert lib.lrp_gemm_nt_rs_bias(x, A, A, A, A, M, N, K, P, K, N, BF16, None) == -2
    assert lib.lrp_gemm_nt_rs_bias_rope(x, A, A, A, A, A, A, M, N, K, P, K, N, seq, 23552, 128, BF16, None) == -2
    assert lib.lrp_gemm_nn_rs(x, A, A, A, M, N, K, P, N, N, BF16, None) == -2
    assert lib.lrp_gemm_nn_rs_res(x, A, A, A, A, M, N, K, P, N, N, N, BF16, None) == -2
    del keep


def _site_operands(rows, nq, nk, d, seq):
    e = lambda c, dt=BF: torch.zeros(rows, c, dtype=dt)      # noqa: E731
    tab = torch.zeros(seq, d)
    return e, tab


@pytest.mark.parametrize("bad", ["short", "strided", "wide", "sin_only"])
def test_qk_norm_rope_fwd_checks_the_rope_tables(bad):
    """ops.qk_norm_rope_fwd: the kernel reads cos / sin as [row % seq][d] with a row pitch of d -- a table of fewer than seq rows or a strided view
    is refused (ValueError) before any pointer is handed over (CPU tensors: a call that got past the check would raise RuntimeError instead)"""
    from lxt_amd import ops
    rows, nq, nk, d, seq = 16, 4, 2, 64, 8
    e, tab = _site_operands(rows, nq, nk, d, seq)
    cos, sin = {"short": (tab[: seq - 1], tab[: seq - 1]), "strided": (torch.zeros(seq, 2 * d)[:, :d],) * 2, "wide": (torch.zeros(seq, 2 * d),) * 2,
                "sin_only": (tab, tab[: seq - 1])}[bad]
    args = (e((nq + 2 * nk) * d), torch.ones(d), torch.ones(d), e(nq * d), e(nk * d), torch.zeros(rows * nq), torch.zeros(rows * nk))
    with pytest.raises(ValueError, match="cos / sin"):
        ops.qk_norm_rope_fwd(*args, cos, sin, seq, nq, nk, d, 1e-6)
    with pytest.raises(RuntimeError, match="device tensors"):          # well-formed tables: the call goes on to the (absent) device
        ops.qk_norm_rope_fwd(*args, tab, tab, seq, nq, nk, d, 1e-6)


@pytest.mark.parametrize("bad", ["short", "strided", "wide", "sin_only"])
def test_qkv_bwd_pack_checks_the_rope_tables(bad):
    from lxt_amd import ops
    rows, nq, nk, d, seq = 16, 4, 2, 64, 8
    e, tab = _site_operands(rows, nq, nk, d, seq)
    cos, sin = {"short": (tab[: seq - 1], tab[: seq - 1]), "strided": (torch.zeros(seq, 2 * d)[:, :d],) * 2, "wide": (torch.zeros(seq, 2 * d),) * 2,
                "sin_only": (tab, tab[: seq - 1])}[bad]
    args = (e(nq * d), e(nq * d), e(nq * d), torch.ones(d), torch.ones(d), torch.zeros(rows * nq), torch.zeros(rows * nk))
    with pytest.raises(ValueError, match="cos / sin"):
        ops.qkv_bwd_pack(*args, cos, sin, e((nq + 2 * nk) * d), seq, nq, nk, d)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.qkv_bwd_pack(*args, tab, tab, e((nq + 2 * nk) * d), seq, nq, nk, d)


def test_gemm_nt_rs_rope_checks_the_rope_tables():
    """(the check the two site wrappers now share with the fused QKV GEMM's wrapper)"""
    from lxt_amd import ops
    x, W, out = torch.zeros(256, 64, dtype=BF), torch.zeros(256, 64, dtype=BF), torch.zeros(256, 256, dtype=BF)
    with pytest.raises(AssertionError):
        ops.gemm_nt_rs_rope(x, W, torch.zeros(256), torch.zeros(15, 128), torch.zeros(15, 128), out, 16, 128, 128)


def test_sandwich_norm_bwd_refuses_what_the_forward_gate_refuses():
    """ops.sandwich_norm_bwd takes contiguous [M, H] rows of a width lrp_sandwich_norm_ok accepts (the C ABI carries no row pitch): anything
    else is a ValueError before a pointer is handed over"""
    import lxt_amd._lib as L
    from lxt_amd import ops
    M = 4
    H_bad = next(h for h in (4, 100, 1 << 20) if not L.lib.lrp_sandwich_norm_ok(h, L.BF16))
    assert L.lib.lrp_sandwich_norm_ok(2560, L.BF16) == 1 and not ops.sandwich_norm_ok(torch.zeros(M, H_bad, dtype=BF))

    def call(Gx, Gres=None, Gs=None, Ga=None):
        H = Gx.shape[1]
        z = lambda: torch.zeros(M, H, dtype=BF)      # noqa: E731
        return ops.sandwich_norm_bwd(Gres, Gx, torch.ones(H), torch.ones(M), torch.ones(H), torch.ones(M), z() if Gs is None else Gs,
                                     z() if Ga is None else Ga, 1.0)

    with pytest.raises(ValueError, match="sandwich_norm_ok"):
        call(torch.zeros(M, H_bad, dtype=BF))
    wide = torch.zeros(M, 2 * 2560, dtype=BF)
    with pytest.raises(ValueError, match="sandwich_norm_ok"):
        call(wide[:, :2560])                                             # strided rows
    with pytest.raises(ValueError, match="sandwich_norm_ok"):
        call(torch.zeros(M, 2560, dtype=BF), Gres=wide[:, :2560])
    with pytest.raises(ValueError, match="sandwich_norm_ok"):
        call(torch.zeros(M, 2560, dtype=BF), Ga=torch.zeros(M + 1, 2560, dtype=BF))
    with pytest.raises(RuntimeError, match="device tensors"):          # an accepted call goes on to the (absent) device
        call(torch.zeros(M, 2560, dtype=BF))
    # the module switch of the site kernels is a dispatch policy, not part of this gate
    keep = ops.SITE_FUSION
    ops.SITE_FUSION = False
    try:
        with pytest.raises(RuntimeError, match="device tensors"):
            call(torch.zeros(M, 2560, dtype=BF))
    finally:
        ops.SITE_FUSION = keep
