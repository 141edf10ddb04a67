"""GPU: the bias epilogues of the fused QKV forward (lrp_gemm_nt_rs_bias, lrp_gemm_nt_rs_bias_rope) against an fp64 restatement."""
import pytest
import torch

from tests.util import nmax

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import lxt_amd.ops as o
    return o


def f64(x):
    return x.double()


def _operands(M, N, K, seq, d=128):
    g_ = torch.Generator().manual_seed(M + N + K + seq)
    bf = torch.bfloat16
    x = torch.randn(M, K, generator=g_).to(bf).cuda()
    W = (torch.randn(N, K, generator=g_) * K ** -0.5).to(bf).cuda()
    rs = (torch.rand(M, generator=g_) + 0.5).cuda()
    bias = torch.randn(N, generator=g_).to(bf).cuda()
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    fr = torch.arange(seq + 7, dtype=torch.float32)[:, None] * inv[None]
    emb = torch.cat((fr, fr), -1)
    return x, W, rs, bias, emb.cos().to(bf).float().cuda().contiguous(), emb.sin().to(bf).float().cuda().contiguous()


def _rope64(z, cos, sin, seq, rope_cols, d=128):
    M = z.shape[0]
    zr = z[:, :rope_cols].view(M, rope_cols // d, d)
    pos = torch.arange(M, device=z.device) % seq
    c, s_ = cos.double()[pos][:, None, :], sin.double()[pos][:, None, :]
    rot = torch.cat((-zr[..., d // 2:], zr[..., : d // 2]), -1)
    return torch.cat(((zr * c + rot * s_).view(M, rope_cols), z[:, rope_cols:]), 1)


# (M, N, K, seq, rope_cols): M, N multiples of 256; the Llama-3-8B / Qwen2.5-7B class QKV at S = 2048; prompts that end inside a tile (seq 192)
SHAPES = [(2048, 6144, 256, 512, 5120), (2304, 5632, 192, 192, 4608), (8192, 6144, 4096, 2048, 5120), (24576, 1024, 512, 1024, 768)]


@pytest.mark.parametrize("M,N,K,seq,rope_cols", SHAPES)
def test_gemm_nt_rs_bias_and_bias_rope(ops, M, N, K, seq, rope_cols):
    """out = bf16(rs (x W^T) + bias) and the same with HF's RoPE on the columns [0, rope_cols): the bias is added in fp32 ahead of the rotation,
    one rounding at the store.  Bars: those of test_gemm_norm_fused_epilogues / test_gemm_nt_rs_rope for a bf16 output (the same accumulation
    with one more fp32 add): nmax < 1e-2 and one bf16 rounding of the fp32 result.  With bias = 0: bit-identical to the un-biased entries."""
    bf, d = torch.bfloat16, 128
    x, W, rs, bias, cos, sin = _operands(M, N, K, seq)
    z = rs.double()[:, None] * (f64(x) @ f64(W).T) + f64(bias)[None]
    out = torch.full((M, N), float("nan"), dtype=bf, device="cuda")
    ops.gemm_nt_rs_bias(x, W, rs, bias, out)
    e = nmax(out, z)
    print(f"[gemm_nt_rs_bias {M}x{N}x{K}] nmax vs fp64 {e:.2e}")
    assert not torch.isnan(out).any() and e < 1e-2
    assert (out.double() - z).abs().max() <= z.abs().max() * 2.0 ** -8
    assert ops.gemm_nt_rs_bias_rope_ok(x, W, out, seq, rope_cols, d)
    assert not ops.gemm_nt_rs_bias_rope_ok(x, W, out, seq, rope_cols, 64) and not ops.gemm_nt_rs_bias_rope_ok(x, W, out, seq + 8, rope_cols, d)
    outr = torch.full((M, N), float("nan"), dtype=bf, device="cuda")
    ops.gemm_nt_rs_bias_rope(x, W, rs, bias, cos, sin, outr, seq, rope_cols, d)
    ref = _rope64(z, cos, sin, seq, rope_cols)
    e = nmax(outr, ref)
    print(f"[gemm_nt_rs_bias_rope {M}x{N}x{K}] nmax vs fp64 {e:.2e}")
    assert not torch.isnan(outr).any() and e < 1e-2
    assert (outr.double() - ref).abs().max() <= ref.abs().max() * 2.0 ** -8
    assert torch.equal(outr[:, rope_cols:], out[:, rope_cols:])                      # v: bias, no rotation
    # bias = 0: the same bits as the un-biased entry points
    zero = torch.zeros_like(bias)
    a, b = torch.empty_like(out), torch.empty_like(out)
    ops.gemm_nt_rs_bias_rope(x, W, rs, zero, cos, sin, a, seq, rope_cols, d)
    ops.gemm_nt_rs_rope(x, W, rs, cos, sin, b, seq, rope_cols, d)
    assert torch.equal(a, b)
    ops.gemm_nt_rs_bias(x, W, rs, zero, a)
    ops.gemm_nt_rs(x, W, rs, b)
    assert torch.equal(a, b)


def test_gemm_nt_rs_bias_rope_refuses_an_odd_head_count(ops):
    """nq + nk odd at d = 128 (rope_cols % 256 == 128): the 256-column tile that holds the last k head holds the first v head, and the kernel
    rotates whole tiles -- the predicate says no and the entry point returns LRP_ESHAPE without launching (out keeps its NaN fill); the
    two-launch form the caller falls back to is right"""
    import lxt_amd._lib as L
    bf, d = torch.bfloat16, 128
    M, N, K, seq, rope_cols = 8192, 4352, 256, 2048, 4224          # nq 32, nk 1
    x, W, rs, bias, cos, sin = _operands(M, N, K, seq)
    out = torch.full((M, N), float("nan"), dtype=bf, device="cuda")
    assert not ops.gemm_nt_rs_bias_rope_ok(x, W, out, seq, rope_cols, d)
    p = lambda t: t.data_ptr()                                      # noqa: E731
    rc = L.lib.lrp_gemm_nt_rs_bias_rope(p(x), p(W), p(rs), p(bias), p(cos), p(sin), p(out), M, N, K, x.stride(0), W.stride(0), out.stride(0), seq,
                                        rope_cols, d, 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == L.lib.lrp_gemm_nt_rs(p(x), p(W), p(rs), p(out), 512, 512, K, K, K, 512, 1, None) and rc < 0      # LRP_ESHAPE, as a 4-tile problem gets
    assert torch.isnan(out).all()
    with pytest.raises(Exception):
        ops.gemm_nt_rs_bias_rope(x, W, rs, bias, cos, sin, out, seq, rope_cols, d)
    ops.gemm_nt_rs_bias(x, W, rs, bias, out)
    qkr = ops.rope_fwd(out, torch.empty(M, rope_cols, dtype=bf, device="cuda"), cos, sin, seq, rope_cols // d, d)
    z = rs.double()[:, None] * (f64(x) @ f64(W).T) + f64(bias)[None]
    assert nmax(qkr, _rope64(z, cos, sin, seq, rope_cols)[:, :rope_cols]) < 1.5e-2
