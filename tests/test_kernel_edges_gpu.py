"""GPU parity of the HIP kernels AT THEIR DISPATCH EDGES (tests/test_kernels_gpu.py sits in the middle of each range): the fused QKV + RoPE GEMM
on odd head counts (a 256-column tile that holds the last k head and the first v head), the attention kernels at exact multiples of their
128-row query block / below one MFMA row block / at window = block size, on strided operands as the engines pass them, the q_begin argument
(top-layer sparsity) and the row intervals of the D-forming dQ kernel.  References: fp64 restatements of the same op; bars: those of
tests/test_kernels_gpu.py, plus per-block bars so that a wrong block of small values cannot hide behind the global maximum (the GEMM forms are
held element by element to a derived rounding bound in tests/test_gemm_bound_gpu.py; the edges here keep the odd head counts and the row chunks)."""
import pytest
import torch

from oracle import llama as ol
from tests.util import nmax
from tests.test_kernels_gpu import _attn_ref, _intervals, _tm, f64, rnd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import lxt_amd.ops as o
    return o


# ------------------------------------------------------------------------------------- A. RoPE GEMM, odd nq + nk
@pytest.mark.parametrize("M,N,K,seq,rope_cols", [(3072, 4352, 128, 192, 4224), (9728, 1280, 192, 2432, 1152)])
def test_gemm_nt_rs_rope_odd_head_count(ops, M, N, K, seq, rope_cols):
    """lrp_gemm_nt_rs_rope with an odd number of rotated heads at head_dim 128 (nq 32 / nk 1: 12 x 17 = 204 tiles, the mixed tile in the middle
    of the row of tiles; nq 8 / nk 1: the mixed tile is the last column tile): the 256-column tile that holds the last k head AND the first v
    head rotates the k head only.  Operands, reference and bars of test_gemm_nt_rs_rope, plus a bar per 128-column head (nmax is normalised by
    the global maximum)."""
    g_ = torch.Generator().manual_seed(M + N + seq)
    bf, d = torch.bfloat16, 128
    x = torch.randn(M, K, generator=g_).to(bf).cuda()
    W = (torch.randn(N, K, generator=g_) * K ** -0.5).to(bf).cuda()
    rs = (torch.rand(M, generator=g_) + 0.5).cuda()
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    fr = torch.arange(seq + 7, dtype=torch.float32)[:, None] * inv[None]
    emb = torch.cat((fr, fr), -1)
    cos, sin = emb.cos().to(bf).float().cuda().contiguous(), emb.sin().to(bf).float().cuda().contiguous()
    out = torch.full((M, N), float("nan"), dtype=bf, device="cuda")
    assert ops.gemm_nt_rs_rope_ok(x, W, out, seq, rope_cols, d)
    ops.gemm_nt_rs_rope(x, W, rs, cos, sin, out, seq, rope_cols, d)
    z = rs.double()[:, None] * (f64(x) @ f64(W).T)
    zr = z[:, :rope_cols].view(M, rope_cols // d, d)
    pos = torch.arange(M, device="cuda") % seq
    c, s_ = cos.double()[pos][:, None, :], sin.double()[pos][:, None, :]
    rot = torch.cat((-zr[..., d // 2:], zr[..., : d // 2]), -1)
    ref = torch.cat(((zr * c + rot * s_).view(M, rope_cols), z[:, rope_cols:]), 1)
    two = torch.empty(M, N, dtype=bf, device="cuda")
    ops.gemm_nt_rs(x, W, rs, two)
    two_r = ops.rope_fwd(two, torch.empty(M, rope_cols, dtype=bf, device="cuda"), cos, sin, seq, rope_cols // d, d)
    err = (out.double() - ref).abs()
    head_err = err.view(M, N // d, d).amax((0, 2)) / ref.abs().view(M, N // d, d).amax((0, 2))
    print(f"[rope_cols {rope_cols} of {N}] nmax {nmax(out, ref):.2e} | max abs err / max|ref| {float(err.max() / ref.abs().max()):.2e} | worst head "
          f"{int(head_err.argmax())} of {N // d}: {float(head_err.max()):.2e} | v columns differing from the un-rotated GEMM: "
          f"{int((out[:, rope_cols:] != two[:, rope_cols:]).sum())} | rotated part vs two launches {nmax(out[:, :rope_cols], two_r.double()):.2e}")
    assert not torch.isnan(out).any() and nmax(out, ref) < 1e-2
    assert err.max() <= ref.abs().max() * 2.0 ** -8                                              # ONE bf16 rounding of the fp32 result
    assert torch.equal(out[:, rope_cols:], two[:, rope_cols:])                                   # v: un-rotated, bit for bit
    assert nmax(out[:, :rope_cols], two_r.double()) < 1.5e-2
    assert float(head_err.max()) <= 4e-2, head_err                                               # every head: the 4 x block bar of the big-tile test


def test_llama_bf16_odd_head_count_fused_qkv():
    """LlamaLRP with n_heads 16, n_kv 1 at head_dim 128 (rope_cols 2176 of 2304: an odd number of rotated heads) at a row count that admits the
    fused flow (M = 6144: 24 x 9 QKV tiles, 24 x 8 H-wide ones): the bf16 engine with the RoPE-fused QKV GEMM, and with the two-launch form,
    against the fp32 engine, and against each other -- the bars of test_llama_bf16_norm_folded_into_gemms."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import lxt_amd.engine as E
    import lxt_amd.ops as ops
    cfg = dict(hidden=2048, inter=5632, n_layers=2, n_heads=16, n_kv=1, head_dim=128, vocab=1024, rope_theta=1e4, rms_eps=1e-5)
    W = ol.random_weights(cfg, seed=77)
    g = torch.Generator().manual_seed(78)
    for L in W["layers"]:
        L["ln1"] = (0.25 + 1.5 * torch.rand(cfg["hidden"], generator=g))
        L["ln2"] = (0.25 + 1.5 * torch.rand(cfg["hidden"], generator=g))
    B, S = 3, 2048
    ids = torch.randint(0, cfg["vocab"], (B, S), generator=g)
    ref = E.LlamaLRP(cfg, W, dtype=torch.float32, mode="efficient", max_seq=S).explain(ids)
    tgt = ref["idx"]
    eng = E.LlamaLRP(cfg, W, dtype=torch.bfloat16, mode="efficient", max_seq=S)
    assert eng._norm_fused(B * S)
    keep = ops.ROPE_FWD_FUSION
    try:
        ops.ROPE_FWD_FUSION = True
        fused = eng.explain(ids, target=tgt)
        ops.ROPE_FWD_FUSION = False
        plain = eng.explain(ids, target=tgt)
    finally:
        ops.ROPE_FWD_FUSION = keep
    e_f, e_p, d_fp = nmax(fused["R_tok"], ref["R_tok"]), nmax(plain["R_tok"], ref["R_tok"]), nmax(fused["R_tok"], plain["R_tok"])
    print(f"[nq 16, nk 1] vs the fp32 engine: RoPE-fused QKV GEMM {e_f:.2e}, two launches {e_p:.2e}; fused vs two launches {d_fp:.2e}")
    assert torch.isfinite(fused["R_tok"]).all() and torch.isfinite(plain["R_tok"]).all()
    assert e_f < 2e-2
    assert e_p < 2e-2
    assert d_fp < 1.5e-2


# ------------------------------------------------------------------------------- B / C. attention: shared pieces
def _cases(cases):
    """(case..., dtype) for every dtype that serves the case's head dim: fp32 has no d = 96 kernels, bf16 needs d >= 32 (one 64-byte MFMA K chunk)"""
    out = []
    for c in cases:
        d = c[4]
        if d != 96:
            out.append(c + (torch.float32,))
        if d >= 32:
            out.append(c + (torch.bfloat16,))
    return out


def _qkv_slices(B, S, Hq, Hkv, d, dtype):
    """q, k, v as the engines pass them: column slices of ONE fused [B S, (Hq + 2 Hkv) d + 64] buffer (row pitch != row width);
    -> the three 2-D views and their [B, H, S, d] forms"""
    buf = rnd(B * S, (Hq + 2 * Hkv) * d + 64, dtype=dtype, seed=1)
    q, k, v = buf[:, : Hq * d], buf[:, Hq * d: (Hq + Hkv) * d], buf[:, (Hq + Hkv) * d: (Hq + 2 * Hkv) * d]
    h4 = lambda x, H: x.reshape(B, S, H, d).permute(0, 2, 1, 3)      # noqa: E731
    return (q, k, v), (h4(q, Hq), h4(k, Hkv), h4(v, Hkv))


def _nan_buf(rows, cols, spare, dtype):
    """a [rows, cols] view into a NaN-filled [rows, cols + spare] buffer -> (view, the spare columns)"""
    buf = torch.full((rows, cols + spare), float("nan"), dtype=dtype, device="cuda")
    return buf[:, :cols], buf[:, cols:]


def _h4(x, B, S, H, d):
    return x.double().reshape(B, S, H, d).permute(0, 2, 1, 3)


def _ref_bwd(q, k, v, Gh, p, vis, scale):
    """fp64 backward of the efficient placement (every stabiliser 0): Ghs = dS3 scale / 2 -> (dQ [B,Hq,S,d], dK, dV [B,Hkv,S,d], dP)"""
    B, Hq, S, d = q.shape
    Hkv = k.shape[1]
    rep = Hq // Hkv
    kx, vx = k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1)
    dP = Gh @ vx.transpose(-1, -2)
    dS3 = p * (dP - (dP * p).sum(-1, keepdim=True))
    Ghs = torch.where(vis, dS3 * scale * 0.5, torch.zeros_like(dS3))
    dQ = Ghs @ kx
    dK = (Ghs.transpose(-1, -2) @ q).reshape(B, Hkv, rep, S, d).sum(2)
    dV = (p.transpose(-1, -2) @ Gh).reshape(B, Hkv, rep, S, d).sum(2)
    return dQ, dK, dV, dP


def _check(name, x, ref, bar, norm=None, rows=None):
    """x [B*S, H*d] (token-major) against ref [B, H, S, d] fp64: finite; normalised max error below bar; and below 4 x bar in EVERY (head, 128-row
    block) normalised by that block's own maximum (a wrong block of small values cannot hide behind the global maximum).  norm: the normaliser where
    the reference is identically zero (see test_attention_block_edges); rows: check query rows >= rows only"""
    B, H, S, d = ref.shape
    x4 = _h4(x, B, S, H, d)
    if rows:
        x4, ref = x4[:, :, rows:], ref[:, :, rows:]
    assert torch.isfinite(x4).all(), name
    err = (x4 - ref).abs().amax(-1)                                   # [B, H, S']
    top = float(ref.abs().max()) if norm is None else norm
    print(f"  {name}: max err / max|ref| = {float(err.max()) / max(top, 1e-300):.2e} (bar {bar:.0e})")
    assert float(err.max()) < bar * top, (name, float(err.max()), top)
    if norm is None:
        n = err.shape[-1]
        pad = (-(n if not rows else n + rows % 128)) % 128
        lead = rows % 128 if rows else 0                               # keep the 128-row grid of the FULL sequence
        grid = lambda t: torch.nn.functional.pad(t, (lead, pad)).reshape(B, H, -1, 128).amax(-1)      # noqa: E731
        eb, rb = grid(err), grid(ref.abs().amax(-1))
        worst = float((eb / rb.clamp_min(1e-300)).max())
        print(f"  {name}: worst (head, 128-row block) err / block max = {worst:.2e} (bar {4 * bar:.0e})")
        assert bool((eb <= 4 * bar * rb).all()), (name, worst)


def _attn_pipeline(ops, views, B, S, Hq, Hkv, d, dtype, causal, window, Go, q_begin=0, row_iv=None, fwd_from=None, t_pitch=None):
    """forward, prep, dQ, dK / dV (+ the D-forming dQ kernel where it serves the call) on strided operands with NaN-filled, over-wide outputs;
    fwd_from = (o, lse): the backward is fed these instead of this call's forward; t_pitch: row pitch of the head-transposed operands
    (default: ops.transpose_heads' own, S padded to 64)"""
    q, k, v = views
    scale = d ** -0.5
    R = {}

    def tr(x, H):
        out = None if t_pitch is None else torch.zeros(B, H, d, t_pitch, dtype=dtype, device="cuda")
        return ops.transpose_heads(x, B, S, H, d, out=out)

    v_t = tr(v, Hkv)
    R["o"], R["o_spare"] = _nan_buf(B * S, Hq * d, 64, dtype)
    R["lse"] = torch.full((B, Hq, S), float("nan"), device="cuda")
    ops.attn_fwd(q, k, v, v_t, R["o"], R["lse"], B, S, Hq, Hkv, d, scale, causal, window, q_begin=q_begin, row_iv=row_iv)
    if Go is None:
        return R
    o, lse = fwd_from if fwd_from is not None else (R["o"], R["lse"])
    R["Gho"], R["D"] = torch.full_like(Go, float("nan")), torch.full((B, Hq, S), float("nan"), device="cuda")
    ops.attn_bwd_prep(Go, o, R["Gho"], R["D"], B, S, Hq, d, 0.0, 0.5)
    k_t, q_t, Gho_t = tr(k, Hkv), tr(q, Hq), tr(R["Gho"], Hq)
    R["dq"], R["dq_spare"] = _nan_buf(B * S, Hq * d, 64, dtype)
    ops.attn_bwd_dq(q, k, v, k_t, R["Gho"], lse, R["D"], R["dq"], B, S, Hq, Hkv, d, scale, 0.0, 0.0, causal, window, q_begin=q_begin, row_iv=row_iv)
    R["dk_h"], R["dk_spare"] = _nan_buf(B * S, Hq * d, 8, dtype)
    R["dv_h"], R["dv_spare"] = _nan_buf(B * S, Hq * d, 8, dtype)
    ops.attn_bwd_dkv(q, k, v, q_t, R["Gho"], Gho_t, lse, R["D"], R["dk_h"], R["dv_h"], B, S, Hq, Hkv, d, scale, 0.0, 0.0, causal, window,
                     q_begin=q_begin, row_iv=row_iv)
    R["dk"], R["dv"] = torch.empty(B * S, Hkv * d, dtype=dtype, device="cuda"), torch.empty(B * S, Hkv * d, dtype=dtype, device="cuda")
    ops.gqa_reduce(R["dk_h"], R["dk"], B * S, Hkv, Hq // Hkv, d)
    ops.gqa_reduce(R["dv_h"], R["dv"], B * S, Hkv, Hq // Hkv, d)
    if q_begin == 0 and ops.attn_dq_d_ok(dtype, d):
        R["D2"] = torch.full((B, Hq, S), float("nan"), device="cuda")
        R["dq2"], R["dq2_spare"] = _nan_buf(B * S, Hq * d, 64, dtype)
        ops.attn_bwd_dq_d(q, k, v, R["Gho"], o, lse, R["D2"], R["dq2"], B, S, Hq, Hkv, d, scale, causal, window, row_iv=row_iv)
    return R


def _spares_untouched(R):
    for key in R:
        if key.endswith("_spare"):
            assert torch.isnan(R[key]).all(), f"{key}: the kernel wrote past its row width"


# ------------------------------------------------------------------------------------ B. attention at its block edges
EDGE_CASES = [
    (2, 128, 2, 1, 64, True, 0),         # exactly one 128-row query block
    (1, 256, 4, 2, 128, True, 0), (1, 256, 2, 1, 256, True, 0), (1, 384, 2, 2, 96, False, 0), (1, 256, 2, 1, 32, False, 0),      # exact multiples
    (1, 129, 2, 1, 128, True, 0),        # one row into the second block
    (2, 1, 2, 1, 64, True, 0), (1, 15, 4, 2, 128, True, 0), (1, 7, 2, 2, 32, False, 0),       # less than one MFMA row block
    (1, 256, 2, 1, 128, True, 1),        # every row sees itself only: p = 1, lse = s scale
    (1, 256, 2, 1, 64, True, 128),       # window = block size
    (1, 384, 2, 1, 256, True, 129),      # window one past the block size
    (1, 200, 2, 1, 128, True, 200), (1, 200, 2, 1, 64, True, 1000)]       # window >= S: no window


@pytest.mark.parametrize("B,S,Hq,Hkv,d,causal,window,dtype", _cases(EDGE_CASES))
def test_attention_block_edges(ops, B, S, Hq, Hkv, d, causal, window, dtype):
    """fwd o / lse, attn_bwd_prep, dQ, dK, dV (and the D-forming dQ kernel where it serves the call) where S is an exact multiple of the 128-row
    query block, one row past it, below one MFMA row block, and where the window meets the block size -- on column slices of one fused qkv
    buffer and into over-wide NaN-filled outputs (spare columns must stay NaN).  fp64 reference and bars of test_attention (efficient
    placement), plus a bar per (head, 128-row block).

    Where a row sees ONE key (S = 1, window = 1) p = 1 and dS3 = p (dP - D) = 0: the fp64 dQ and dK are exactly zero and nothing can be
    normalised by them.  What the kernel leaves there is the difference of two fp32 sums of the same products in different orders (dP from the
    MFMA, D from attn_bwd_prep), so those two are held to the same fraction (3 tol) of the un-cancelled term |p dP| scale / 2 times |k| / |q|."""
    tol = 3e-5 if dtype == torch.float32 else 3e-2
    lse_bar = 1e-5 if dtype == torch.float32 else 1e-2
    scale = d ** -0.5
    views, (q4, k4, v4) = _qkv_slices(B, S, Hq, Hkv, d, dtype)
    Go = rnd(B * S, Hq * d, dtype=dtype, seed=4)
    R = _attn_pipeline(ops, views, B, S, Hq, Hkv, d, dtype, causal, window, Go)
    s, p, o_ref, vis, rep = _attn_ref(f64(q4), f64(k4), f64(v4), scale, causal, window)
    lse_ref = torch.logsumexp((s * scale).masked_fill(~vis, float("-inf")), -1)
    print(f"[S {S} d {d} causal {causal} window {window} {dtype}]")
    _spares_untouched(R)
    _check("o", R["o"], o_ref, tol)
    assert torch.isfinite(R["lse"]).all() and nmax(R["lse"], lse_ref) < lse_bar
    if window == 1:
        assert nmax(R["lse"], (s * scale).diagonal(dim1=-2, dim2=-1)) < lse_bar
    Gh = _h4(R["Gho"], B, S, Hq, d)
    assert nmax(R["Gho"], _tm(0.5 * _h4(Go, B, S, Hq, d))) < tol
    assert torch.isfinite(R["D"]).all() and nmax(R["D"], (Gh * _h4(R["o"], B, S, Hq, d)).sum(-1)) < tol
    dQ, dK, dV, dP = _ref_bwd(f64(q4), f64(k4), f64(v4), Gh, p, vis, scale)
    one_key = S == 1 or window == 1
    nq_ = nk_ = None
    if one_key:
        assert float(dQ.abs().max()) == 0.0 and float(dK.abs().max()) == 0.0
        un = (p * dP).abs() * scale * 0.5
        nq_ = float((un @ f64(k4).repeat_interleave(rep, 1).abs()).max())
        nk_ = float((un.transpose(-1, -2) @ f64(q4).abs()).reshape(B, Hkv, rep, S, d).sum(2).max())
    _check("dq", R["dq"], dQ, 3 * tol, norm=nq_)
    _check("dk", R["dk"], dK, 3 * tol, norm=nk_)
    _check("dv", R["dv"], dV, 3 * tol)
    if "dq2" in R:
        D, D2 = R["D"], R["D2"]
        assert not torch.isnan(D2).any() and torch.allclose(D2, D, rtol=1e-4, atol=1e-5 * float(D.abs().max()))
        _check("dq (D-forming kernel)", R["dq2"], dQ, 3 * tol, norm=nq_)
        if not one_key:
            assert nmax(R["dq2"], R["dq"]) < 1e-2
    if window >= S:
        R0 = _attn_pipeline(ops, views, B, S, Hq, Hkv, d, dtype, causal, 0, Go)
        for key in ("o", "lse", "dq", "dk_h", "dv_h") + (("dq2", "D2") if "dq2" in R else ()):
            assert torch.equal(R[key], R0[key]), f"{key}: window >= S differs from no window"


@pytest.mark.parametrize("S,d,t_pitch,dtype", [(100, 64, 100, torch.float32), (100, 32, 104, torch.bfloat16)])
def test_attention_narrow_transposed_pitch(ops, S, d, t_pitch, dtype):
    """head-transposed operands whose pitch is S rounded up to 16 bytes only -- off the 128-byte column-tile grid, which include/lrp_hip.h
    allows: the 8-wave kernels read whole column tiles, so these calls run on the 4-wave kernels (ops.transpose_heads always pads to 64, which
    leaves them fp32 d = 256 alone from Python).  fwd o / lse, dQ, dK, dV against the fp64 reference with test_attention's bars."""
    B, Hq, Hkv, causal = 1, 4, 2, True
    size = torch.empty(0, dtype=dtype).element_size()
    assert t_pitch >= S and (t_pitch * size) % 16 == 0 and (t_pitch * size) % 128 != 0 and (t_pitch - S) * size < 16
    tol = 3e-5 if dtype == torch.float32 else 3e-2
    scale = d ** -0.5
    views, (q4, k4, v4) = _qkv_slices(B, S, Hq, Hkv, d, dtype)
    Go = rnd(B * S, Hq * d, dtype=dtype, seed=4)
    R = _attn_pipeline(ops, views, B, S, Hq, Hkv, d, dtype, causal, 0, Go, t_pitch=t_pitch)
    s, p, o_ref, vis, rep = _attn_ref(f64(q4), f64(k4), f64(v4), scale, causal, 0)
    lse_ref = torch.logsumexp((s * scale).masked_fill(~vis, float("-inf")), -1)
    print(f"[narrow transposed pitch {t_pitch}: S {S} d {d} {dtype}]")
    _spares_untouched(R)
    _check("o", R["o"], o_ref, tol)
    assert torch.isfinite(R["lse"]).all() and nmax(R["lse"], lse_ref) < (1e-5 if dtype == torch.float32 else 1e-2)
    dQ, dK, dV, _ = _ref_bwd(f64(q4), f64(k4), f64(v4), _h4(R["Gho"], B, S, Hq, d), p, vis, scale)
    _check("dq", R["dq"], dQ, 3 * tol)
    _check("dk", R["dk"], dK, 3 * tol)
    _check("dv", R["dv"], dV, 3 * tol)


# ------------------------------------------------------------------------------------------------- C. q_begin
QB_CASES = [(2, 300, 4, 2, 128, 0, 299, None), (2, 300, 4, 2, 64, 0, 128, None), (1, 300, 2, 1, 256, 0, 129, None), (1, 260, 2, 2, 32, 0, 1, None),
            (1, 300, 2, 1, 96, 0, 255, None), (1, 400, 2, 1, 128, 90, 399, None), (2, 256, 2, 1, 128, 0, 255, None), (2, 256, 2, 1, 128, 0, 255, "left_pad")]


@pytest.mark.parametrize("B,S,Hq,Hkv,d,window,q_begin,kind,dtype", _cases(QB_CASES))
def test_attention_q_begin(ops, B, S, Hq, Hkv, d, window, q_begin, kind, dtype):
    """q_begin (top-layer sparsity; include/lrp_hip.h: only query rows >= q_begin are needed / carry relevance, query blocks wholly below are
    skipped, rows below are unspecified in o / lse / dq) in all four kernel families, at q_begin = S - 1 (what the engines pass), on a block
    boundary, one past it, at 1, with a window and with left-padding intervals.  (1) forward rows >= q_begin vs fp64; (2) backward with q_begin
    of a seed that is zero below q_begin, fed a dense forward's o / lse: dq rows >= q_begin and dk, dv at ALL rows vs the fp64 dense backward,
    and dk, dv equal to the dense call's (the skipped blocks contributed zeros); (3) the same backward fed the sparse forward's own o / lse
    (unwritten rows NaN) with operands prepared as LlamaLRP / Gemma3LRP prepare them (engine.top_attn_operands: prep on the live rows,
    scattered into zeroed Gho / D; zeroed dq)."""
    tol = 3e-5 if dtype == torch.float32 else 3e-2
    lse_bar = 1e-5 if dtype == torch.float32 else 1e-2
    scale = d ** -0.5
    rep = Hq // Hkv
    views, (q4, k4, v4) = _qkv_slices(B, S, Hq, Hkv, d, dtype)
    q, k, v = views
    row_iv = None
    s, p, o_ref, vis, _ = _attn_ref(f64(q4), f64(k4), f64(v4), scale, True, window)
    if kind is not None:
        lo, hi, causal = _intervals(kind, B, S)
        assert causal
        row_iv = (lo.cuda().contiguous(), hi.cuda().contiguous())
        j = torch.arange(S, device="cuda")
        vis = vis[None, None] & ((j[None, None, :] >= row_iv[0][:, :, None]) & (j[None, None, :] < row_iv[1][:, :, None]))[:, None]
        p = torch.nan_to_num(torch.softmax((s * scale).masked_fill(~vis, float("-inf")), -1), nan=0.0)
        o_ref = p @ f64(v4).repeat_interleave(rep, 1)
        assert bool(vis[:, :, q_begin:].any(-1).all())                 # the checked rows see something
    lse_ref = torch.logsumexp((s * scale).masked_fill(~vis, float("-inf")), -1)
    print(f"[S {S} d {d} window {window} q_begin {q_begin} {kind} {dtype}]")
    # (1) the sparse forward
    Rs = _attn_pipeline(ops, views, B, S, Hq, Hkv, d, dtype, True, window, None, q_begin=q_begin, row_iv=row_iv)
    _spares_untouched(Rs)
    _check("o, rows >= q_begin", Rs["o"], o_ref, tol, rows=q_begin)
    assert torch.isfinite(Rs["lse"][:, :, q_begin:]).all() and nmax(Rs["lse"][:, :, q_begin:], lse_ref[:, :, q_begin:]) < lse_bar
    # (2) seed zero below q_begin; o / lse of a dense forward
    Go = rnd(B * S, Hq * d, dtype=dtype, seed=4)
    Go.view(B, S, Hq * d)[:, :q_begin] = 0
    R1 = _attn_pipeline(ops, views, B, S, Hq, Hkv, d, dtype, True, window, Go, row_iv=row_iv)               # dense: q_begin = 0
    fwd = (R1["o"], R1["lse"])
    Rq = _attn_pipeline(ops, views, B, S, Hq, Hkv, d, dtype, True, window, Go, q_begin=q_begin, row_iv=row_iv, fwd_from=fwd)
    _spares_untouched(Rq)
    Gh = _h4(Rq["Gho"], B, S, Hq, d)
    assert float(Gh[:, :, :q_begin].abs().max()) == 0.0 and float(Rq["D"][:, :, :q_begin].abs().max()) == 0.0
    dQ, dK, dV, _ = _ref_bwd(f64(q4), f64(k4), f64(v4), Gh, p, vis, scale)
    _check("dq, rows >= q_begin", Rq["dq"], dQ, 3 * tol, rows=q_begin)
    _check("dk", Rq["dk"], dK, 3 * tol)
    _check("dv", Rq["dv"], dV, 3 * tol)
    same_bar = 1e-6 if dtype == torch.float32 else 2.0 ** -8
    for key in ("dk", "dv"):
        gap = float((Rq[key].double() - R1[key].double()).abs().max()) / float(R1[key].double().abs().max())
        print(f"  {key}: q_begin call vs dense call {gap:.2e} (bar {same_bar:.1e})")
        assert gap <= same_bar, (key, gap)
    # (3) the sparse forward's own o / lse, operands as the engines prepare them
    n = S - q_begin
    live = lambda x: x.view(B, S, -1)[:, q_begin:].reshape(B * n, -1)      # noqa: E731
    Gho_l, D_l = torch.empty(B * n, Hq * d, dtype=dtype, device="cuda"), torch.empty(B, Hq, n, device="cuda")
    ops.attn_bwd_prep(live(Go).contiguous(), live(Rs["o"]).contiguous(), Gho_l, D_l, B, n, Hq, d, 0.0, 0.5)
    Gho = torch.zeros(B * S, Hq * d, dtype=dtype, device="cuda")
    Gho.view(B, S, Hq * d)[:, q_begin:] = Gho_l.view(B, n, Hq * d)
    D = torch.zeros(B, Hq, S, device="cuda")
    D[:, :, q_begin:] = D_l
    k_t, q_t, Gho_t = ops.transpose_heads(k, B, S, Hkv, d), ops.transpose_heads(q, B, S, Hq, d), ops.transpose_heads(Gho, B, S, Hq, d)
    dq = torch.zeros(B * S, Hq * d + 64, dtype=dtype, device="cuda")[:, : Hq * d]
    ops.attn_bwd_dq(q, k, v, k_t, Gho, Rs["lse"], D, dq, B, S, Hq, Hkv, d, scale, 0.0, 0.0, True, window, q_begin=q_begin, row_iv=row_iv)
    dk_h, _ = _nan_buf(B * S, Hq * d, 8, dtype)
    dv_h, _ = _nan_buf(B * S, Hq * d, 8, dtype)
    ops.attn_bwd_dkv(q, k, v, q_t, Gho, Gho_t, Rs["lse"], D, dk_h, dv_h, B, S, Hq, Hkv, d, scale, 0.0, 0.0, True, window, q_begin=q_begin, row_iv=row_iv)
    dk, dv = torch.empty(B * S, Hkv * d, dtype=dtype, device="cuda"), torch.empty(B * S, Hkv * d, dtype=dtype, device="cuda")
    ops.gqa_reduce(dk_h, dk, B * S, Hkv, rep, d)
    ops.gqa_reduce(dv_h, dv, B * S, Hkv, rep, d)
    dq_live, dq1_live = live(dq), live(Rq["dq"])
    assert torch.isfinite(dq_live.float()).all() and torch.isfinite(dk.float()).all() and torch.isfinite(dv.float()).all()
    e = (nmax(dq_live, dq1_live), nmax(dk, Rq["dk"]), nmax(dv, Rq["dv"]))
    print(f"  engine-style operands vs (2): dq {e[0]:.2e} dk {e[1]:.2e} dv {e[2]:.2e} (bar {3 * tol:.0e})")
    assert max(e) < 3 * tol


# ------------------------------------------------------------------- C. row intervals in the D-forming dQ kernel
def _rope_tables(S, d):
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    fr = torch.arange(S, dtype=torch.float32)[:, None] * inv[None, :]
    emb = torch.cat((fr, fr), -1)
    return emb.cos().cuda().contiguous(), emb.sin().cuda().contiguous()


def _rope_t64(G, cos, sin):
    """fp64 transpose of HF's rotation (the VJP of x cos + rotate_half(x) sin): G [B, H, S, d], tables [S, d]"""
    h = G.shape[-1] // 2
    Gs = G * sin.double()
    return G * cos.double() + torch.cat((Gs[..., h:], -Gs[..., :h]), -1)


@pytest.mark.parametrize("kind", ["left_pad", "right_pad", "packed"])
@pytest.mark.parametrize("B,S,Hq,Hkv,d", [(2, 200, 4, 2, 128), (2, 150, 4, 2, 64), (2, 210, 2, 1, 96), (2, 256, 2, 1, 128)])
def test_attn_bwd_dq_d_row_intervals(ops, kind, B, S, Hq, Hkv, d):
    """lrp_attn_bwd_dq_d with row_lo / row_hi (what LlamaLRP runs for every padded batch; test_attention_row_intervals calls attn_bwd_dq only):
    bf16, causal + the interval families of left / right padding and packed sequences, dq written into a column slice of a NaN-filled
    [B S, (Hq + 2 Hkv) d + 64] buffer, with and without RoPE's backward on the way out (d = 64 / 128).  Against the fp64 reference of
    test_attention_row_intervals, against attn_bwd_prep's D and attn_bwd_dq's dq; then attn_bwd_dkv fed THIS kernel's D."""
    dtype, tol = torch.bfloat16, 3e-2
    scale, rep = d ** -0.5, Hq // Hkv
    assert ops.attn_dq_d_ok(dtype, d)
    lo, hi, causal = _intervals(kind, B, S)
    assert causal
    row_iv = (lo.cuda().contiguous(), hi.cuda().contiguous())
    views, (q4, k4, v4) = _qkv_slices(B, S, Hq, Hkv, d, dtype)
    q, k, v = views
    o = torch.empty(B * S, Hq * d, dtype=dtype, device="cuda")
    lse = torch.empty(B, Hq, S, device="cuda")
    ops.attn_fwd(q, k, v, None, o, lse, B, S, Hq, Hkv, d, scale, True, 0, row_iv=row_iv)
    j = torch.arange(S, device="cuda")
    vis = ((j[None, None, :] >= row_iv[0][:, :, None]) & (j[None, None, :] < row_iv[1][:, :, None]) & (j[None, :] <= j[:, None])[None])[:, None]
    s = f64(q4) @ f64(k4).repeat_interleave(rep, 1).transpose(-1, -2)
    p = torch.nan_to_num(torch.softmax((s * scale).masked_fill(~vis, float("-inf")), -1), nan=0.0)
    Go = rnd(B * S, Hq * d, dtype=dtype, seed=4)
    Gho, D = torch.empty_like(Go), torch.empty(B, Hq, S, device="cuda")
    ops.attn_bwd_prep(Go, o, Gho, D, B, S, Hq, d, 0.0, 0.5)
    dQ, dK, dV, _ = _ref_bwd(f64(q4), f64(k4), f64(v4), _h4(Gho, B, S, Hq, d), p, vis, scale)
    empty = ~vis.any(-1).expand(B, Hq, S)                                # [B, Hq, S]
    assert bool(empty.any()) == (kind == "left_pad")
    width = (Hq + 2 * Hkv) * d + 64

    def run(rope):
        A = torch.full((B * S, width), float("nan"), dtype=dtype, device="cuda")
        D2 = torch.full((B, Hq, S), float("nan"), device="cuda")
        ops.attn_bwd_dq_d(q, k, v, Gho, o, lse, D2, A[:, : Hq * d], B, S, Hq, Hkv, d, scale, True, 0, row_iv=row_iv, rope=rope)
        assert torch.isnan(A[:, Hq * d:]).all() and torch.isfinite(A[:, : Hq * d].float()).all() and torch.isfinite(D2).all()
        assert torch.allclose(D2[~empty], D[~empty], rtol=1e-4, atol=1e-5 * float(D.abs().max()))
        assert bool((_h4(A[:, : Hq * d], B, S, Hq, d)[empty] == 0).all())
        return A[:, : Hq * d], D2

    dq2, D2 = run(None)
    print(f"[dq_d {kind} S {S} d {d}] dq vs fp64 {nmax(dq2, _tm(dQ)):.2e}")
    _check("dq", dq2, dQ, 3 * tol)
    dq1 = torch.empty(B * S, Hq * d, dtype=dtype, device="cuda")
    ops.attn_bwd_dq(q, k, v, None, Gho, lse, D, dq1, B, S, Hq, Hkv, d, scale, 0.0, 0.0, True, 0, row_iv=row_iv)
    assert nmax(dq2, dq1) < 1e-2
    dk_h, dv_h = torch.full_like(Go, float("nan")), torch.full_like(Go, float("nan"))
    ops.attn_bwd_dkv(q, k, v, None, Gho, None, lse, D2, dk_h, dv_h, B, S, Hq, Hkv, d, scale, 0.0, 0.0, True, 0, row_iv=row_iv)
    dk, dv = torch.empty(B * S, Hkv * d, dtype=dtype, device="cuda"), torch.empty(B * S, Hkv * d, dtype=dtype, device="cuda")
    ops.gqa_reduce(dv_h, dv, B * S, Hkv, rep, d)
    _check("dv", dv, dV, 3 * tol)
    if d in (64, 128):
        cs, sn = _rope_tables(S, d)
        dq3, _ = run((cs, sn))
        dq_rot = torch.empty_like(dq1)
        ops.rope_bwd(dq2, None, None, dq_rot, cs, sn, S, Hq, d, 0.0, 0.0)
        assert nmax(dq3, dq_rot) < 1e-2
        _check("dq, rotated back", dq3, _rope_t64(dQ, cs, sn), 3 * tol)
        ops.gqa_reduce_rope(dk_h, dk, B * S, S, Hkv, rep, d, cs, sn)
        _check("dk, rotated back", dk, _rope_t64(dK, cs, sn), 3 * tol)
    else:
        ops.gqa_reduce(dk_h, dk, B * S, Hkv, rep, d)
        _check("dk", dk, dK, 3 * tol)
