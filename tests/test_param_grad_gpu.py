"""GPU: the kernels behind the parameter gradients of a trainable model under the drop-in patches (DESIGN.md section 18,
include/lrp_hip_param_grad.h).
  lrp_wgrad          the plain weight.grad G^T X against fp64 on the rounded inputs, both dtypes, padded pitches, nothing written outside
                     [N, K]; exact on small-integer data; bf16 bit-equal to the ROUNDED lrp_wgrad_rel accumulator (the shared token loop);
  lrp_colsum_affine  norm-weight / bias column sums against fp64, every NULL combination of the wrapper, both load paths, bitwise repeatable;
  refusals           one case per documented code of both entries, returned before any launch (outputs keep their sentinel).
Bars are derived, not tuned: with mag = sum_t |terms|, an fp32 sum of M terms is within mag 2 M 2^-24 (one rounding per term and per add, a
factor 2 of margin); the bf16 output of lrp_wgrad adds its one rounding to nearest: 8 significand bits, at most 2^-8 |value| / (1 + 2^-8), so
the 2^-8 |ref| term is met by construction and with no spare factor (measured: 0.99 of the bar at M = 1, where the sum itself is exact)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
EINVAL, EALIGN, ESHAPE = -1, -2, -3
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from lxt_amd import ops
    return ops


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _padded(rows, cols, pad, dtype, gen):
    """a [rows, cols] view of [rows, cols + pad] storage"""
    return torch.randn(rows, cols + pad, generator=gen, device="cuda").to(dtype)[:, :cols]


# ---- lrp_wgrad ------------------------------------------------------------------------------------------------------------------------
WG_M = [1, 63, 64, 65, 130]
WG_NK = [(8, 8), (136, 72), (264, 200)]          # inside one tile; a ragged tile in both directions; three by two tiles (bf16: 128 x 128)


@pytest.mark.parametrize("M", WG_M)
@pytest.mark.parametrize("dtype,N,K", [(d, n, k) for d in (BF16, F32) for n, k in WG_NK] + [(F32, 5, 3)])
def test_wgrad_vs_fp64(ops, dtype, M, N, K):
    gen = _gen(1000 * M + N + K)
    v = 16 // dtype.itemsize
    G, X = _padded(M, N, 3 * v, dtype, gen), _padded(M, K, v, dtype, gen)
    store = torch.full((N + 2, K + 8), SENTINEL, device="cuda", dtype=dtype)
    out = ops.wgrad(G, X, out=store[:N, :K])
    ref = G.double().T @ X.double()
    mag = G.double().abs().T @ X.double().abs()
    bar = mag * 2 * M * 2.0 ** -24 + (2.0 ** -8 * ref.abs() if dtype == BF16 else 0.0)
    err = (out.double() - ref).abs()
    worst = float((err / bar.clamp_min(1e-300)).max())
    print(f"[wgrad {dtype} M={M} N={N} K={K}] max err / bar {worst:.3f}  normalised max {float(err.max() / ref.abs().max()):.2e}")
    assert out.dtype == dtype and out.data_ptr() == store.data_ptr()
    assert torch.isfinite(out).all() and bool((err <= bar).all()), worst
    assert bool((store[N:] == SENTINEL).all()) and bool((store[:, K:] == SENTINEL).all())       # rows and pitch padding outside [N, K]
    fresh = ops.wgrad(G, X)
    assert fresh.dtype == dtype and fresh.is_contiguous() and torch.equal(fresh, out) and torch.equal(fresh, ops.wgrad(G, X))


@pytest.mark.parametrize("M,N,K", [(1, 8, 8), (77, 136, 72), (200, 264, 200)])
def test_wgrad_bf16_exact_on_small_integers(ops, M, N, K):
    """entries from {-1, 0, 1}, M <= 200: every sum is an integer below 256 in magnitude, exact in the fp32 accumulator AND in bf16"""
    gen = _gen(7 * M + N)
    G = (torch.randint(-1, 2, (M, N + 8), generator=gen, device="cuda").to(BF16))[:, :N]
    X = (torch.randint(-1, 2, (M, K + 16), generator=gen, device="cuda").to(BF16))[:, :K]
    out = ops.wgrad(G, X)
    ref = G.double().T @ X.double()
    assert float(ref.abs().max()) <= 200
    assert torch.equal(out.double(), ref)


@pytest.mark.parametrize("M,N,K", [(1, 8, 8), (65, 136, 72), (130, 264, 200), (300, 128, 256)])
def test_wgrad_bf16_is_the_rounded_wgrad_rel_accumulator(ops, M, N, K):
    """W = 1 turns lrp_wgrad_rel's epilogue into a copy of its fp32 accumulator: the plain entry is that accumulator rounded once"""
    gen = _gen(31 * M + K)
    G, X = _padded(M, N, 8, BF16, gen), _padded(M, K, 24, BF16, gen)
    ones = torch.ones(N, K, device="cuda", dtype=BF16)
    assert torch.equal(ops.wgrad(G, X), ops.wgrad_rel(G, X, ones).to(BF16))


def test_wgrad_refusals(ops):
    from lxt_amd._lib import lib
    gen = _gen(0)
    G, X = _padded(16, 64, 0, BF16, gen), _padded(16, 64, 0, BF16, gen)
    assert ops.wgrad_ok(16, 64, 64, 64, 64, 64, BF16) and ops.wgrad_ok(1, 3, 5, 3, 5, 5, F32)
    assert lib.lrp_wgrad_ok(16, 64, 64, 64, 64, 64, 7) == EINVAL                         # an unknown dtype
    assert lib.lrp_wgrad_ok(16, 60, 64, 64, 64, 64, 1) == ESHAPE                         # bf16: N off the grid of 8
    assert lib.lrp_wgrad_ok(16, 64, 64, 56, 64, 64, 1) == ESHAPE                         # ldg < N
    assert lib.lrp_wgrad_ok(0, 64, 64, 64, 64, 64, 0) == ESHAPE
    assert lib.lrp_wgrad_ok(16, 64, 64, 68, 64, 64, 1) == EALIGN                         # bf16: a row pitch off the 16-byte grid
    assert lib.lrp_wgrad_ok(16, 64, 64, 64, 64, 66, 1) == EALIGN                         # bf16: ldo off the grid of 4
    out = torch.full((64, 72), SENTINEL, device="cuda", dtype=BF16)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.lrp_wgrad(G.data_ptr(), X.data_ptr(), out.data_ptr(), 16, 64, 64, 64, 64, 72, 7, st) == EINVAL
    with pytest.raises(RuntimeError, match="LRP_ESHAPE"):
        ops.wgrad(G[:, :60], X, out=out[:60, :64])
    with pytest.raises(RuntimeError, match="LRP_EALIGN"):
        ops.wgrad(_padded(16, 64, 4, BF16, gen), X, out=out[:, :64])
    with pytest.raises(RuntimeError, match="LRP_EALIGN"):
        ops.wgrad(G, X, out=torch.full((64, 66), SENTINEL, device="cuda", dtype=BF16)[:, :64])
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                                  # every refusal came before a launch
    with pytest.raises(TypeError):
        ops.wgrad(G, X.float())
    with pytest.raises(TypeError):
        ops.wgrad(G, X, out=torch.empty(64, 64, device="cuda"))
    with pytest.raises(ValueError):
        ops.wgrad(G, X[:8])
    with pytest.raises(ValueError):
        ops.wgrad(G, X, out=out[:32, :64])
    with pytest.raises(RuntimeError):
        ops.wgrad(G.cpu(), X.cpu())


# ---- lrp_colsum_affine ----------------------------------------------------------------------------------------------------------------
# (x, mean, rstd, want_bias): everything the wrapper can hand to the entry
NULLS = [(False, False, False, True)] + [(True, mu, rs, b) for mu in (False, True) for rs in (False, True) for b in (False, True)]


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("N", [1, 7, 8, 100])
@pytest.mark.parametrize("M", [1, 64, 65, 200])
def test_colsum_affine_vs_fp64(ops, dtype, M, N):
    v = 16 // dtype.itemsize
    for pad in (0, (-N) % v + v):             # rows as they come (N = 1, 7, 100 in bf16: one element per lane) and on the 16-byte grid (vector loads + tail)
        gen = _gen(10000 * M + 10 * N + pad)
        g, x = _padded(M, N, pad, dtype, gen), _padded(M, N, pad, dtype, gen)
        x += 0.5                                  # (in place: x keeps its pitch) a non-zero mean, so x - mean cancels
        mean = torch.randn(M, generator=gen, device="cuda") * 0.3
        rstd = torch.rand(M, generator=gen, device="cuda") + 0.5
        for has_x, has_mu, has_rs, bias in NULLS:
            args = (g, x if has_x else None, mean if has_mu else None, rstd if has_rs else None)
            dw, db = ops.colsum_affine(*args, want_bias=bias)
            assert (dw is not None) == has_x and (db is not None) == bias
            tag = f"[colsum_affine {dtype} M={M} N={N} pad={pad} x={has_x} mean={has_mu} rstd={has_rs} bias={bias}]"
            if has_x:
                terms = g.double() * (x.double() - (mean.double()[:, None] if has_mu else 0.0)) * (rstd.double()[:, None] if has_rs else 1.0)
                err, bar = (dw.double() - terms.sum(0)).abs(), terms.abs().sum(0) * 2 * M * 2.0 ** -24
                print(f"{tag} dw max err / bar {float((err / bar.clamp_min(1e-300)).max()):.3f}")
                assert dw.dtype == F32 and tuple(dw.shape) == (N,) and bool((err <= bar).all())
            if bias:
                err, bar = (db.double() - g.double().sum(0)).abs(), g.double().abs().sum(0) * 2 * M * 2.0 ** -24
                print(f"{tag} db max err / bar {float((err / bar.clamp_min(1e-300)).max()):.3f}")
                assert db.dtype == F32 and tuple(db.shape) == (N,) and bool((err <= bar).all())
            dw2, db2 = ops.colsum_affine(*args, want_bias=bias)                         # bitwise repeatable
            assert (dw is None or torch.equal(dw, dw2)) and (db is None or torch.equal(db, db2))


def test_colsum_affine_refusals(ops):
    from lxt_amd._lib import lib
    M, N = 130, 16
    g, x = torch.randn(M, N, device="cuda"), torch.randn(M, N, device="cuda")
    dw, db = (torch.full((N,), SENTINEL, device="cuda") for _ in range(2))
    need = lib.lrp_colsum_affine_ws(M, N)
    assert need > 0 and lib.lrp_colsum_affine_ws(64, N) == 0 and lib.lrp_colsum_affine_ws(0, N) == ESHAPE
    ws = torch.zeros(need + 16, device="cuda", dtype=torch.uint8)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda *a: lib.lrp_colsum_affine(*a, st)                                        # noqa: E731
    P = lambda t: None if t is None else t.data_ptr()                                      # noqa: E731
    assert call(P(g), P(x), None, None, None, None, P(ws), M, N, N, N, 0) == EINVAL        # neither dw nor db
    assert call(P(g), None, None, None, P(dw), None, P(ws), M, N, N, N, 0) == EINVAL       # dw without x
    assert call(P(g), P(x), None, None, P(dw), P(db), None, M, N, N, N, 0) == EINVAL       # M > 64 without a workspace
    assert call(P(g), P(x), None, None, P(dw), P(db), P(ws), M, N, N, N, 7) == EINVAL      # an unknown dtype
    assert call(P(g), P(x), None, None, P(dw), P(db), P(ws), M, N, N - 1, N, 0) == ESHAPE  # ldg < N
    assert call(P(g), P(x), None, None, P(dw), P(db), P(ws), M, N, N, N - 1, 0) == ESHAPE  # ldx < N
    assert call(P(g), P(x), None, None, P(dw), P(db), P(ws), 0, N, N, N, 0) == ESHAPE
    assert call(P(g), P(x), None, None, P(dw), P(db), ctypes.c_void_p(ws.data_ptr() + 1), M, N, N, N, 0) == EALIGN     # ws off 4 bytes
    torch.cuda.synchronize()
    assert bool((dw == SENTINEL).all()) and bool((db == SENTINEL).all())                   # every refusal came before a launch
    with pytest.raises(ValueError):
        ops.colsum_affine(g)                                                               # nothing to compute
    with pytest.raises(ValueError):
        ops.colsum_affine(g, x[:, :8])
    with pytest.raises(ValueError):
        ops.colsum_affine(g, None, torch.zeros(M, device="cuda"), want_bias=True)          # mean without x
    with pytest.raises(ValueError):
        ops.colsum_affine(g, x, torch.zeros(M - 1, device="cuda"))
    with pytest.raises(TypeError):
        ops.colsum_affine(g, x.to(BF16))
    with pytest.raises(TypeError):
        ops.colsum_affine(g, x, torch.zeros(M, device="cuda", dtype=BF16))
    with pytest.raises(ValueError):
        ops.colsum_affine(g, x, ws=torch.zeros(16, device="cuda", dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        ops.colsum_affine(g.cpu(), x.cpu())
