"""GPU: the weight-streaming Linear on MXFP4 codes (csrc/linear_stream_q.hip) and the decode step that uses it.
The kernel is held to BIT EQUALITY with the route it replaces -- ops.mxfp4_dequant into bf16, then ops.linear_stream_fwd on those bytes (the
plain kernel has its own fp64 tests: equality transfers them) -- in both forms (full K, K splits), at every MBMAX instantiation and partial row
block, both output types, with pitches, and at the format's corners.  The engine tests hold generate() of a quantised bf16 engine to the
outputs of the engine built from its dequantised weights, and count the dequant launches of the generation loop: none per token for a served
matrix."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def splits(M, N, K):
    import lxt_amd._lib as L
    return L.lib.lrp_linear_stream_fwd_splits(M, N, K)


def rand_q(N, K, seed, ldc=None, ldsc=None):
    """random codes / scales (E in 118 .. 131: |w| <= 96), in buffers of row pitch ldc / ldsc whose padding bytes are 0xFF"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    cb = torch.full((N, ldc or K // 2), 0xFF, device=DEV, dtype=torch.uint8)
    sb = torch.full((N, ldsc or K // 32), 0xFF, device=DEV, dtype=torch.uint8)
    codes, scales = cb[:, : K // 2], sb[:, : K // 32]
    codes.copy_(torch.randint(0, 256, (N, K // 2), generator=g, device=DEV, dtype=torch.uint8))
    scales.copy_(torch.randint(118, 132, (N, K // 32), generator=g, device=DEV, dtype=torch.uint8))
    return codes, scales


def rand_x(M, K, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(M, K, generator=g, device=DEV) * scale).bfloat16()


def control(x, codes, scales, bias=None, out_dtype=None, ldw=None):
    """the route the kernel replaces: dequantise into a bf16 matrix (row pitch ldw), then the plain stream kernel"""
    from lxt_amd import ops
    N, K = codes.shape[0], x.shape[1]
    D = torch.empty(N, ldw or K, device=DEV, dtype=BF16)[:, :K]
    ops.mxfp4_dequant(codes, scales, D)
    assert ops.linear_stream_ok(x, D)
    z = ops.linear_stream_fwd(x, D, bias, out_dtype=out_dtype)
    assert bool(torch.isfinite(z).all())
    return z


# (N, K, K splits, ((M, out dtype, bias), ...)): the M values cover every MBMAX instantiation (<= 32, <= 64, <= 128 rows) and the partial
# 16-row blocks in both forms
FULL = [(12288, 512, 1, ((1, BF16, False), (17, F32, True))),          # 8 K tiles: two groups, everything out of the prologue; rw = 12
        (16384, 1024, 1, ((16, F32, False), (128, BF16, True))),       # rw = 16, 16 K tiles
        (14336, 512, 1, ((15, BF16, True), (65, F32, False))),         # rw = 14
        (12300, 512, 1, ((33, F32, True), (64, BF16, False)))]         # rw = 13: 236 whole 52-row blocks and a ragged one
SPLIT = [(4096, 1536, 3, ((1, F32, True), (33, BF16, False))),
         (6144, 4096, 2, ((16, BF16, True), (65, F32, False))),
         (4096, 4096, 4, ((17, BF16, False), (128, F32, True))),
         (1536, 4096, 8, ((15, F32, False), (64, BF16, True)))]


@pytest.mark.parametrize("N,K,sp,rows", FULL + SPLIT, ids=lambda v: str(v) if isinstance(v, int) else "")
def test_equals_dequant_then_plain_stream_kernel_bit_for_bit(N, K, sp, rows):
    from lxt_amd import ops
    codes, scales = rand_q(N, K, seed=N + K)
    bias = rand_x(1, N, seed=5)[0]
    for M, odt, with_bias in rows:
        assert splits(M, N, K) == sp, "the split policy moved: this case no longer tests the form it names"
        x = rand_x(M, K, seed=M)
        assert ops.linear_stream_q_ok(x, codes, scales)
        b = bias if with_bias else None
        want = control(x, codes, scales, b, odt)
        got = ops.linear_stream_fwd_q(x, codes, scales, b, out_dtype=odt)
        assert got.dtype == odt and torch.equal(got, want), (M, odt, with_bias)
        if not with_bias:          # bias = 0 gives the bias-free bits
            assert torch.equal(ops.linear_stream_fwd_q(x, codes, scales, torch.zeros_like(bias), out_dtype=odt), want), (M, "zero bias")


@pytest.mark.parametrize("N,K,sp,M", [(12300, 512, 1, 19), (4096, 4096, 4, 35)], ids=["full-ragged", "split"])
@pytest.mark.parametrize("odt", [BF16, F32], ids=["bf16", "fp32"])
def test_pitches_padding_and_untouched_memory(N, K, sp, M, odt):
    """codes / scales with pitches beyond the row (padding 0xFF: E = 255 and the code of -6 if it were read), x with a pitch (NaN in the padding,
    NaN rows after row M), z inside a larger sentinel-filled buffer; the tickets are re-armed; a second call on them gives the same bits"""
    from lxt_amd import ops
    assert splits(M, N, K) == sp
    codes, scales = rand_q(N, K, seed=7, ldc=K // 2 + 32, ldsc=K // 32 + 8)
    xb = torch.full((M + 3, K + 16), float("nan"), device=DEV, dtype=BF16)
    x = xb[:M, :K]
    x.copy_(rand_x(M, K, seed=11))
    bias = rand_x(1, N, seed=5)[0]
    want = control(x, codes, scales, bias, odt, ldw=K + 24)
    zb = torch.full((M + 2, N + 8), 7.0, device=DEV, dtype=odt)
    z = zb[:M, :N]
    assert ops.linear_stream_q_ok(x, codes, scales)
    ops.linear_stream_fwd_q(x, codes, scales, bias, out=z)
    assert torch.equal(z, want)
    assert bool((zb[M:] == 7.0).all()) and bool((zb[:, N:] == 7.0).all()), "stored outside [M, N]"
    if sp > 1:
        assert not bool(ops.tickets(N // 64, x).any()), "tickets not re-armed"
    z.fill_(7.0)
    ops.linear_stream_fwd_q(x, codes, scales, bias, out=z)
    assert torch.equal(z, want), "second call on the same tickets"


@pytest.mark.parametrize("N,K,sp", [(12288, 512, 1), (4096, 1536, 3)], ids=["full", "split"])
def test_format_corners_equal_the_dequant_route(N, K, sp):
    """hand-made bytes: every code in both nibbles (the 256 byte values in turn: -0 = 0x8 included), E in {0, 1, 2, 127, 252} alternating from
    block to block along every row (subnormal results at E < 2, the largest finite ones at 252), and all-zero blocks"""
    from lxt_amd import ops
    M = 20
    assert splits(M, N, K) == sp
    r, c = torch.arange(N, device=DEV)[:, None], torch.arange(K // 2, device=DEV)[None]
    codes = ((r * 7 + c * 3) % 256).to(torch.uint8)
    assert len(set(codes[0].tolist())) == 256
    codes[5, 48:64] = 0                                # an all-zero block (block 3 of row 5), and one of -0 only
    codes[6, 16:32] = 0x88
    E = torch.tensor([0, 1, 2, 127, 252], device=DEV, dtype=torch.uint8)
    scales = E[(r + torch.arange(K // 32, device=DEV)[None]) % 5].contiguous()
    assert codes.is_contiguous() and set(scales[0].tolist()) == {0, 1, 2, 127, 252}
    # |w| <= 6 * 2^125 in a fifth of the blocks: |x| ~ 2^-12 keeps every fp32 sum far inside the range (the controls are checked finite)
    x = rand_x(M, K, seed=3, scale=2.0 ** -12)
    for odt in (BF16, F32):
        want = control(x, codes, scales, None, odt)
        assert bool((want != 0).any())
        assert torch.equal(ops.linear_stream_fwd_q(x, codes, scales, out_dtype=odt), want), odt
    # with moderate scales only (E = 127 +- 2), the same codes at full-size activations
    scales2 = (125 + (r + torch.arange(K // 32, device=DEV)[None]) % 5).to(torch.uint8).contiguous()
    x2 = rand_x(M, K, seed=4)
    assert torch.equal(ops.linear_stream_fwd_q(x2, codes, scales2, out_dtype=F32), control(x2, codes, scales2, None, F32))


def test_refusals_launch_nothing():
    from lxt_amd import ops
    N, K = 6144, 4096
    codes, scales = rand_q(N, K, seed=1)
    out = torch.full((4, N), 7.0, device=DEV, dtype=BF16)
    x = rand_x(4, K, seed=2)
    assert ops.linear_stream_q_ok(x, codes, scales)
    # fp32 activations
    assert not ops.linear_stream_q_ok(x.float(), codes, scales)
    with pytest.raises(RuntimeError, match="lrp_linear_stream_fwd_q"):
        ops.linear_stream_fwd_q(x.float(), codes, scales, out=out.float())
    # K = 768 (not a multiple of 512), M = 129
    c768, s768 = rand_q(N, 768, seed=1)
    assert not ops.linear_stream_q_ok(rand_x(4, 768, 2), c768, s768)
    with pytest.raises(RuntimeError, match="lrp_linear_stream_fwd_q"):
        ops.linear_stream_fwd_q(rand_x(4, 768, 2), c768, s768, out=out)
    x129, out129 = rand_x(129, K, 2), torch.full((129, N), 7.0, device=DEV, dtype=BF16)
    assert not ops.linear_stream_q_ok(x129, codes, scales)
    with pytest.raises(RuntimeError, match="lrp_linear_stream_fwd_q"):
        ops.linear_stream_fwd_q(x129, codes, scales, out=out129)
    # a codes view off the 16-byte grid
    buf = torch.zeros(N * (K // 2) + 16, device=DEV, dtype=torch.uint8)
    off = buf[8: 8 + N * (K // 2)].view(N, K // 2)
    assert off.data_ptr() % 16 == 8 and not ops.linear_stream_q_ok(x, off, scales)
    with pytest.raises(RuntimeError, match="lrp_linear_stream_fwd_q"):
        ops.linear_stream_fwd_q(x, off, scales, out=out)
    # a weight the wrong shape for x is a ValueError of the wrapper
    with pytest.raises(ValueError):
        ops.linear_stream_fwd_q(x, codes[:, :1024], scales, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((out129 == 7.0).all())


# ---- the engine ------------------------------------------------------------------------------------------------------------------------------
KEYS = ("sequences", "new_tokens", "n_new", "logit", "logprob", "logits", "lengths")
LENS = (40, 21, 9)


def cfg_w(inter, bias=False, seed=3):
    """2 layers at the Llama-3-8B attention widths (H 4096, 32 / 8 heads of 128, V 4096) with an MLP of `inter`"""
    H, d, V = 4096, 128, 4096
    cfg = dict(hidden=H, inter=inter, n_layers=2, n_heads=32, n_kv=8, head_dim=d, vocab=V, rope_theta=5e5, rms_eps=1e-5)
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: (torch.randn(*s, generator=g, device=DEV) * 0.02).bfloat16()              # noqa: E731
    nw = lambda: (1.0 + 0.1 * torch.randn(H, generator=g, device=DEV)).bfloat16()            # noqa: E731
    layers = []
    for _ in range(2):
        L = dict(ln1=nw(), ln2=nw(), wq=rn(32 * d, H), wk=rn(8 * d, H), wv=rn(8 * d, H), wo=rn(H, 32 * d), wg=rn(inter, H), wu=rn(inter, H),
                 wd=rn(H, inter))
        if bias:
            L.update(bq=rn(32 * d), bk=rn(8 * d), bv=rn(8 * d))
        layers.append(L)
    if bias:
        cfg.update(qkv_bias=True, qk_norm=False, tied=False)
    return cfg, dict(embed=rn(V, H), norm=nw(), lm_head=rn(V, H), layers=layers)


def ids340():
    return torch.randint(0, 4096, (3, 40), generator=torch.Generator().manual_seed(9))


def count_dequants(monkeypatch, fn):
    """-> (fn's result, number of ops.mxfp4_dequant calls it made)"""
    from lxt_amd import ops
    n, real = [0], ops.mxfp4_dequant

    def counted(*a, **kw):
        n[0] += 1
        return real(*a, **kw)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "mxfp4_dequant", counted)
        out = fn()
    return out, n[0]


def q_ok_set(eng, B):
    """which of the four layer matrices ops.linear_stream_q_ok serves at B rows, from the engine's own codes and fresh operands of the step's shapes"""
    from lxt_amd import ops
    c, Q = eng.cfg, eng._qlayers[0]
    K = dict(wqkv=c["hidden"], wo=c["n_heads"] * c["head_dim"], wgu=c["hidden"], wd=c["inter"])
    return {k for k in K if ops.linear_stream_q_ok(torch.zeros(B, K[k], device=DEV, dtype=eng.dtype), Q[k + "_c"], Q[k + "_s"])}


def same(a, b, what):
    for k in KEYS:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("model", ["llama", "qwen-bias"])
def test_generate_equals_the_dequantised_engine_and_dequantises_nothing_per_token(model, monkeypatch):
    from lxt_amd.engine import LlamaLRP
    from lxt_amd.engine_qwen import QwenLRP
    cls, (cfg, W) = (LlamaLRP, cfg_w(3072)) if model == "llama" else (QwenLRP, cfg_w(3072, bias=True))
    q = cls(cfg, W, weight_format="mxfp4", dtype=BF16, device=DEV, max_seq=64)
    del W
    assert q_ok_set(q, 3) == {"wqkv", "wo", "wgu", "wd"} and q._decode_served(3) == {"wqkv", "wo", "wgu", "wd"}
    ids = ids340()
    gen = lambda T, **kw: q.generate(ids, T, lengths=LENS, return_logits=True, **kw)      # noqa: E731
    eager, n8 = count_dequants(monkeypatch, lambda: gen(8))
    _, n1 = count_dequants(monkeypatch, lambda: gen(1))
    assert n1 == 4 * 2, n1          # the prefill: every matrix of every layer once
    assert n8 == n1, f"{n8 - n1} dequantisations in 7 decode steps (served matrices are read as codes)"
    cap = gen(8, graph=True)
    rep = gen(8, graph=True)
    plain = cls(*q.dequantized_weights(), dtype=BF16, device=DEV, max_seq=64)
    want = plain.generate(ids, 8, lengths=LENS, return_logits=True)
    assert bool(torch.isfinite(want["logits"]).all())
    same(eager, want, "eager")
    same(cap, want, "graph capture")
    same(rep, want, "graph replay")
    same(plain.generate(ids, 8, lengths=LENS, return_logits=True, graph=True), want, "plain graph")


def test_mixed_service_dequantises_only_what_is_not_served(monkeypatch):
    """I = 1024: the down projection [4096, 1024] is 64 workgroups x 2 possible splits -- not a stream problem -- while the other three are"""
    from lxt_amd.engine import LlamaLRP
    cfg, W = cfg_w(1024)
    q = LlamaLRP(cfg, W, weight_format="mxfp4", dtype=BF16, device=DEV, max_seq=64)
    del W
    assert {"wqkv", "wo", "wgu", "wd"} - q_ok_set(q, 3) == {"wd"}
    ids = ids340()
    gen = lambda T, **kw: q.generate(ids, T, lengths=LENS, return_logits=True, **kw)      # noqa: E731
    eager, n8 = count_dequants(monkeypatch, lambda: gen(8))
    _, n1 = count_dequants(monkeypatch, lambda: gen(1))
    assert n8 - n1 == 7 * 2 * 1, (n8, n1)
    plain = LlamaLRP(*q.dequantized_weights(), dtype=BF16, device=DEV, max_seq=64)
    want = plain.generate(ids, 8, lengths=LENS, return_logits=True)
    same(eager, want, "eager")
    same(gen(8, graph=True), want, "graph")


def raising(*a, **kw):
    raise AssertionError("ops.linear_stream_fwd_q must not be called here")


def test_nothing_served_on_a_tiny_model(monkeypatch):
    from lxt_amd import ops
    from lxt_amd.engine import LlamaLRP
    from tests.util import llama_case
    cfg, W, _, _ = llama_case("d128")                 # H 512, I 1024: no matrix fills the chip
    q = LlamaLRP(cfg, W, weight_format="mxfp4", dtype=BF16, device=DEV, max_seq=128)
    assert q_ok_set(q, 3) == set() and q._decode_served(3) == frozenset()
    monkeypatch.setattr(ops, "linear_stream_fwd_q", raising)
    ids = torch.randint(0, cfg["vocab"], (3, 40), generator=torch.Generator().manual_seed(9))
    _, n = count_dequants(monkeypatch, lambda: q.generate(ids, 4, lengths=LENS))
    assert n == 4 * len(q.layers) * 4          # today's behaviour: prefill + 3 steps, every matrix each time


def test_unquantised_and_fp32_engines_never_call_the_kernel(monkeypatch):
    from lxt_amd import ops
    from lxt_amd.engine import LlamaLRP
    monkeypatch.setattr(ops, "linear_stream_fwd_q", raising)
    cfg, W = cfg_w(1024)
    ids = ids340()
    bf = LlamaLRP(cfg, W, dtype=BF16, device=DEV, max_seq=64)
    assert bf._decode_served(3) == frozenset()
    assert bf.generate(ids, 3, lengths=LENS)["new_tokens"].shape == (3, 3)
    del bf
    f32 = LlamaLRP(cfg, W, weight_format="mxfp4", dtype=F32, device=DEV, max_seq=64)
    assert f32._decode_served(3) == frozenset()
    out, n = count_dequants(monkeypatch, lambda: f32.generate(ids, 3, lengths=LENS))
    assert out["new_tokens"].shape == (3, 3) and n == 3 * 2 * 4
