"""GPU: MXFP4 weight storage.  The two kernels against the torch restatement of the format (tests/test_mxfp4_cpu.py) bit for bit; the quantised
engine against an ordinary engine built from its own dequantised weights, bit for bit (bf16, the fused and the per-kernel layer, the sparse
top layer, ragged batches, the latent read-outs, Qwen2 / Qwen3, graph replay); the fp32 engine against the real reference run on the
dequantised weights (tests/golden/mxfp4_llama.npz); the byte accounting; and that the default engine is untouched."""
import gc

import numpy as np
import pytest
import torch

from tests.test_mxfp4_cpu import TIES, mx_dequant, mx_quantize
from tests.util import llama_case, load, nmax, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32


# ---- the kernels -----------------------------------------------------------------------------------------------------------------------------
def _edge_blocks(dtype):
    """[5, 32] in dtype: every listed tie (both signs) under a 6 X element; an all-zero block; a block with -0.0; an amax that is exactly a
    power of two; an amax one bf16 ulp below a power of two (saturates to 6)"""
    e = torch.zeros(5, 32, dtype=torch.float64)
    X = 2.0 ** -3
    e[0, 0] = 6 * X
    for i, (v, _) in enumerate(TIES):
        e[0, 1 + i], e[0, 9 + i] = v * X, -v * X
    e[0, 16:24] = torch.tensor([0.26, -0.74, 1.26, -1.74, 2.51, -3.49, 5.01, -7.9]) * X
    e[2] = torch.linspace(-1, 1, 32) * 2.0 ** 5
    e[2, 4] = -0.0
    e[3] = torch.linspace(-0.9, 0.9, 32) * 2.0 ** 9
    e[3, 30] = -(2.0 ** 9)
    e[4] = torch.linspace(-0.9, 0.9, 32) * 2.0 ** -6
    e[4, 2] = 2.0 ** -6 * (1 - 2.0 ** -8)
    out = e.to(BF16).to(dtype)          # (every edge value is a bf16 number: the same blocks in both types)
    assert bool(torch.signbit(out[2, 4])) and float(out[3].abs().max()) == 2.0 ** 9 and float(out[4].abs().max()) == 2.0 ** -6 * (1 - 2.0 ** -8)
    return out


def _matrix(rows, cols, dtype, seed):
    """seeded normal, scaled per block by 2^k, k in -30 ... 30, the edge blocks spliced into the first blocks (as many as the shape holds)"""
    g = torch.Generator().manual_seed(seed)
    nb = cols // 32
    w = torch.randn(rows, nb, 32, generator=g) * torch.exp2(torch.randint(-30, 31, (rows, nb, 1), generator=g).float())
    w = w.to(dtype).reshape(rows * nb, 32)
    edge = _edge_blocks(dtype)
    n = min(len(edge), rows * nb)
    w[:n] = edge[:n]
    return w.reshape(rows, cols)


def _padded(rows, cols, pad, dtype, fill):
    """[rows, cols] view of [rows + 1, cols + pad] storage filled with `fill`: the pitch padding and a guard row behind the matrix"""
    buf = torch.full((rows + 1, cols + pad), fill, dtype=dtype, device=DEV)
    return buf, buf[:rows, :cols]


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("rows,cols", [(1, 32), (5, 96), (33, 160), (257, 4096), (64, 14336)])
def test_kernels_match_the_restatement_bit_for_bit(rows, cols, dtype):
    from lxt_amd import ops
    w = _matrix(rows, cols, dtype, seed=rows + cols)
    codes_ref, scales_ref = mx_quantize(w)
    out_ref = mx_dequant(codes_ref, scales_ref, dtype)
    assert bool(torch.isfinite(out_ref).all())
    for pad in (0, 64):
        wbuf, wd = _padded(rows, cols, pad, dtype, 3.0)
        wd.copy_(w)
        cbuf, codes = _padded(rows, cols // 2, pad, torch.uint8, 0xA5)
        # (scale rows keep the 4-byte pitch the kernel asks for: K / 32 = 1, 3, 5 are no multiples of 4)
        sbuf, scales = _padded(rows, cols // 32, pad + -(cols // 32 + pad) % 4, torch.uint8, 0xA5)
        ops.mxfp4_quantize(wd, codes, scales)
        assert torch.equal(codes.cpu(), codes_ref) and torch.equal(scales.cpu(), scales_ref), (pad, "quantise")
        obuf, out = _padded(rows, cols, pad, dtype, 7.0)
        ops.mxfp4_dequant(codes, scales, out)
        got = out.cpu()
        bits = torch.int16 if dtype == BF16 else torch.int32          # (torch.equal takes -0.0 for 0.0: the quantiser emits no signed zero)
        assert torch.equal(got, out_ref) and torch.equal(got.view(bits), out_ref.view(bits)), (pad, "dequant")
        # nothing outside the rows' columns is written: pitch padding and the guard row keep their fill
        for buf, v, fill in ((cbuf, codes, 0xA5), (sbuf, scales, 0xA5), (obuf, out, 7.0)):
            keep = torch.ones_like(buf, dtype=torch.bool)
            keep[: v.shape[0], : v.shape[1]] = False
            assert bool((buf[keep] == fill).all()), (pad, "wrote outside its matrix")
        # the allocating form of the binding, and the round trip
        c2, s2 = ops.mxfp4_quantize(out)
        assert torch.equal(c2.cpu(), codes_ref) and torch.equal(s2.cpu(), scales_ref)


def test_dequant_scale_255_is_nan_and_binding_checks_shapes():
    from lxt_amd import ops
    codes = torch.zeros(2, 32, dtype=torch.uint8, device=DEV)
    scales = torch.tensor([[127, 255], [255, 127]], dtype=torch.uint8, device=DEV)
    pad = torch.zeros(2, 4, dtype=torch.uint8, device=DEV)
    pad[:, :2] = scales
    out = ops.mxfp4_dequant(codes, pad[:, :2], torch.empty(2, 64, device=DEV)).cpu()
    assert out[0, 32:].isnan().all() and out[1, :32].isnan().all() and not out[0, :32].any() and not out[1, 32:].any()
    w = torch.zeros(4, 64, device=DEV)
    for bad in (dict(codes=torch.zeros(4, 16, dtype=torch.uint8, device=DEV)), dict(scales=torch.zeros(4, 4, dtype=torch.uint8, device=DEV)),
                dict(codes=torch.zeros(4, 32, dtype=torch.int8, device=DEV))):
        with pytest.raises(ValueError):
            ops.mxfp4_quantize(w, **bad)
    with pytest.raises(ValueError):
        ops.mxfp4_quantize(torch.zeros(4, 48, device=DEV))
    with pytest.raises(ValueError):
        ops.mxfp4_quantize(torch.zeros(4, 64, device=DEV, dtype=torch.float16))


# ---- the engine: identity with an ordinary engine on the dequantised weights -------------------------------------------------------------------
KEYS = ("R_tok", "idx", "logit", "layer_R", "R_trace", "R_resid", "R_mlp")


def _same(a, b, what):
    for k in KEYS:
        assert (k in a) == (k in b), (what, k)
        if k in a:
            assert torch.equal(a[k], b[k]), (what, k, nmax(a[k], b[k]))


def _llama(d):
    """the d = 128 Llama of tests/golden (llama_d128.npz: H 512, I 1024, 2 layers, 4 + 1 heads); d = 64: the same widths as 8 + 2 heads of 64"""
    from oracle import llama as ol
    cfg, W, _, _ = llama_case("d128")
    if d == 64:
        cfg = dict(cfg, n_heads=8, n_kv=2, head_dim=64)
        W = ol.random_weights(cfg, seed=64)
    return cfg, W


def _pair(cls, cfg, W, **kw):
    q = cls(cfg, W, weight_format="mxfp4", device=DEV, **kw)
    plain = cls(*q.dequantized_weights(), device=DEV, **kw)
    assert q.weight_format == "mxfp4" and plain.weight_format is None and q.dtype == plain.dtype
    return q, plain


@pytest.mark.parametrize("d", [64, 128])
def test_llama_bf16_equals_the_engine_on_its_dequantised_weights(d):
    from lxt_amd.engine import LlamaLRP, MX_MATRICES
    cfg, W = _llama(d)
    ids = torch.randint(0, cfg["vocab"], (3, 160), generator=torch.Generator().manual_seed(d))
    for sparse_top in (True, False):
        q, plain = _pair(LlamaLRP, cfg, W, max_seq=1024, sparse_top=sparse_top)
        if sparse_top:
            # the ordinary engine folded by exactly 1.0: the same bits in its matrices as the quantised engine computes with
            for li in range(cfg["n_layers"]):
                q._load_layer(li)
                for k in MX_MATRICES:
                    assert torch.equal(q.layers[li][k], plain.layers[li][k]), (li, k)
                assert bool((q.layers[li]["ln1"] == 1).all())
        _same(q.explain(ids, layer_relevance=True), plain.explain(ids, layer_relevance=True), ("plain", sparse_top))
        _same(q.explain(ids, layer_relevance=True, lengths=[160, 97, 5]), plain.explain(ids, layer_relevance=True, lengths=[160, 97, 5]),
              ("lengths", sparse_top))
        lat = ("trace", "resid", "mlp")
        _same(q.explain(ids, latent=lat), plain.explain(ids, latent=lat), ("latent", sparse_top))
        del q, plain


def test_llama_bf16_fused_layer_path_equals_the_engine_on_its_dequantised_weights():
    """B S = 24576 rows at H 512 / I 1024: the smallest row count at which every GEMM of the layer (the narrowest: 512 columns) fills the 190
    output tiles the fused-epilogue kernels ask for -- asserted, so the test cannot quietly run the un-fused path only"""
    from lxt_amd.engine import LlamaLRP
    cfg, W = _llama(128)
    B, S = 24, 1024
    q, plain = _pair(LlamaLRP, cfg, W, max_seq=S)
    assert q._fused(B * S).norm and plain._fused(B * S).norm and not q._fused(B * S // 2).norm
    ids = torch.randint(0, cfg["vocab"], (B, S), generator=torch.Generator().manual_seed(7))
    _same(q.explain(ids, layer_relevance=True), plain.explain(ids, layer_relevance=True), "fused")
    _same(q.explain(ids, latent=("trace", "resid", "mlp")), plain.explain(ids, latent=("trace", "resid", "mlp")), "fused latent")


@pytest.mark.parametrize("case", ["qwen2_d64", "qwen3_d128"])
def test_qwen_bf16_equals_the_engine_on_its_dequantised_weights(case):
    from tests.golden import qwen_models as qm
    from lxt_amd.engine_qwen import QwenLRP
    q = QwenLRP.from_hf(qm.to_bf16_rotary_fp32(qm.build(case)), max_seq=256, weight_format="mxfp4", device=DEV)
    plain = QwenLRP(*q.dequantized_weights(), max_seq=256, device=DEV)
    assert q.weight_format == "mxfp4" and q.flat.dtype == BF16 and ("bqkv" in q.layers[0]) == (case == "qwen2_d64")
    assert ("qn" in q.layers[0]) == (case == "qwen3_d128") and q.layers[0].get("bqkv", q.layers[0].get("qn")).dtype == BF16
    ids = qm.prompts(case)[:3, :192]
    _same(q.explain(ids, layer_relevance=True), plain.explain(ids, layer_relevance=True), case)
    _same(q.explain(ids, lengths=[192, 100, 17], latent=("trace", "resid", "mlp")),
          plain.explain(ids, lengths=[192, 100, 17], latent=("trace", "resid", "mlp")), case + " lengths latent")


def test_graph_replay_equals_eager_bit_for_bit_and_dequant_runs_once_per_layer_and_pass(monkeypatch):
    from lxt_amd import ops
    from lxt_amd.engine import LlamaLRP
    cfg, W = _llama(128)
    q = LlamaLRP(cfg, W, weight_format="mxfp4", device=DEV, max_seq=256)
    ids = torch.randint(0, cfg["vocab"], (2, 128), generator=torch.Generator().manual_seed(3))
    calls, inner = [], ops.mxfp4_dequant
    monkeypatch.setattr(ops, "mxfp4_dequant", lambda c, s, o: (calls.append((c.data_ptr(), torch.cuda.current_stream().cuda_stream)), inner(c, s, o))[1])
    eager = {k: v.clone() for k, v in q.explain(ids, layer_relevance=True).items()}
    # every matrix of every layer once in the forward and once in the backward, all on the explanation's stream
    assert len(calls) == 2 * 4 * cfg["n_layers"] and len({c for c, _ in calls}) == 4 * cfg["n_layers"] and len({s for _, s in calls}) == 1
    g1 = {k: v.clone() for k, v in q.explain(ids, layer_relevance=True, graph=True).items()}
    n = len(calls)
    g2 = q.explain(ids, layer_relevance=True, graph=True)
    assert len(calls) == n                                        # a replay launches nothing from Python
    for g in (g1, g2):
        for k in ("R_tok", "idx", "logit", "logits", "layer_R"):
            assert torch.equal(g[k], eager[k]), k


# ---- the fp32 parity engine against the real reference -------------------------------------------------------------------------------------------
def test_fp32_engine_matches_the_reference_on_the_dequantised_weights():
    """tests/golden/mxfp4_llama.npz: the reference (fp64) on the quantise-dequantise images of the Linears; the fp32 engine quantises the
    ORIGINAL weights itself.  Bar: 1e-4 normalised max (every fp32 engine test's); the reference's own fp32 run is within
    1e-5 of its fp64 run on this instance (asserted by the generator, recorded as ref_fp32_gap)"""
    from oracle import llama as ol
    from lxt_amd.engine import LlamaLRP
    fx = load("mxfp4_llama.npz")
    cfg = {k: (float(v) if k in ("rope_theta", "rms_eps") else int(v)) for k, v in zip(fx["cfg_keys"].tolist(), fx["cfg_vals"].tolist())}
    W = ol.random_weights(cfg, seed=int(fx["wseed"]))
    eng = LlamaLRP(cfg, W, dtype=F32, device=DEV, max_seq=int(fx["S"]), weight_format="mxfp4")
    assert not eng.folded and eng.scratch.dtype == F32
    Q = eng._qlayers[0]
    assert np.array_equal(Q["wd_c"].cpu().numpy(), fx["wd_codes"]) and np.array_equal(Q["wd_s"].cpu().numpy(), fx["wd_scales"])
    for sparse_top in (True, False):
        eng.sparse_top = sparse_top
        out = eng.explain(t(fx["ids"])[None])
        err = nmax(out["R_tok"][0], fx["R_tok"])
        print(f"[mxfp4 fp32 parity] sparse_top {sparse_top}: idx {int(out['idx'][0])} (ref {int(fx['idx'])}), logit {float(out['logit'][0]):+.6f} "
              f"(ref {float(fx['logit']):+.6f}), R_tok normalised max {err:.2e}; the reference's own fp32 {float(fx['ref_fp32_gap']):.1e}")
        assert int(out["idx"][0]) == int(fx["idx"]) and err <= 1e-4
    # the same model as an ordinary fp32 engine on the dequantised weights: the W^T copies cached on the shared scratch must not go stale
    plain = LlamaLRP(*eng.dequantized_weights(), dtype=F32, device=DEV, max_seq=int(fx["S"]), sparse_top=False)
    # (a stale copy would be another layer's matrix: an error of order 1; fp32 reduction orders are not pinned, so no bit identity is asked)
    assert nmax(plain.explain(t(fx["ids"])[None])["R_tok"], out["R_tok"]) <= 1e-5


# ---- refusals, accounting, the default path --------------------------------------------------------------------------------------------------
def test_non_finite_weights_are_refused_naming_the_layer():
    from lxt_amd.engine import LlamaLRP
    cfg, W = _llama(128)
    W = dict(W, layers=[dict(L) for L in W["layers"]])
    W["layers"][1]["wo"] = W["layers"][1]["wo"].clone()
    W["layers"][1]["wo"][5, 7] = float("inf")
    with pytest.raises(ValueError, match="layer 1"):
        LlamaLRP(cfg, W, weight_format="mxfp4", device=DEV, max_seq=64)


def test_weight_bytes_and_device_memory():
    from lxt_amd import engine as E
    cfg, W = _llama(128)
    # memory_allocated counts whole blocks: a block under 1 MiB is rounded up to 512 bytes, a larger one may keep up to 1 MiB of the segment
    # it was cut from; "requested_bytes" of the allocator's statistics is the exact sum of what was asked for
    SMALL, LARGE = 512, 1 << 20
    slack = lambda *sizes: sum(SMALL if n < LARGE else LARGE for n in sizes)      # noqa: E731
    asked = lambda: torch.cuda.memory_stats(DEV).get("requested_bytes.all.current")      # noqa: E731
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base, base_req = torch.cuda.memory_allocated(DEV), asked()
    plain = E.LlamaLRP(cfg, W, device=DEV, max_seq=256)
    wb = plain.weight_bytes()
    assert plain.flat_q is None and plain.scratch is None and wb == dict(resident=plain.flat.numel() * 2, scratch=0)
    tables = plain.cos.numel() * 4 * 2
    used = torch.cuda.memory_allocated(DEV) - base
    assert 0 <= used - (wb["resident"] + tables) <= slack(wb["resident"], tables // 2, tables // 2), (used, wb)
    assert base_req is None or asked() - base_req == wb["resident"] + tables
    del plain
    gc.collect()
    torch.cuda.empty_cache()
    base, base_req = torch.cuda.memory_allocated(DEV), asked()
    q = E.LlamaLRP(cfg, W, device=DEV, max_seq=256, weight_format="mxfp4")
    qb = q.weight_bytes()
    top, layer = E.LlamaLRP.flat_layout(cfg, BF16)
    rest, lin, _ = E.quant_layout(layer)
    nL = cfg["n_layers"]
    kept = E.pack_flat(top, rest, nL, BF16, "meta")[0].numel() * 2                  # the unquantised parts: embedding, LM head, norms
    assert q.flat.numel() * 2 == kept and qb["resident"] == kept + q.flat_q.numel() and q.flat_q.dtype == torch.uint8
    assert qb["resident"] <= 0.27 * (wb["resident"] - kept) + kept
    assert qb["scratch"] == E.pack_flat({}, lin, 1, BF16, "meta")[0].numel() * 2 == q.scratch.numel() * 2
    for k in E.MX_MATRICES:          # one scratch layer, at the engine's pitches, shared by every layer's dict
        assert all(L[k].data_ptr() == q.layers[0][k].data_ptr() and L[k].stride() == q.layers[0][k].stride() for L in q.layers)
        assert q.layers[0][k].stride(0) == E.pack_flat(top, layer, nL, BF16, "meta")[2][0][k].stride(0)
    used = torch.cuda.memory_allocated(DEV) - base
    assert 0 <= used - (qb["resident"] + qb["scratch"] + tables) <= slack(kept, q.flat_q.numel(), qb["scratch"], tables // 2, tables // 2), (used, qb)
    assert base_req is None or asked() - base_req == qb["resident"] + qb["scratch"] + tables
    assert q.flat_q.data_ptr() % 128 == 0 and all(v.data_ptr() % 128 == 0 for Q in q._qlayers for v in Q.values())


def test_default_engine_is_untouched(monkeypatch):
    from lxt_amd import ops
    from lxt_amd.engine import LlamaLRP
    cfg, W = _llama(128)
    eng = LlamaLRP(cfg, W, device=DEV, max_seq=256)
    assert eng.weight_format is None and eng.flat_q is None and eng.scratch is None and eng.weight_bytes()["scratch"] == 0
    assert all(L["wqkv"].untyped_storage().data_ptr() == eng.flat.untyped_storage().data_ptr() for L in eng.layers)

    def boom(*a, **k):
        raise AssertionError("the default engine dequantises nothing")
    monkeypatch.setattr(ops, "mxfp4_dequant", boom)
    monkeypatch.setattr(ops, "mxfp4_quantize", boom)
    ids = torch.randint(0, cfg["vocab"], (2, 96), generator=torch.Generator().manual_seed(1))
    out = eng.explain(ids)
    assert bool(torch.isfinite(out["R_tok"]).all())
