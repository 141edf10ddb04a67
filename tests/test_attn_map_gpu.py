"""GPU: token-to-token attention relevance maps (explain(attn_map=...)) on the Llama / Qwen engines.
  (1) lrp_attn_relmap against an fp64 torch restatement on the rounded inputs (lse computed in fp64, then cast): bf16 / fp32, GQA, head
      ranges, padded pitches, gscale != 1, causal off, left-pad intervals; a NaN-filled out comes back fully written; bitwise repeatable
      and batch invariant;
  (2) LlamaLRP / QwenLRP in fp32 against tests/golden/attn_map_llama.npz / attn_map_qwen3.npz (the REAL lxt.efficient in fp64,
      make_golden_attn_map.py), sparse top layer on and off, left-padded inside a batch; the row sums against R_head_out of the same call;
  (3) the bf16 engine at the Llama-3-8B layer dimensions against the fp32 engine on the same weights: the fused layer plus the sparse top
      layer, one hipGraph replay, and nothing else moves."""
import functools

import pytest
import torch

from oracle import llama as ol
from tests.util import load, nmax

pytestmark = pytest.mark.gpu

LATENT = ("trace", "resid", "mlp")
HEADS = ("out", "q", "k", "v")
OTHERS = ("R_tok", "logit", "idx", "layer_R", "R_trace", "R_resid", "R_mlp", "R_head", "R_head_out", "R_head_q", "R_head_k", "R_head_v")


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import lxt_amd.engine as E
    from lxt_amd import ops
    return E, ops


def _cosine(a, b):
    return float(torch.nn.functional.cosine_similarity(a.double().flatten(), b.double().flatten().to(a.device), dim=0))


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
def _intervals(B, S, lengths):
    """the engine's left-pad key intervals (engine.explain_inputs): prompt b occupies columns S - lengths[b] .. S - 1, pad rows are empty"""
    lens = torch.tensor(lengths, device="cuda", dtype=torch.int32)
    i = torch.arange(S, device="cuda", dtype=torch.int32)
    first = (S - lens)[:, None]
    lo = first.expand(B, S).contiguous()
    hi = torch.where(i[None] >= first, (i + 1)[None].expand(B, S), torch.zeros_like(lo)).contiguous()
    return lo, hi


@functools.lru_cache(maxsize=None)
def _case(dtype, B, S, Hq, Hkv, d, causal, lengths):
    """operands with padded pitches (a different pad on each), the mask, and the fp64 restatement of every head's map on the rounded operands:
    computed once per case and shared"""
    v = 16 // dtype.itemsize
    gen = torch.Generator(device="cuda").manual_seed(S + Hq + d)
    mk = lambda nh, pad: torch.randn(B * S, nh * d + pad * v, generator=gen, device="cuda").to(dtype)      # noqa: E731
    store = (mk(Hq, 1), mk(Hkv, 3), mk(Hkv, 2), mk(Hq, 4))
    q, k, vv, g = (t[:, : nh * d] for t, nh in zip(store, (Hq, Hkv, Hkv, Hq)))
    scale, rep = d ** -0.5, Hq // Hkv
    i = torch.arange(S, device="cuda")
    vis = torch.ones(B, S, S, dtype=torch.bool, device="cuda")
    if causal:
        vis &= (i[None, :] <= i[:, None])[None]
    iv = None
    if lengths is not None:
        iv = _intervals(B, S, lengths)
        vis &= (i[None, None, :] >= iv[0][:, :, None]) & (i[None, None, :] < iv[1][:, :, None])
    hd = lambda t, nh: t.double().view(B, S, nh, d).permute(0, 2, 1, 3)                                      # noqa: E731
    kd, vd = hd(k, Hkv).repeat_interleave(rep, 1), hd(vv, Hkv).repeat_interleave(rep, 1)
    sc = (scale * hd(q, Hq) @ kd.transpose(2, 3)).masked_fill(~vis[:, None], float("-inf"))
    lse = torch.logsumexp(sc, -1)                                                                        # (-inf on a row that sees nothing)
    maps = torch.where(vis[:, None], torch.exp(sc - lse[..., None]) * (hd(g, Hq) @ vd.transpose(2, 3)), torch.zeros((), dtype=torch.float64, device="cuda"))
    return store, (q, k, vv, g), lse.float().contiguous(), iv, vis, maps, scale


F32, BF16 = torch.float32, torch.bfloat16
#        dtype B  S    Hq Hkv d   heads   gscale causal lengths
CASES = [(F32, 1, 1, 1, 1, 32, None, 1.0, True, None),
         (F32, 2, 77, 4, 2, 32, None, 2.0, True, None),
         (F32, 2, 40, 6, 1, 8, (2, 5), 0.37, True, None)]
for _dt in (BF16, F32):
    CASES += [(_dt, 3, 130, 8, 2, 64, None, 2.0, True, None),
              (_dt, 3, 130, 8, 2, 64, None, 1.0, False, None),
              (_dt, 3, 130, 8, 2, 64, None, 2.0, True, (130, 37, 1)),
              (_dt, 2, 200, 6, 6, 128, (1, 2), 1.0, True, None),
              (_dt, 2, 520, 8, 2, 128, None, 2.0, True, None)]


@pytest.mark.parametrize("dtype,B,S,Hq,Hkv,d,heads,gscale,causal,lengths", CASES)
def test_relmap_vs_fp64(mods, dtype, B, S, Hq, Hkv, d, heads, gscale, causal, lengths):
    """normalised max error against the fp64 restatement <= 1e-5 in both dtypes: both contractions accumulate in fp32 and P, G_P are never
    rounded, so the bar is lrp_headdot's"""
    _, ops = mods
    store, (q, k, v, g), lse, iv, vis, maps, scale = _case(dtype, B, S, Hq, Hkv, d, causal, lengths)
    lo, hi = heads or (0, Hq)
    ref = gscale * maps[:, lo:hi].sum(1)
    out = torch.full((B, S, S), float("nan"), device="cuda")
    kw = dict(heads=heads, gscale=gscale, causal=causal)
    assert ops.attn_relmap(q, k, v, g, lse, B, S, Hq, Hkv, d, scale, row_iv=iv, out=out, **kw) is out
    assert all(t.stride(0) > t.shape[1] for t in (q, k, v, g))
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    print(f"[attn_relmap {dtype} B={B} S={S} Hq={Hq} Hkv={Hkv} d={d} heads={heads} gscale={gscale} causal={causal} lengths={lengths}] "
          f"normalised max err vs fp64 {err:.2e}")
    assert torch.isfinite(out).all(), "a NaN-filled out must come back fully written, pad rows included"
    assert not out[~vis].any(), "masked (i, j) must be exactly 0"
    assert out.dtype == torch.float32 and err <= 1e-5
    # bitwise repeatable, and a prompt's result does not depend on its neighbours
    assert torch.equal(ops.attn_relmap(q, k, v, g, lse, B, S, Hq, Hkv, d, scale, row_iv=iv, **kw), out)
    for b in {0, B - 1}:
        rows = slice(b * S, (b + 1) * S)
        iv1 = None if iv is None else (iv[0][b:b + 1].contiguous(), iv[1][b:b + 1].contiguous())
        one = ops.attn_relmap(q[rows], k[rows], v[rows], g[rows], lse[b:b + 1].contiguous(), 1, S, Hq, Hkv, d, scale, row_iv=iv1, **kw)
        assert torch.equal(one[0], out[b])


def test_relmap_refuses_bad_calls(mods):
    _, ops = mods
    q, kv, lse = torch.randn(60, 64, device="cuda"), torch.randn(60, 32, device="cuda"), torch.zeros(3, 2, 20, device="cuda")
    with pytest.raises(RuntimeError, match="LRP_ESHAPE"):
        ops.attn_relmap(q, kv, kv, q, lse, 3, 20, 2, 1, 32, 1.0, heads=(1, 1))                 # an empty head range
    with pytest.raises(RuntimeError, match="LRP_ESHAPE"):
        ops.attn_relmap(q.bfloat16(), kv.bfloat16(), kv.bfloat16(), q.bfloat16(), lse, 3, 20, 2, 1, 32, 1.0)      # bf16 is served at 64 / 128
    with pytest.raises(ValueError):
        ops.attn_relmap(q, kv, kv, q, lse, 3, 20, 2, 1, 32, 1.0, out=torch.empty(3, 20, 21, device="cuda"))
    with pytest.raises(TypeError):
        ops.attn_relmap(q, kv, kv.bfloat16(), q, lse, 3, 20, 2, 1, 32, 1.0)


# ---- the engines in fp32 against the reference -----------------------------------------------------------------------------------------
def _llama_case():
    fx = load("attn_map_llama.npz")
    cfg = {k: (float(v) if k in ("rope_theta", "rms_eps") else int(v)) for k, v in zip(fx["cfg_keys"].tolist(), fx["cfg_vals"].tolist())}
    W = ol.random_weights(cfg, seed=int(fx["wseed"]))
    tot = float(W["embed"].double().abs().sum() + W["lm_head"].double().abs().sum())
    for L in W["layers"]:
        tot += sum(float(v.double().abs().sum()) for v in L.values())
    assert abs(tot - float(fx["wsum"])) <= 1e-9 * abs(tot), "synthetic weights did not reproduce"
    return cfg, W, torch.from_numpy(fx["ids"]), fx


def _pairs(fx, nq):
    """a handful of (layer, head) pairs among the stored layers, first, a middle and last layer included, not in layer order"""
    layers = fx["head_layers"].tolist()
    return [(layers[-1], nq - 1), (layers[0], 0), (layers[len(layers) // 2], nq - 2), (layers[0], nq // 2), (layers[-1], 1)]


def _vs_fixture(tag, out, fx, pairs, b=0, live=slice(None)):
    """normalised max errors of the head sum (over all layers at once) and of every requested pair against the frozen maps"""
    layers = fx["head_layers"].tolist()
    errs = {"sum": nmax(out["R_attn"][:, b, live, live], fx["total"])}
    for n, (l, h) in enumerate(pairs):
        errs[(l, h)] = nmax(out["R_attn_heads"][n, b, live, live], fx["per_head"][layers.index(l), h])
    print(f"[{tag}] vs reference fp64: " + "  ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    return errs


@pytest.mark.parametrize("sparse_top", [True, False])
def test_engine_fp32_attn_map_vs_reference(mods, sparse_top):
    E, _ = mods
    cfg, W, ids, fx = _llama_case()
    L, S, nq = cfg["n_layers"], int(fx["S"]), cfg["n_heads"]
    pairs = _pairs(fx, nq)
    eng = E.LlamaLRP(cfg, W, dtype=torch.float32, mode="efficient", max_seq=S, sparse_top=sparse_top)
    plain = eng.explain(ids[None], layer_relevance=True, latent=LATENT, heads=HEADS)
    out = eng.explain(ids[None], layer_relevance=True, latent=LATENT, heads=HEADS, attn_map=["sum"] + pairs)
    assert int(out["idx"][0]) == int(fx["idx"]) and out["attn_map_heads"] == pairs
    assert out["R_attn"].shape == (L, 1, S, S) and out["R_attn_heads"].shape == (len(pairs), 1, S, S) and out["R_attn"].dtype == torch.float32
    errs = _vs_fixture(f"fp32 attn_map, sparse_top={sparse_top}", out, fx, pairs)
    assert max(errs.values()) <= 1e-4
    # a row of the map splits what heads="out" reports over the source positions
    e_row = nmax(out["R_attn"].sum(-1), out["R_head_out"].sum(2))
    print(f"   R_attn.sum(-1) vs R_head_out.sum(heads) {e_row:.2e}")
    assert e_row <= 1e-4
    # strictly above the diagonal exactly 0; above the top layer only the last query row is live
    up = torch.ones(S, S, dtype=torch.bool, device="cuda").triu(1)
    assert not out["R_attn"][..., up].any() and not out["R_attn_heads"][..., up].any()
    assert not out["R_attn"][L - 1, :, : S - 1].any() and out["R_attn"][L - 1, :, S - 1].abs().max() > 0
    # nothing else moves, and each form alone gives its output alone, the same bits
    assert "R_attn" not in plain and "R_attn_heads" not in plain
    for k in OTHERS:
        assert torch.equal(out[k], plain[k]), k
    only = eng.explain(ids[None], attn_map="sum")
    assert torch.equal(only["R_attn"], out["R_attn"]) and "R_attn_heads" not in only and "attn_map_heads" not in only
    one = eng.explain(ids[None], attn_map=[pairs[2]])
    assert torch.equal(one["R_attn_heads"][0], out["R_attn_heads"][2]) and "R_attn" not in one and one["attn_map_heads"] == [pairs[2]]


def test_engine_fp32_attn_map_left_padded_vs_reference(mods):
    """lengths in fp32: the reference's prompt left-padded inside a batch of 2 still matches the reference's maps on its live block, and its
    pad rows and pad columns are exactly 0"""
    E, _ = mods
    cfg, W, ids, fx = _llama_case()
    n, S = int(fx["S"]), int(fx["S"]) + 32
    pairs = _pairs(fx, cfg["n_heads"])
    other = torch.randint(0, cfg["vocab"], (S,), generator=torch.Generator().manual_seed(99))
    batch = torch.stack([torch.cat([torch.zeros(S - n, dtype=ids.dtype), ids]), other])
    eng = E.LlamaLRP(cfg, W, dtype=torch.float32, mode="efficient", max_seq=S)
    out = eng.explain(batch, lengths=[n, S], attn_map=["sum"] + pairs)
    assert int(out["idx"][0]) == int(fx["idx"])
    errs = _vs_fixture(f"fp32 attn_map, left-padded by {S - n}", out, fx, pairs, live=slice(S - n, None))
    assert max(errs.values()) <= 1e-4
    for t in (out["R_attn"][:, 0], out["R_attn_heads"][:, 0]):
        assert torch.isfinite(t).all() and not t[:, : S - n, :].any() and not t[:, :, : S - n].any()
    assert torch.isfinite(out["R_attn"]).all() and out["R_attn"][:, 1].abs().max() > 0


def test_qwen3_fp32_attn_map_vs_reference(mods):
    """QwenLRP on Qwen3: q and k after the head norms and RoPE, as the attention kernels read them"""
    from lxt_amd.engine_qwen import QwenLRP
    from tests.golden import hf_models
    fx = load("attn_map_qwen3.npz")
    model = hf_models.build_qwen3()
    assert abs(hf_models.wsum(model) - float(fx["wsum"])) <= 1e-9 * float(fx["wsum"]), "seeded weights did not reproduce"
    ids = torch.from_numpy(fx["ids"])
    pairs = _pairs(fx, int(fx["per_head"].shape[1]))
    for sparse_top in (True, False):
        eng = QwenLRP.from_hf(model, dtype=torch.float32, max_seq=int(fx["S"]), sparse_top=sparse_top)
        plain = eng.explain(ids[None], layer_relevance=True, heads="out")
        out = eng.explain(ids[None], layer_relevance=True, heads="out", attn_map=pairs + ["sum"])
        assert int(out["idx"][0]) == int(fx["idx"])
        errs = _vs_fixture(f"fp32 Qwen3 attn_map, sparse_top={sparse_top}", out, fx, pairs)
        assert max(errs.values()) <= 1e-4
        assert nmax(out["R_attn"].sum(-1), out["R_head_out"].sum(2)) <= 1e-4
        for k in ("R_tok", "logit", "idx", "layer_R", "R_head_out"):
            assert torch.equal(out[k], plain[k])


# ---- the bf16 engine at the Llama-3-8B layer dimensions -------------------------------------------------------------------------------
CFG8B = dict(hidden=4096, inter=14336, n_layers=2, n_heads=32, n_kv=8, head_dim=128, vocab=4096, rope_theta=5e5, rms_eps=1e-5)

# (nmax bar, cosine floor) per output of test_engine_bf16_8b_attn_map, and the bar of the row-sum identity in bf16: 3 x the measured values
BARS_8B = {"sum": (3 * 1.03e-2, 0.9999), (0, 5): (3 * 2.41e-2, 0.9998), (1, 31): (3 * 3.96e-2, 0.9994), "rows": 3 * 5.44e-4}


def test_engine_bf16_8b_attn_map(mods):
    """bf16 against the fp32 engine on the same weights and targets, B 4, S 1024: the fully fused dense layer (layer 0) and the sparse top
    layer (layer 1); one hipGraph replay equals the eager call; nothing else moves.  (Four prompts, not two: at B S = 2048 rows the GEMMs
    of these dimensions have fewer output tiles than the fused epilogues take and the layer would run on the partial path, which the fp32
    tests above cover; 4096 rows is the smallest batch of S 1024 that reaches fused_layer_bwd.)
    Bars: 3 x the error measured against the fp32 engine (itself pinned to the reference at 1e-4), the margin the latent tests use for bf16;
    the cosine floor one digit below the measured cosine.  Measured on an MI355X, (nmax, cosine):
    "sum" 1.03e-2, 0.99993;  pair (0, 5) 2.41e-2, 0.99983;  pair (1, 31) 3.96e-2, 0.99948;  R_attn.sum(-1) against R_head_out.sum(heads)
    5.44e-4."""
    E, _ = mods
    H, I, d, B, S, L = 4096, 14336, 128, 4, 1024, 2
    g = torch.Generator(device="cuda").manual_seed(3)
    rn = lambda *s: (torch.randn(*s, generator=g, device="cuda") * 0.02).bfloat16()              # noqa: E731
    nw = lambda: (1.0 + 0.1 * torch.randn(H, generator=g, device="cuda")).bfloat16()            # noqa: E731
    W = dict(embed=rn(4096, H), norm=nw(), lm_head=rn(4096, H),
             layers=[dict(ln1=nw(), ln2=nw(), wq=rn(32 * d, H), wk=rn(8 * d, H), wv=rn(8 * d, H), wo=rn(H, 32 * d), wg=rn(I, H), wu=rn(I, H),
                          wd=rn(H, I)) for _ in range(L)])
    bf = E.LlamaLRP(CFG8B, W, dtype=torch.bfloat16, mode="efficient", max_seq=S)
    f32 = E.LlamaLRP(CFG8B, W, dtype=torch.float32, mode="efficient", max_seq=S)
    ids = torch.randint(0, 4096, (B, S), generator=torch.Generator().manual_seed(4))
    assert bf._fused(B * S).full and bf.sparse_top
    pairs = [(0, 5), (1, 31)]
    req = ["sum"] + pairs
    plain = bf.explain(ids, layer_relevance=True, latent=LATENT, heads=HEADS)
    out = bf.explain(ids, layer_relevance=True, latent=LATENT, heads=HEADS, attn_map=req)
    ref = f32.explain(ids, heads="out", attn_map=req, target=out["idx"])
    for k in OTHERS:
        assert torch.equal(out[k], plain[k]), k
    res = {"sum": (nmax(out["R_attn"], ref["R_attn"]), _cosine(out["R_attn"], ref["R_attn"]))}
    for n, pr in enumerate(pairs):
        res[pr] = (nmax(out["R_attn_heads"][n], ref["R_attn_heads"][n]), _cosine(out["R_attn_heads"][n], ref["R_attn_heads"][n]))
    e_row = nmax(out["R_attn"].sum(-1), out["R_head_out"].sum(2))
    print("[bf16 8B dims attn_map] vs fp32 engine (nmax, cosine): " + "  ".join(f"{k} {e:.2e} {c:.5f}" for k, (e, c) in res.items())
          + f"   R_attn.sum(-1) vs R_head_out.sum(heads) {e_row:.2e}")
    assert out["R_attn"].shape == (L, B, S, S) and torch.isfinite(out["R_attn"]).all() and torch.isfinite(out["R_attn_heads"]).all()
    assert not out["R_attn"][L - 1, :, : S - 1].any() and out["R_attn"][L - 1, :, S - 1].abs().max() > 0
    for k, (e, c) in res.items():
        assert e <= BARS_8B[k][0] and c >= BARS_8B[k][1], (k, e, c)
    assert e_row <= BARS_8B["rows"]
    eager = {k: out[k].clone() for k in OTHERS + ("R_attn", "R_attn_heads")}
    for _ in range(2):                                              # capture, then one replay
        gr = bf.explain(ids, layer_relevance=True, latent=LATENT, heads=HEADS, attn_map=req, graph=True)
    for k, t in eager.items():
        assert torch.equal(gr[k], t), k

