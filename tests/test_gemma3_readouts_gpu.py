"""GPU: the read-outs of the Gemma-3 drivers.
  (1) ops.attn_relmap in bf16 at d = 256 (lrp_attn_relmap_d256) against an fp64 torch restatement on the rounded operands, as
      test_attn_map_gpu.test_relmap_vs_fp64: padded pitches, GQA with rep 2 and 4, a head range, gscale, causal off, left-pad and sliding
      window intervals, one and many tiles; NaN-filled out comes back finite, masked entries exactly 0, bitwise repeatable, batch invariant;
  (2) Gemma3LRP in fp32 against tests/golden/gemma3_readouts_tiny.npz / gemma3_readouts_d256.npz (the REAL lxt.efficient in fp64,
      make_golden_gemma3_readouts.py), sparse top layer on and off, left-padded inside a batch; nothing else moves with a request;
  (3) Gemma3LRP in bf16 at d = 256 against the fp64 fixture, bar 3 x the reference's own bf16 loss on the instance;
  (4) Gemma3MMLRP in fp32 against gemma3_mm_readouts.npz, and a text-only prompt through it against Gemma3LRP."""
import functools

import pytest
import torch

from tests.util import load, nmax, ref_bar

pytestmark = pytest.mark.gpu

LATENT = ("trace", "resid", "mlp")
HEADS = ("out", "q", "k", "v")
PLAIN = ("R_tok", "logit", "idx", "logits")


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import lxt_amd.engine_gemma3 as g3
    from lxt_amd import ops
    return g3, ops


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
def _intervals(B, S, lengths, window):
    """left-pad key intervals as engine.explain_inputs builds them (prompt b occupies columns S - lengths[b] .. S - 1, pad rows empty) and / or
    a sliding window folded into the lower ends, lo = max(first, i - w + 1)"""
    i = torch.arange(S, device="cuda", dtype=torch.int32)
    first = torch.zeros(B, 1, device="cuda", dtype=torch.int32)
    if lengths is not None:
        first = (S - torch.tensor(lengths, device="cuda", dtype=torch.int32))[:, None]
    lo = first.expand(B, S)
    if window:
        lo = torch.maximum(lo, (i - (window - 1))[None].expand(B, S))
    hi = torch.where(i[None] >= first, (i + 1)[None].expand(B, S), torch.zeros(B, S, device="cuda", dtype=torch.int32))
    return lo.contiguous(), hi.contiguous()


@functools.lru_cache(maxsize=None)
def _case(B, S, Hq, Hkv, causal, lengths, window):
    """bf16 operands at d = 256 with padded pitches (a different pad on each), the mask, and the fp64 restatement of every head's map on the
    rounded operands: computed once per case and shared"""
    d, dtype = 256, torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(S + Hq + d)
    mk = lambda nh, pad: torch.randn(B * S, nh * d + pad * 8, generator=gen, device="cuda").to(dtype)      # noqa: E731
    store = (mk(Hq, 1), mk(Hkv, 3), mk(Hkv, 2), mk(Hq, 4))
    q, k, vv, g = (t[:, : nh * d] for t, nh in zip(store, (Hq, Hkv, Hkv, Hq)))
    scale, rep = d ** -0.5, Hq // Hkv
    i = torch.arange(S, device="cuda")
    vis = torch.ones(B, S, S, dtype=torch.bool, device="cuda")
    if causal:
        vis &= (i[None, :] <= i[:, None])[None]
    iv = None
    if lengths is not None or window:
        iv = _intervals(B, S, lengths, window)
        vis &= (i[None, None, :] >= iv[0][:, :, None]) & (i[None, None, :] < iv[1][:, :, None])
    hd = lambda t, nh: t.double().view(B, S, nh, d).permute(0, 2, 1, 3)                                      # noqa: E731
    kd, vd = hd(k, Hkv).repeat_interleave(rep, 1), hd(vv, Hkv).repeat_interleave(rep, 1)
    sc = (scale * hd(q, Hq) @ kd.transpose(2, 3)).masked_fill(~vis[:, None], float("-inf"))
    lse = torch.logsumexp(sc, -1)                                                                        # (-inf on a row that sees nothing)
    maps = torch.where(vis[:, None], torch.exp(sc - lse[..., None]) * (hd(g, Hq) @ vd.transpose(2, 3)), torch.zeros((), dtype=torch.float64, device="cuda"))
    return store, (q, k, vv, g), lse.float().contiguous(), iv, vis, maps, scale


#        B  S    Hq Hkv heads   gscale causal lengths        window
CASES = [(1, 1, 1, 1, None, 1.0, True, None, 0),
         (3, 130, 4, 2, None, 2.0, True, None, 0),
         (3, 130, 4, 2, None, 2.0, False, None, 0),
         (3, 130, 4, 2, None, 2.0, True, (130, 37, 1), 0),
         (2, 200, 4, 1, (1, 3), 1.0, True, None, 70),
         (2, 520, 4, 2, None, 1.0, True, None, 0)]


@pytest.mark.parametrize("B,S,Hq,Hkv,heads,gscale,causal,lengths,window", CASES)
def test_relmap_d256_vs_fp64(mods, B, S, Hq, Hkv, heads, gscale, causal, lengths, window):
    """normalised max error against the fp64 restatement <= 1e-5, the family's bar: both contractions accumulate in fp32 and P, G_P are never
    rounded (d 64 / 128 measure 2e-7 .. 6e-7; twice the fp32 terms do not approach the bar)"""
    _, ops = mods
    d = 256
    store, (q, k, v, g), lse, iv, vis, maps, scale = _case(B, S, Hq, Hkv, causal, lengths, window)
    lo, hi = heads or (0, Hq)
    ref = gscale * maps[:, lo:hi].sum(1)
    out = torch.full((B, S, S), float("nan"), device="cuda")
    kw = dict(heads=heads, gscale=gscale, causal=causal)
    assert ops.attn_relmap(q, k, v, g, lse, B, S, Hq, Hkv, d, scale, row_iv=iv, out=out, **kw) is out
    assert all(t.stride(0) > t.shape[1] for t in (q, k, v, g)) and q.dtype == torch.bfloat16
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    print(f"[attn_relmap bf16 d=256 B={B} S={S} Hq={Hq} Hkv={Hkv} heads={heads} gscale={gscale} causal={causal} lengths={lengths} "
          f"window={window}] normalised max err vs fp64 {err:.2e}")
    assert torch.isfinite(out).all(), "a NaN-filled out must come back fully written, pad rows included"
    assert not out[~vis].any(), "masked (i, j) must be exactly 0"
    assert out.dtype == torch.float32 and err <= 1e-5
    assert torch.equal(ops.attn_relmap(q, k, v, g, lse, B, S, Hq, Hkv, d, scale, row_iv=iv, **kw), out)
    for b in {0, B - 1}:
        rows = slice(b * S, (b + 1) * S)
        iv1 = None if iv is None else (iv[0][b:b + 1].contiguous(), iv[1][b:b + 1].contiguous())
        one = ops.attn_relmap(q[rows], k[rows], v[rows], g[rows], lse[b:b + 1].contiguous(), 1, S, Hq, Hkv, d, scale, row_iv=iv1, **kw)
        assert torch.equal(one[0], out[b])


# ---- the engine in fp32 against the reference -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(name):
    from tests.golden import gemma3_readout_models as gm
    from tests.golden.hf_models import build_gemma3, wsum
    fx = load(f"gemma3_readouts_{name}.npz")
    model = build_gemma3(seed=3, attn="eager") if name == "tiny" else gm.build_gemma3_d256()
    assert abs(wsum(model) - float(fx["wsum"])) <= 1e-9 * float(fx["wsum"]), "seeded weights did not reproduce"
    return model, torch.from_numpy(fx["ids"]).long(), fx


def _pairs(fx, nq):
    layers = fx["head_layers"].tolist()
    return [(layers[-1], nq - 1), (layers[0], 0), (layers[len(layers) // 2], nq - 2), (layers[0], nq // 2), (layers[-1], 1)]


def _errors(out, fx, pairs, b=0, live=slice(None)):
    """normalised max error of every read-out of prompt b against the fixture (live: the prompt's columns inside a padded batch)"""
    layers = fx["head_layers"].tolist()
    e = dict(layer_R=nmax(out["layer_R"][:, b], fx["trace"].sum(-1)), trace=nmax(out["R_trace"][:, b, live], fx["trace"]),
             resid=nmax(out["R_resid"][:, b], fx["resid"]), mlp=nmax(out["R_mlp"][:, b], fx["mlp"]),
             head=nmax(out["R_head"][:, b], fx["out"].sum(-1)), total=nmax(out["R_attn"][:, b, live, live], fx["total"]))
    for n in HEADS:
        e[n] = nmax(out["R_head_" + n][:, b, :, live], fx[n])
    for n, (l, h) in enumerate(pairs):
        e[(l, h)] = nmax(out["R_attn_heads"][n, b, live, live], fx["per_head"][layers.index(l), h])
    return e


def _outside(fx, S, first=0):
    """[L, S, S] bool: what no row may see -- above the diagonal, in front of the prompt's first column, outside a sliding layer's window"""
    i = torch.arange(S, device="cuda")
    dead = (i[None, :] > i[:, None]) | (i[None, :] < first) | (i[:, None] < first)
    win = i[None, :] <= i[:, None] - int(fx["window"])
    return torch.stack([dead | win if s else dead for s in fx["layer_sliding"].tolist()])


@pytest.mark.parametrize("sparse_top", [True, False])
@pytest.mark.parametrize("name", ["tiny", "d256"])
def test_engine_fp32_readouts_vs_reference(mods, name, sparse_top):
    g3, _ = mods
    model, ids, fx = _model(name)
    S, nq = ids.numel(), fx["out"].shape[1]
    L = fx["out"].shape[0]
    pairs = _pairs(fx, nq)
    eng = g3.Gemma3LRP.from_hf(model, dtype=torch.float32, max_seq=S, sparse_top=sparse_top)
    plain = eng.explain(ids[None])
    out = eng.explain(ids[None], layer_relevance=True, latent=LATENT, heads=HEADS, attn_map=["sum"] + pairs)
    assert int(out["idx"][0]) == int(fx["idx"]) and out["attn_map_heads"] == pairs
    H, I = fx["resid"].shape[1], fx["mlp"].shape[1]
    shapes = dict(layer_R=(L + 1, 1), R_trace=(L + 1, 1, S), R_resid=(L + 1, 1, H), R_mlp=(L, 1, I), R_head=(L, 1, nq), R_attn=(L, 1, S, S),
                  R_attn_heads=(len(pairs), 1, S, S), **{"R_head_" + n: (L, 1, nq, S) for n in HEADS})
    for k, shp in shapes.items():
        assert tuple(out[k].shape) == shp and out[k].dtype == torch.float32, k
    errs = _errors(out, fx, pairs)
    e_row = nmax(out["R_attn"].sum(-1), out["R_head_out"].sum(2))
    print(f"[gemma3 {name} fp32, sparse_top={sparse_top}] vs reference fp64: " + "  ".join(f"{k} {e:.2e}" for k, e in errs.items())
          + f"   R_attn.sum(-1) vs R_head_out.sum(heads) {e_row:.2e}")
    assert max(errs.values()) <= 1e-4 and e_row <= 1e-4
    dead = _outside(fx, S)
    assert not out["R_attn"][:, 0][dead].any()
    for n, (l, h) in enumerate(pairs):
        assert not out["R_attn_heads"][n, 0][dead[l]].any()
    assert not out["R_attn"][L - 1, :, : S - 1].any() and out["R_attn"][L - 1, :, S - 1].abs().max() > 0
    # nothing else moves, and each request alone gives its outputs alone, the same bits
    assert set(plain) == set(PLAIN)
    for k in PLAIN:
        assert torch.equal(out[k], plain[k]), k
    alone = [dict(layer_relevance=True), dict(latent="trace"), dict(latent="resid"), dict(latent="mlp"), dict(attn_map="sum"),
             dict(attn_map=[pairs[2]])] + [dict(heads=n) for n in HEADS]
    for kw in alone:
        one = eng.explain(ids[None], **kw)
        keys = set(one) - set(PLAIN) - {"attn_map_heads"}
        assert keys and all(torch.equal(one[k], plain[k]) for k in PLAIN), kw
        for k in keys - {"R_attn_heads"}:
            assert torch.equal(one[k], out[k]), (kw, k)
        if "R_attn_heads" in keys:
            assert torch.equal(one["R_attn_heads"][0], out["R_attn_heads"][2]) and one["attn_map_heads"] == [pairs[2]]
    assert set(eng.explain(ids[None], latent="mlp")) == set(PLAIN) | {"R_mlp"}


def test_engine_fp32_readouts_left_padded_vs_reference(mods):
    """the tiny prompt left-padded inside a batch of 2: the reference's read-outs on its live block, pad rows and columns exactly 0"""
    g3, _ = mods
    model, ids, fx = _model("tiny")
    n, S = ids.numel(), ids.numel() + 24
    pairs = _pairs(fx, fx["out"].shape[1])
    other = torch.randint(0, 512, (S,), generator=torch.Generator().manual_seed(99))
    batch = torch.stack([torch.cat([torch.zeros(S - n, dtype=ids.dtype), ids]), other])
    for sparse_top in (True, False):
        eng = g3.Gemma3LRP.from_hf(model, dtype=torch.float32, max_seq=S, sparse_top=sparse_top)
        out = eng.explain(batch, lengths=[n, S], layer_relevance=True, latent=LATENT, heads=HEADS, attn_map=["sum"] + pairs)
        assert int(out["idx"][0]) == int(fx["idx"])
        errs = _errors(out, fx, pairs, live=slice(S - n, None))
        print(f"[gemma3 tiny fp32, left-padded by {S - n}, sparse_top={sparse_top}] " + "  ".join(f"{k} {e:.2e}" for k, e in errs.items()))
        assert max(errs.values()) <= 1e-4
        dead = _outside(fx, S, first=S - n)
        assert torch.isfinite(out["R_attn"]).all() and not out["R_attn"][:, 0][dead].any() and out["R_attn"][:, 1].abs().max() > 0
        assert not out["R_attn_heads"][:, 0, : S - n].any() and not out["R_attn_heads"][:, 0, :, : S - n].any()
        for k in ("R_trace",) + tuple("R_head_" + h for h in HEADS):
            assert not out[k][:, 0, ..., : S - n].any(), k


# ---- bf16 at d = 256 -------------------------------------------------------------------------------------------------------------------
def test_engine_bf16_d256_readouts_vs_reference(mods):
    """bf16 Gemma3LRP (lrp_attn_relmap_d256, the d = 256 attention kernels) on the d256 model, target = the fixture's idx, against the fp64
    fixture: every output within 3 x gap_bf16 of that output, the reference's OWN bf16 loss on this instance (tests.util.ref_bar: one
    instance is one draw).  Measured on an MI355X, engine error / the reference's gap: layer_R 2.58e-3 / 3.75e-3,
    trace 2.19e-3 / 3.80e-3, resid 1.39e-2 / 8.08e-3, mlp 1.22e-2 / 1.04e-2, sum map 9.76e-3 / 9.98e-3, out 1.06e-2 / 1.29e-2, q 1.05e-2 /
    1.04e-2, k 8.50e-3 / 1.14e-2, v 7.48e-3 / 1.01e-2, pairs (2, 3) 1.24e-2 / 1.61e-2, (0, 0) 4.12e-3 / 6.28e-3, (1, 2) 2.26e-2 / 2.35e-2,
    (0, 2) 1.12e-2 / 1.65e-2, (2, 1) 5.90e-2 / 6.21e-2: the largest ratio is 1.72 (resid)."""
    g3, _ = mods
    from tests.golden import gemma3_readout_models as gm
    model, ids, fx = _model("d256")
    S, nq = ids.numel(), fx["out"].shape[1]
    pairs = _pairs(fx, nq)
    eng = g3.Gemma3LRP.from_hf(gm.build_gemma3_d256().to(torch.bfloat16), dtype=torch.bfloat16, max_seq=S)
    assert eng.cfg["head_dim"] == 256
    out = eng.explain(ids[None], target=[int(fx["idx"])], layer_relevance=True, latent=LATENT, heads=HEADS, attn_map=["sum"] + pairs)
    plain = eng.explain(ids[None], target=[int(fx["idx"])])
    for k in PLAIN:
        assert torch.equal(out[k], plain[k]), k
    errs = _errors(out, fx, pairs)
    del errs["head"]
    gap = lambda k: float(fx["gap_bf16/per_head"][k] if isinstance(k, tuple) else fx["gap_bf16/" + k])      # noqa: E731  (a head's map: its own gap)
    print("[gemma3 d256 bf16] engine vs reference fp64 / the reference's own bf16 gap: "
          + "  ".join(f"{k} {e:.2e} / {gap(k):.2e}" for k, e in errs.items()))
    assert not out["R_attn"][:, 0][_outside(fx, S)].any() and torch.isfinite(out["R_attn"]).all()
    for k, e in errs.items():
        assert e <= ref_bar(gap(k), floor=0.0), (k, e, gap(k))


# ---- image + text ---------------------------------------------------------------------------------------------------------------------
def test_mm_engine_fp32_readouts_vs_reference(mods):
    g3, _ = mods
    import lxt_amd.engine_gemma3_mm as mm
    from tests.golden.hf_models import build_gemma3_mm, gemma3_mm_inputs, wsum
    fx = load("gemma3_mm_readouts.npz")
    model = build_gemma3_mm(attn="eager")
    assert abs(wsum(model) - float(fx["wsum"])) <= 1e-9 * float(fx["wsum"]), "seeded weights did not reproduce"
    ids, tt, pv = gemma3_mm_inputs()
    assert torch.equal(ids, torch.from_numpy(fx["ids"]))
    eng = mm.Gemma3MMLRP.from_hf(model, dtype=torch.float32, max_seq=256, vision_attn_rule=False)      # (eager: the tower's attention is not patched)
    plain = eng.explain(ids, pv, token_type_ids=tt)
    out = eng.explain(ids, pv, token_type_ids=tt, layer_relevance=True, heads="out", attn_map="sum")
    assert int(out["idx"][0]) == int(fx["idx"])
    errs = dict(layer_R=nmax(out["layer_R"][:, 0], fx["layer_R"]), out=nmax(out["R_head_out"][:, 0], fx["out"]),
                total=nmax(out["R_attn"][:, 0], fx["total"]))
    print("[gemma3 image + text fp32] vs reference fp64: " + "  ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert max(errs.values()) <= 1e-4
    img = tt[0].bool().cuda()
    blk = img[:, None] & img[None, :]
    up = torch.ones_like(blk).triu(1)
    assert not out["R_attn"][:, 0][:, up & ~blk].any() and out["R_attn"][:2, 0][:, up & blk].abs().max() > 0
    for k in ("R_tok", "R_pix", "R_patch", "logit", "idx", "logits"):
        assert torch.equal(out[k], plain[k]), k
    # a text-only prompt through the image + text driver: the text driver's maps, bit for bit
    text = torch.randint(0, 290, (2, 40), generator=torch.Generator().manual_seed(4))
    req = dict(layer_relevance=True, heads=HEADS, attn_map=["sum", (1, 2)])
    a = eng.explain(text, pv[:0], **req)
    b = g3.Gemma3LRP.from_hf(model, dtype=torch.float32, max_seq=256).explain(text, **req)
    for k in ("R_tok", "layer_R", "R_attn", "R_attn_heads", "R_head_out", "R_head_q", "R_head_k", "R_head_v"):
        assert torch.equal(a[k], b[k]), k
