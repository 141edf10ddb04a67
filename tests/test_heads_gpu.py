"""GPU: per-head attention relevance (explain(heads=...)) on the fused Llama / Qwen engines.
  (1) lrp_headdot against an fp64 torch restatement on the rounded inputs: bf16 / fp32, GQA, padded pitches, with and without the rotated
      form, scale != 1; bitwise repeatable and batch invariant; the rotated form against the plain form on an explicitly rotated g;
  (2) LlamaLRP / QwenLRP in fp32 against tests/golden/heads_llama.npz / heads_qwen3.npz (the REAL lxt.efficient in fp64,
      make_golden_heads.py), sparse top layer on and off, left-padded inside a batch;
  (3) the bf16 engine at the Llama-3-8B layer dimensions against the fp32 engine on the same weights: the fully fused layer with the
      rotated read-out plus the sparse top layer; hipGraph replay; the explicit placement;
  (4) nothing else moves: every other output is bitwise the same with and without the request."""
import pytest
import torch

from oracle import llama as ol
from tests.util import load, nmax

pytestmark = pytest.mark.gpu

HEADS = ("out", "q", "k", "v")
LATENT = ("trace", "resid", "mlp")
OTHERS = ("R_tok", "logit", "idx", "layer_R", "R_trace", "R_resid", "R_mlp")


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
def _rotate(g, cos, sin, S, nh, d):
    """forward rotate-half RoPE of g [B S, nh d] at position t = row % S, in g's own precision (fp64 for the reference)"""
    gv = g.view(-1, S, nh, d)
    rot = torch.cat((-gv[..., d // 2:], gv[..., : d // 2]), dim=-1)
    c, s = cos[:S].to(g.dtype)[None, :, None, :], sin[:S].to(g.dtype)[None, :, None, :]
    return (gv * c + rot * s).reshape(g.shape)


def _ref(x, g, B, S, nh, rep, d, scale, rope):
    gd = g.double()
    if rope is not None:
        gd = _rotate(gd, rope[0], rope[1], S, nh, d)
    xd = x.double().view(B, S, nh // rep, d).repeat_interleave(rep, dim=2)
    return scale * (xd * gd.view(B, S, nh, d)).sum(-1).permute(0, 2, 1)


def _tables(S, d, scaling=1.0):
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    from lxt_amd.engine import rope_tables
    return rope_tables(inv, scaling, S + 3, torch.float32, "cuda")


def _operands(dtype, B, S, nh, rep, d, padx, padg, seed):
    v = 16 // dtype.itemsize
    nx, ng = (nh // rep) * d, nh * d
    gen = torch.Generator(device="cuda").manual_seed(seed)
    xs = torch.randn(B * S, nx + padx * v, generator=gen, device="cuda").to(dtype)
    gs = torch.randn(B * S, ng + padg * v, generator=gen, device="cuda").to(dtype)
    return xs, gs, xs[:, :nx], gs[:, :ng]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("B,S,nh,rep,d,padx,padg,scale", [(4, 2048, 32, 4, 128, 0, 0, 1.0), (1, 1, 8, 1, 32, 0, 0, 1.0), (5, 130, 8, 4, 64, 3, 1, 2.0),
                                                          (2, 77, 4, 2, 256, 0, 8, 0.37), (3, 33, 96, 3, 96, 2, 0, 1.0), (2, 40, 6, 1, 8, 1, 5, 4.0)])
def test_headdot_vs_fp64(mods, dtype, rope, B, S, nh, rep, d, padx, padg, scale):
    _, ops = mods
    xs, gs, x, g = _operands(dtype, B, S, nh, rep, d, padx, padg, S + nh + d)
    tab = _tables(S, d, 1.25 if scale != 1.0 else 1.0) if rope else None
    out = ops.headdot(x, g, B, S, nh, rep, d, scale=scale, rope=tab)
    ref = _ref(x, g, B, S, nh, rep, d, scale, tab)
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    print(f"[headdot {dtype} rope={rope} B={B} S={S} nh={nh} rep={rep} d={d} ld=({x.stride(0)},{g.stride(0)}) scale={scale}] "
          f"normalised max err vs fp64 {err:.2e}")
    assert out.shape == (B, nh, S) and out.dtype == torch.float32 and out.is_contiguous() and err <= 1e-5
    # bitwise repeatable (also into a caller's buffer), and a prompt's result does not depend on its neighbours
    into = torch.full((B, nh, S), float("nan"), device="cuda")
    assert ops.headdot(x, g, B, S, nh, rep, d, scale=scale, rope=tab, out=into) is into
    assert torch.equal(into, out) and torch.equal(ops.headdot(x, g, B, S, nh, rep, d, scale=scale, rope=tab), out)
    for b in {0, B - 1}:
        rows = slice(b * S, (b + 1) * S)
        one = ops.headdot(x[rows], g[rows], 1, S, nh, rep, d, scale=scale, rope=tab)
        cp = ops.headdot(xs[rows].clone()[:, : x.shape[1]], gs[rows].clone()[:, : g.shape[1]], 1, S, nh, rep, d, scale=scale, rope=tab)
        assert torch.equal(one[0], out[b]) and torch.equal(cp[0], out[b])


@pytest.mark.parametrize("B,S,nh,rep,d", [(4, 2048, 32, 1, 128), (5, 130, 8, 4, 64), (2, 40, 6, 1, 8)])
def test_headdot_rotated_form_equals_plain_on_rotated_g(mods, B, S, nh, rep, d):
    """sum_d x RoPE(g) by the kernel's rotated form against its plain form on a g rotated ahead of the call.  fp32 operands: a bf16 copy of
    the rotated g would carry a rounding of its own (2^-9) that the rotated read-out does not have"""
    _, ops = mods
    _, _, x, g = _operands(torch.float32, B, S, nh, rep, d, 0, 0, 5)
    tab = _tables(S, d)
    a = ops.headdot(x, g, B, S, nh, rep, d, rope=tab)
    b = ops.headdot(x, _rotate(g, tab[0], tab[1], S, nh, d).contiguous(), B, S, nh, rep, d)
    err = nmax(a, b)
    print(f"[headdot rotated vs plain on a rotated g, B={B} S={S} nh={nh} rep={rep} d={d}] {err:.2e}")
    assert err <= 1e-5


def test_headdot_refuses_bad_calls(mods):
    _, ops = mods
    x = torch.randn(3 * 20, 64, device="cuda")
    with pytest.raises(RuntimeError, match="LRP_ESHAPE"):
        ops.headdot(x, x, 4, 20, 2, 1, 32, out=torch.empty(4, 2, 20, device="cuda"))        # B S != rows
    with pytest.raises(ValueError):
        ops.headdot(x, x, 3, 20, 2, 1, 32, out=torch.empty(3, 20, 2, device="cuda"))
    with pytest.raises(TypeError):
        ops.headdot(x, x.bfloat16(), 3, 20, 2, 1, 32)


# ---- the engines in fp32 against the reference -----------------------------------------------------------------------------------------
def _heads_case():
    fx = load("heads_llama.npz")
    cfg = {k: (float(v) if k in ("rope_theta", "rms_eps") else int(v)) for k, v in zip(fx["cfg_keys"].tolist(), fx["cfg_vals"].tolist())}
    W = ol.random_weights(cfg, seed=int(fx["wseed"]))
    tot = float(W["embed"].double().abs().sum() + W["lm_head"].double().abs().sum())
    for L in W["layers"]:
        tot += sum(float(v.double().abs().sum()) for v in L.values())
    assert abs(tot - float(fx["wsum"])) <= 1e-9 * abs(tot), "synthetic weights did not reproduce"
    return cfg, W, torch.from_numpy(fx["ids"]), fx


def _vs_fixture(tag, out, fx, b=0, cols=slice(None)):
    errs = {n: nmax(out["R_head_" + n][:, b, :, cols], fx[n]) for n in HEADS}
    print(f"[{tag}] vs reference fp64: " + "  ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    return errs


@pytest.mark.parametrize("sparse_top", [True, False])
def test_engine_fp32_heads_vs_reference(mods, sparse_top):
    E, _ = mods
    cfg, W, ids, fx = _heads_case()
    L, S, nq = cfg["n_layers"], int(fx["S"]), cfg["n_heads"]
    eng = E.LlamaLRP(cfg, W, dtype=torch.float32, mode="efficient", max_seq=S, sparse_top=sparse_top)
    out = eng.explain(ids[None], heads=HEADS)
    assert int(out["idx"][0]) == int(fx["idx"])
    for n in HEADS:
        assert out["R_head_" + n].shape == (L, 1, nq, S) and out["R_head_" + n].dtype == torch.float32
    errs = _vs_fixture(f"fp32 heads, sparse_top={sparse_top}", out, fx)
    assert max(errs.values()) <= 1e-4
    assert out["R_head"].shape == (L, 1, nq) and torch.equal(out["R_head"], out["R_head_out"].sum(-1))
    e_v = nmax(out["R_head_v"].sum(-1), 0.5 * out["R_head"])
    print(f"   sum_t R_head_v vs 1/2 R_head {e_v:.2e}")
    assert e_v <= 1e-5
    # above the top layer only the last position is live
    assert not out["R_head_out"][L - 1, :, :, : S - 1].any() and not out["R_head_q"][L - 1, :, :, : S - 1].any()
    # a single name gives that output alone, the same bits
    one = eng.explain(ids[None], heads="k")
    assert torch.equal(one["R_head_k"], out["R_head_k"]) and not any(k.startswith("R_head") and k != "R_head_k" for k in one)


def test_engine_fp32_heads_left_padded_vs_reference(mods):
    """lengths in fp32: the reference's prompt left-padded inside a batch still matches the reference's maps and its pad columns are exactly
    0; a second prompt of another length equals its own un-padded call"""
    E, _ = mods
    cfg, W, ids, fx = _heads_case()
    n, S = int(fx["S"]), int(fx["S"]) + 32
    other = torch.randint(0, cfg["vocab"], (S,), generator=torch.Generator().manual_seed(99))
    batch = torch.stack([torch.cat([torch.zeros(S - n, dtype=ids.dtype), ids]), other])
    eng = E.LlamaLRP(cfg, W, dtype=torch.float32, mode="efficient", max_seq=S)
    out = eng.explain(batch, lengths=[n, S], heads=HEADS)
    assert int(out["idx"][0]) == int(fx["idx"])
    errs = _vs_fixture(f"fp32 heads, left-padded by {S - n}", out, fx, cols=slice(S - n, None))
    assert max(errs.values()) <= 1e-4
    for k in HEADS:
        assert not out["R_head_" + k][:, 0, :, : S - n].any(), k
    alone = eng.explain(other[None], heads=HEADS, target=out["idx"][1:])
    for k in HEADS:
        assert nmax(out["R_head_" + k][:, 1], alone["R_head_" + k][:, 0]) <= 1e-5


def test_qwen3_fp32_heads_vs_reference(mods):
    """QwenLRP on Qwen3: the head norms sit in front of RoPE, the read-out takes the rotated dq (no rotation in the read-out)"""
    from lxt_amd.engine_qwen import QwenLRP
    from tests.golden import hf_models
    fx = load("heads_qwen3.npz")
    model = hf_models.build_qwen3()
    assert abs(hf_models.wsum(model) - float(fx["wsum"])) <= 1e-9 * float(fx["wsum"]), "seeded weights did not reproduce"
    ids = torch.from_numpy(fx["ids"])
    for sparse_top in (True, False):
        eng = QwenLRP.from_hf(model, dtype=torch.float32, max_seq=int(fx["S"]), sparse_top=sparse_top)
        plain = eng.explain(ids[None], layer_relevance=True)
        out = eng.explain(ids[None], layer_relevance=True, heads=HEADS)
        assert int(out["idx"][0]) == int(fx["idx"])
        errs = _vs_fixture(f"fp32 Qwen3 heads, sparse_top={sparse_top}", out, fx)
        assert max(errs.values()) <= 1e-4
        assert torch.equal(out["R_head"], out["R_head_out"].sum(-1)) and nmax(out["R_head_v"].sum(-1), 0.5 * out["R_head"]) <= 1e-5
        for k in ("R_tok", "logit", "idx", "layer_R"):
            assert torch.equal(out[k], plain[k])


def test_engine_fp32_nothing_else_moves(mods):
    E, _ = mods
    cfg, W, ids, _ = _heads_case()
    eng = E.LlamaLRP(cfg, W, dtype=torch.float32, mode="efficient", max_seq=ids.numel())
    for graph in (False, True):
        plain = {k: v.clone() for k, v in eng.explain(ids[None], layer_relevance=True, latent=LATENT, graph=graph).items()}
        out = eng.explain(ids[None], layer_relevance=True, latent=LATENT, heads=HEADS, graph=graph)
        for k in OTHERS:
            assert torch.equal(out[k], plain[k]), (k, graph)
        assert "R_head" not in plain and "R_head_q" in out


# ---- the bf16 engine at the Llama-3-8B layer dimensions -------------------------------------------------------------------------------
CFG8B = dict(hidden=4096, inter=14336, n_layers=2, n_heads=32, n_kv=8, head_dim=128, vocab=4096, rope_theta=5e5, rms_eps=1e-5)


@pytest.fixture(scope="module")
def big(mods):
    E, _ = mods
    H, I, d = 4096, 14336, 128
    g = torch.Generator(device="cuda").manual_seed(3)
    rn = lambda *s: (torch.randn(*s, generator=g, device="cuda") * 0.02).bfloat16()              # noqa: E731
    nw = lambda: (1.0 + 0.1 * torch.randn(H, generator=g, device="cuda")).bfloat16()            # noqa: E731
    W = dict(embed=rn(4096, H), norm=nw(), lm_head=rn(4096, H),
             layers=[dict(ln1=nw(), ln2=nw(), wq=rn(32 * d, H), wk=rn(8 * d, H), wv=rn(8 * d, H), wo=rn(H, 32 * d), wg=rn(I, H), wu=rn(I, H),
                          wd=rn(H, I)) for _ in range(2)])
    bf = E.LlamaLRP(CFG8B, W, dtype=torch.bfloat16, mode="efficient", max_seq=2048)
    f32 = E.LlamaLRP(CFG8B, W, dtype=torch.float32, mode="efficient", max_seq=2048)
    ids = torch.randint(0, 4096, (4, 2048), generator=torch.Generator().manual_seed(4))
    return bf, f32, ids


def test_engine_bf16_8b_heads(mods, big):
    """bf16 against the fp32 engine on the same weights and targets: the fully fused dense layer with the rotated read-out (layer 0) and the
    sparse top layer (layer 1).  The project's bf16 bars, each over a whole [L, B, nq, S] tensor: normalised max <= 5e-2, cosine >= 0.995.
    The four pairs of values are printed; none has been measured yet."""
    bf, f32, ids = big
    B, S, L, nq = 4, 2048, 2, 32
    assert bf._fused(B * S).full and bf.sparse_top
    plain = bf.explain(ids, layer_relevance=True, latent=LATENT)
    out = bf.explain(ids, layer_relevance=True, latent=LATENT, heads=HEADS)
    ref = f32.explain(ids, layer_relevance=True, latent=LATENT, heads=HEADS, target=out["idx"])
    for k in OTHERS:
        assert torch.equal(out[k], plain[k]), k
    res = {n: (nmax(out["R_head_" + n], ref["R_head_" + n]), _cosine(out["R_head_" + n], ref["R_head_" + n])) for n in HEADS}
    print("[bf16 8B dims heads] vs fp32 engine (nmax, cosine): " + "  ".join(f"{n} {e:.2e} {c:.5f}" for n, (e, c) in res.items())
          + f"   [R_trace of the same run {nmax(out['R_trace'], ref['R_trace']):.2e}]")
    per_layer = {n: [f"{nmax(out['R_head_' + n][l], ref['R_head_' + n][l]):.1e}" for l in range(L)] for n in HEADS}
    print(f"   per layer (0: fused layer, rotated read-out; 1: sparse top layer): {per_layer}")
    for n in HEADS:
        t = out["R_head_" + n]
        assert t.shape == (L, B, nq, S) and torch.isfinite(t).all()
        assert res[n][0] <= 5e-2 and res[n][1] >= 0.995, (n, res[n])
    assert torch.equal(out["R_head"], out["R_head_out"].sum(-1))
    assert not out["R_head_out"][L - 1, :, :, : S - 1].any() and not out["R_head_q"][L - 1, :, :, : S - 1].any()


def test_engine_bf16_8b_heads_graph_and_explicit(mods, big):
    bf, _, ids = big
    eager = bf.explain(ids, layer_relevance=True, latent=LATENT, heads=HEADS)
    plain = {k: v.clone() for k, v in bf.explain(ids, layer_relevance=True, latent=LATENT, graph=True).items()}
    for _ in range(2):                                              # capture, then replay
        gr = bf.explain(ids, layer_relevance=True, latent=LATENT, heads=HEADS, graph=True)
        for k in OTHERS + ("R_head",) + tuple("R_head_" + n for n in HEADS):
            assert torch.equal(gr[k], eager[k]), k
        for k in OTHERS:
            assert torch.equal(gr[k], plain[k]), k
    only = bf.explain(ids, heads=["v"], graph=True)                 # another request: another graph
    assert torch.equal(only["R_head_v"], eager["R_head_v"]) and "R_head_q" not in only and "R_head" not in only
    bf.set_mode("explicit")
    try:
        ex = bf.explain(ids, heads=HEADS)
    finally:
        bf.set_mode("efficient")
    for n in HEADS:
        assert torch.isfinite(ex["R_head_" + n]).all() and ex["R_head_" + n].abs().max() > 0


def test_engine_bf16_8b_heads_left_padded(mods, big):
    """lengths at the 8B dims in bf16: pad columns of every map are exactly 0, nothing else changes"""
    bf, _, ids = big
    S = 2048
    lengths = torch.tensor([2048, 1500, 2048, 777])
    plain = bf.explain(ids, layer_relevance=True, lengths=lengths)
    out = bf.explain(ids, layer_relevance=True, lengths=lengths, heads=HEADS)
    for k in ("R_tok", "layer_R", "logit", "idx"):
        assert torch.equal(out[k], plain[k])
    for b, n in enumerate(lengths.tolist()):
        for k in HEADS:
            assert torch.isfinite(out["R_head_" + k][:, b]).all() and not out["R_head_" + k][:, b, :, : S - n].any(), (k, b)
