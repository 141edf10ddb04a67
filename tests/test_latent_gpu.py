"""GPU: latent feature attribution (docs/source/latent-feature-attribution-efficient.rst of the reference) on the fused Llama engine.
  (1) lrp_colsum_dot against an fp64 torch restatement: bf16 / fp32, odd N, padded pitches, S off the chunk grid, B = 1 and 5; bitwise
      repeatable and batch invariant;
  (2) LlamaLRP.explain(latent=...) in fp32 against tests/golden/latent_llama.npz (the REAL lxt.efficient in fp64, make_golden_latent.py);
  (3) the bf16 engine at the Llama-3-8B layer dimensions against the fp32 engine on the same weights: the fully fused dense layer, the
      sparse top layer, left-padded prompts, hipGraph replay and the explicit placement."""
import pytest
import torch

from oracle import llama as ol
from tests.util import load, nmax

pytestmark = pytest.mark.gpu

ALL = ("trace", "resid", "mlp")


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import lxt_amd.engine as E
    from lxt_amd import ops
    return E, ops


def _ref(x, g, B, S):
    return (x.double() * g.double()).view(B, S, -1).sum(1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,S,N,padx,padg", [(1, 64, 4096, 0, 0), (5, 130, 333, 11, 3), (5, 200, 1000, 64, 0), (1, 1, 17, 7, 0),
                                             (5, 1, 4096, 0, 8), (2, 2047, 14336, 64, 128)])
def test_colsum_dot_vs_fp64(mods, dtype, B, S, N, padx, padg):
    _, ops = mods
    v = 16 // dtype.itemsize
    ldx, ldg = -(-(N + padx) // v) * v, -(-(N + padg) // v) * v           # padded pitches, multiples of 16 bytes
    gen = torch.Generator(device="cuda").manual_seed(N + S)
    xs = torch.randn(B * S, ldx, generator=gen, device="cuda").to(dtype)
    gs = torch.randn(B * S, ldg, generator=gen, device="cuda").to(dtype)
    x, g = xs[:, :N], gs[:, :N]
    out = ops.colsum_dot(x, g, B, S)
    ref = _ref(x, g, B, S)
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    print(f"[colsum_dot {dtype} B={B} S={S} N={N} ld=({ldx},{ldg})] normalised max err vs fp64 {err:.2e}")
    assert out.shape == (B, N) and out.dtype == torch.float32 and err <= 1e-5
    # bitwise repeatable, and a prompt's result does not depend on its neighbours: alone (a view of its rows, and a copy) == inside the batch
    assert torch.equal(ops.colsum_dot(x, g, B, S), out)
    for b in {0, B - 1}:
        one = ops.colsum_dot(x[b * S:(b + 1) * S], g[b * S:(b + 1) * S], 1, S)
        cp = ops.colsum_dot(xs[b * S:(b + 1) * S].clone()[:, :N], gs[b * S:(b + 1) * S].clone()[:, :N], 1, S)      # (fresh memory, same pitch)
        assert torch.equal(one[0], out[b]) and torch.equal(cp[0], out[b])


def test_colsum_dot_caller_workspace(mods):
    _, ops = mods
    import lxt_amd._lib as L
    x = torch.randn(3 * 300, 520, device="cuda")
    need = L.lib.lrp_colsum_dot_ws(3, 300, 520)
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    out = torch.full((3, 520), float("nan"), device="cuda")
    assert ops.colsum_dot(x, x, 3, 300, out=out, ws=ws) is out
    assert torch.equal(out, ops.colsum_dot(x, x, 3, 300))
    with pytest.raises(ValueError):
        ops.colsum_dot(x, x, 3, 300, ws=ws[: need - 4])
    with pytest.raises(RuntimeError, match="LRP_ESHAPE"):
        ops.colsum_dot(x, x, 4, 300)                                     # B S != rows


# ---- the engine in fp32 against the reference ----------------------------------------------------------------------------------------
def _latent_case():
    fx = load("latent_llama.npz")
    cfg = {k: (float(v) if k in ("rope_theta", "rms_eps") else int(v)) for k, v in zip(fx["cfg_keys"].tolist(), fx["cfg_vals"].tolist())}
    W = ol.random_weights(cfg, seed=int(fx["wseed"]))
    tot = float(W["embed"].double().abs().sum() + W["lm_head"].double().abs().sum())
    for L in W["layers"]:
        tot += sum(float(v.double().abs().sum()) for v in L.values())
    assert abs(tot - float(fx["wsum"])) <= 1e-9 * abs(tot), "synthetic weights did not reproduce"
    return cfg, W, torch.from_numpy(fx["ids"]), fx


@pytest.mark.parametrize("sparse_top", [True, False])
def test_engine_fp32_latent_vs_reference(mods, sparse_top):
    E, _ = mods
    cfg, W, ids, fx = _latent_case()
    L, S = cfg["n_layers"], int(fx["S"])
    eng = E.LlamaLRP(cfg, W, dtype=torch.float32, mode="efficient", max_seq=S, sparse_top=sparse_top)
    plain = eng.explain(ids[None], layer_relevance=True)
    out = eng.explain(ids[None], layer_relevance=True, latent=ALL)
    assert int(out["idx"][0]) == int(fx["idx"])
    assert out["R_trace"].shape == (L + 1, 1, S) and out["R_resid"].shape == (L + 1, 1, cfg["hidden"])
    assert out["R_mlp"].shape == (L, 1, cfg["inter"])
    e_tr, e_rs, e_ml = (nmax(out[k][:, 0], fx[f]) for k, f in (("R_trace", "trace"), ("R_resid", "resid"), ("R_mlp", "mlp")))
    per_layer = [nmax(out["R_mlp"][l, 0], fx["mlp"][l]) for l in range(L)]
    print(f"[fp32 latent, sparse_top={sparse_top}] vs reference fp64: trace {e_tr:.2e} resid {e_rs:.2e} mlp {e_ml:.2e} "
          f"(mlp per layer {[f'{e:.1e}' for e in per_layer]})")
    assert e_tr <= 1e-4 and e_rs <= 1e-4 and e_ml <= 1e-4
    # the trace IS the per-token rows layer_R sums; the residual read-out sums to it to fp32 rounding
    for l in range(L + 1):
        assert torch.equal(out["R_trace"][l].sum(-1), out["layer_R"][l])
    assert torch.equal(out["R_trace"][0], out["R_tok"])
    assert not out["R_trace"][L, :, : S - 1].any()
    assert nmax(out["R_resid"].sum(-1), out["layer_R"]) < 1e-5
    # nothing else changes with the request
    for k in ("R_tok", "layer_R", "logit", "idx"):
        assert torch.equal(out[k], plain[k])


# ---- the bf16 engine at the Llama-3-8B layer dimensions -----------------------------------------------------------------------------
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


def test_engine_bf16_8b_latent(mods, big):
    """bf16 against the fp32 engine on the same weights: the fully fused dense layer (layer 0) and the sparse top layer (layer 1)"""
    bf, f32, ids = big
    B, S, L = 4, 2048, 2
    assert bf._fused(B * S).full and bf.sparse_top
    plain = bf.explain(ids, layer_relevance=True)
    out = bf.explain(ids, layer_relevance=True, latent=ALL)
    ref = f32.explain(ids, layer_relevance=True, latent=ALL, target=out["idx"])
    for k in ("R_tok", "layer_R", "logit", "idx"):
        assert torch.equal(out[k], plain[k])
    errs = {k: nmax(out[k], ref[k]) for k in ("R_tok", "R_trace", "R_resid", "R_mlp")}
    print("[bf16 8B dims] vs fp32 engine: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k in ("R_trace", "R_resid", "R_mlp"):                       # the bf16 engine's bar on R_tok (test_engine_gpu.py::test_llama_bf16)
        assert torch.isfinite(out[k]).all() and errs[k] <= 5e-2
    for l in range(L + 1):
        assert torch.equal(out["R_trace"][l].sum(-1), out["layer_R"][l])
    assert torch.equal(out["R_trace"][0], out["R_tok"])


def test_engine_fp32_latent_left_padded_vs_reference(mods):
    """lengths in fp32: the reference's prompt left-padded inside a batch still matches the reference's read-outs, its pad rows are exactly 0,
    and a second prompt of another length equals its own un-padded call"""
    E, _ = mods
    cfg, W, ids, fx = _latent_case()
    L, n, S = cfg["n_layers"], int(fx["S"]), int(fx["S"]) + 32
    other = torch.randint(0, cfg["vocab"], (S,), generator=torch.Generator().manual_seed(99))
    batch = torch.stack([torch.cat([torch.zeros(S - n, dtype=ids.dtype), ids]), other])
    eng = E.LlamaLRP(cfg, W, dtype=torch.float32, mode="efficient", max_seq=S)
    out = eng.explain(batch, lengths=[n, S], layer_relevance=True, latent=ALL)
    assert int(out["idx"][0]) == int(fx["idx"])
    tr = out["R_trace"][:, 0, S - n:]
    e = [nmax(tr, fx["trace"]), nmax(out["R_resid"][:, 0], fx["resid"]), nmax(out["R_mlp"][:, 0], fx["mlp"])]
    print(f"[fp32 latent, left-padded by {S - n}] vs reference fp64: trace {e[0]:.2e} resid {e[1]:.2e} mlp {e[2]:.2e}")
    assert max(e) <= 1e-4 and not out["R_trace"][:, 0, : S - n].any()
    alone = eng.explain(other[None], latent=ALL, target=out["idx"][1:])
    for k in ("R_trace", "R_resid", "R_mlp"):
        assert nmax(out[k][:, 1], alone[k][:, 0]) <= 1e-5
    for l in range(L + 1):
        assert torch.equal(out["R_trace"][l].sum(-1), out["layer_R"][l])


def test_engine_bf16_8b_latent_left_padded(mods, big):
    """lengths at the 8B dims in bf16: pad rows carry no gradient (trace entries exactly 0), nothing else changes, and the padded batch
    against the fp32 engine's padded batch"""
    bf, f32, ids = big
    S = 2048
    lengths = torch.tensor([2048, 1500, 2048, 777])
    plain = bf.explain(ids, layer_relevance=True, lengths=lengths)
    out = bf.explain(ids, layer_relevance=True, lengths=lengths, latent=ALL)
    ref = f32.explain(ids, layer_relevance=True, lengths=lengths, latent=ALL, target=out["idx"])
    for k in ("R_tok", "layer_R", "logit", "idx"):
        assert torch.equal(out[k], plain[k])
    for b, n in enumerate(lengths.tolist()):
        assert not out["R_trace"][:, b, : S - n].any() and not ref["R_trace"][:, b, : S - n].any()
    cos = lambda a, b: float(torch.nn.functional.cosine_similarity(a.double().flatten(), b.double().flatten(), dim=0))   # noqa: E731
    errs = {k: (nmax(out[k], ref[k]), cos(out[k], ref[k])) for k in ("R_tok", "R_trace", "R_resid", "R_mlp")}
    print("[bf16 8B dims, lengths] vs fp32 engine (nmax, cosine): " + "  ".join(f"{k} {e:.2e} {c:.5f}" for k, (e, c) in errs.items()))
    # per token within the bf16 bar.  A prompt left-padded to S (RoPE positions up to S - 1) has R_tok itself 3x further from fp32 than the
    # same prompt alone (measured: 9.3e-3 vs 3.0e-3 at length 777); the token SUMS cancel and scale that up again:
    # bounded by direction and by 3x the bar
    assert errs["R_trace"][0] <= 5e-2
    for k in ("R_resid", "R_mlp"):
        assert torch.isfinite(out[k]).all() and errs[k][1] >= 0.995 and errs[k][0] <= 1.5e-1


def test_engine_bf16_8b_latent_graph_and_explicit(mods, big):
    E, _ = mods
    bf, _, ids = big
    L = 2
    eager = bf.explain(ids, layer_relevance=True, latent=ALL)
    for _ in range(2):                                              # capture, then replay
        gr = bf.explain(ids, layer_relevance=True, latent=ALL, graph=True)
        for k in ("R_tok", "layer_R", "R_trace", "R_resid", "R_mlp"):
            assert torch.equal(gr[k], eager[k]), k
    only = bf.explain(ids, latent=["resid"], graph=True)            # another request: another graph
    assert torch.equal(only["R_resid"], eager["R_resid"]) and "R_mlp" not in only and "R_trace" not in only
    bf.set_mode("explicit")
    try:
        ex = bf.explain(ids, layer_relevance=True, latent=ALL)
    finally:
        bf.set_mode("efficient")
    for k in ("R_trace", "R_resid", "R_mlp"):
        assert torch.isfinite(ex[k]).all() and ex[k].abs().max() > 0
    # index l >= 1: the very rows layer_R sums; index 0 is R_tok, which reads the bf16-rounded G where the norm's kernel sums the fp32 one
    for l in range(1, L + 1):
        assert torch.equal(ex["R_trace"][l].sum(-1), ex["layer_R"][l])
    assert torch.equal(ex["R_trace"][0], ex["R_tok"]) and nmax(ex["R_trace"][0].sum(-1), ex["layer_R"][0]) < 2e-2
