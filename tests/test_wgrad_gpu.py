"""GPU: per-weight relevance (explain(weights=...)) on the fused Llama / Qwen engines.
  (1) lrp_wgrad_rel against an fp64 torch restatement on the rounded inputs: bf16 / fp32, rs, padded pitches on every operand, the row
      map, accumulate; bitwise repeatable; the predicate's refusals;
  (2) LlamaLRP / QwenLRP in fp32 against tests/golden/weight_relevance_*.npz (the REAL lxt.efficient in fp64,
      make_golden_weight_relevance.py): sparse top layer on and off, folded norm weights on and off (and the two against each other);
  (3) identities that need no fixture -- the column sums of down are R_mlp, the per-head sums of o are R_head_out -- on the fixture model
      and on two layers at the Llama-3-8B dimensions in bf16 (the fully fused layer plus the sparse top layer), there also against the fp32
      engine on the same weights;
  (4) behaviour: a left-padded batch is the sum of its prompts, weights_out accumulates, weight_layers slices, nothing else moves,
      weights=None launches nothing, the MXFP4 engine equals the engine on its dequantised weights."""
import pytest
import torch

from oracle import llama as ol
from tests.util import load, nmax

pytestmark = pytest.mark.gpu

NAMES = ("qkv", "o", "gate_up", "down")
OTHERS = ("R_tok", "logit", "idx", "layer_R", "R_trace", "R_resid", "R_mlp", "R_head_out", "R_head_v")
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import lxt_amd.engine as E
    from lxt_amd import ops
    return E, ops


def _gnmax(a, b):
    """tests.util.nmax on the device (the 8B-dims matrices are too large to compare as fp64 on the host)"""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _cosine(a, b):
    return float(torch.nn.functional.cosine_similarity(a.double().flatten(), b.double().flatten(), dim=0))


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
def _padded(rows, cols, pad, dtype, gen, scale=1.0):
    """a [rows, cols] view of [rows, cols + pad] storage"""
    return (torch.randn(rows, cols + pad, generator=gen, device="cuda") * scale).to(dtype)[:, :cols]


def _problem(dtype, M, N, K, pad, gen):
    v = 16 // dtype.itemsize
    G, X = _padded(M, N, 3 * v * pad, dtype, gen), _padded(M, K, v * pad, dtype, gen)
    W = _padded(N, K, 2 * v * pad, dtype, gen, 0.05)
    rs = torch.rand(M, generator=gen, device="cuda") + 0.5
    return G, X, W, rs


def _ref(G, X, W, rs):
    """-> (fp64 restatement on the rounded inputs, |W| sum_t |G rs X|)"""
    Gd = G.double() * (1.0 if rs is None else rs.double()[:, None])
    return W.double() * (Gd.T @ X.double()), W.double().abs() * (Gd.abs().T @ X.double().abs())


# M, N, K of the issue; every one is on the bf16 kernel's grid of 8 (the refusals are asserted in test_wgrad_rel_refusals), fp32 takes any
# size and gets an odd one on top
SHAPES = [(1, 64, 128), (4, 256, 256), (33, 128, 64), (257, 320, 192)]
COMBOS = [dict(rs=False, pad=0, rmap=False, acc=False), dict(rs=True, pad=1, rmap=True, acc=False),
          dict(rs=True, pad=0, rmap=False, acc=True), dict(rs=False, pad=1, rmap=True, acc=True)]


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("M,N,K", SHAPES + [(33, 130, 67)])
def test_wgrad_rel_vs_fp64(mods, dtype, M, N, K):
    """elementwise bar |W| sum_t |G rs X| (2 M 2^-24 [+ 2^-8 when rs is folded into a bf16 operand]).  accumulate: a second call adds another
    M tokens to the first call's result, which is the one contraction over the 2 M tokens of both -- the bar is that problem's"""
    _, ops = mods
    if dtype == BF16 and (N % 8 or K % 8):
        with pytest.raises(RuntimeError, match="LRP_ESHAPE"):
            ops.wgrad_rel(*_problem(dtype, M, N, K, 0, torch.Generator(device="cuda").manual_seed(1))[:3])
        return
    for ci, c in enumerate(COMBOS):
        gen = torch.Generator(device="cuda").manual_seed(100 * M + N + K + ci)
        G, X, W, rs = _problem(dtype, M, N, K, c["pad"], gen)
        rs = rs if c["rs"] else None
        rmap = torch.randperm(N, generator=gen, device="cuda").to(torch.int32) if c["rmap"] else None
        store = torch.full((N, K + 4 * c["pad"]), float("nan"), device="cuda")
        out = ops.wgrad_rel(G, X, W, out=store[:, :K], rs=rs, row_map=rmap)
        ref, mag = _ref(G, X, W, rs)
        tokens = M
        if c["acc"]:
            G2, X2, _, rs2 = _problem(dtype, M, N, K, c["pad"], gen)
            rs2 = rs2 if c["rs"] else None
            assert ops.wgrad_rel(G2, X2, W, out=out, rs=rs2, row_map=rmap, accumulate=True) is out
            r2, m2 = _ref(G2, X2, W, rs2)
            ref, mag, tokens = ref + r2, mag + m2, 2 * M
        if rmap is not None:
            ref, mag = torch.empty_like(ref).index_copy_(0, rmap.long(), ref), torch.empty_like(mag).index_copy_(0, rmap.long(), mag)
        bar = mag * (2 * tokens * 2.0 ** -24 + (2.0 ** -8 if c["rs"] and dtype == BF16 else 0.0))
        err = (out.double() - ref).abs()
        worst = float((err / bar.clamp_min(1e-300)).max())
        print(f"[wgrad_rel {dtype} M={M} N={N} K={K} {c}] max err / bar {worst:.3f}  normalised max {float(err.max() / ref.abs().max()):.2e}")
        assert out.dtype == F32 and torch.isfinite(out).all() and bool((err <= bar).all()), worst
        if c["pad"]:
            assert torch.isnan(store[:, K:]).all()                      # nothing is written past a row's K columns
        # bitwise repeatable
        again = ops.wgrad_rel(G, X, W, rs=rs, row_map=rmap)
        assert torch.equal(again, ops.wgrad_rel(G, X, W, rs=rs, row_map=rmap))
        if not c["acc"]:
            assert torch.equal(again, out)


def test_wgrad_rel_refusals(mods):
    _, ops = mods
    gen = torch.Generator(device="cuda").manual_seed(0)
    G, X, W, rs = _problem(BF16, 16, 64, 64, 0, gen)
    assert ops.wgrad_rel_ok(16, 64, 64, 64, 64, 64, 64, BF16) and ops.wgrad_rel_ok(1, 3, 5, 3, 5, 5, 5, F32)
    assert not ops.wgrad_rel_ok(16, 60, 64, 64, 64, 64, 64, BF16) and not ops.wgrad_rel_ok(16, 64, 64, 68, 64, 64, 64, BF16)
    with pytest.raises(RuntimeError, match="LRP_ESHAPE"):               # N off the grid of 8
        ops.wgrad_rel(G[:, :60], X, W[:60])
    with pytest.raises(RuntimeError, match="LRP_EALIGN"):               # a row pitch off the 16-byte grid
        ops.wgrad_rel(_padded(16, 64, 4, BF16, gen), X, W)
    with pytest.raises(RuntimeError, match="LRP_EALIGN"):               # a base off the 16-byte grid
        ops.wgrad_rel(G, torch.zeros(16 * 72 + 4, device="cuda", dtype=BF16)[4:].view(16, 72)[:, :64], W)
    with pytest.raises(TypeError):
        ops.wgrad_rel(G, X.float(), W)
    with pytest.raises(ValueError):
        ops.wgrad_rel(G, X, W, accumulate=True)
    with pytest.raises(ValueError):
        ops.wgrad_rel(G, X, W[:32])
    with pytest.raises(ValueError, match="permutation"):
        ops.wgrad_rel(G, X, W, row_map=torch.zeros(64, device="cuda", dtype=torch.int32))
    with pytest.raises(RuntimeError):
        ops.wgrad_rel(G.cpu(), X.cpu(), W.cpu())


# ---- the engines in fp32 against the reference -----------------------------------------------------------------------------------------
def _case():
    fx = load("weight_relevance_llama_prompts.npz")
    cfg = {k: (float(v) if k in ("rope_theta", "rms_eps") else int(v)) for k, v in zip(fx["cfg_keys"].tolist(), fx["cfg_vals"].tolist())}
    W = ol.random_weights(cfg, seed=int(fx["wseed"]))
    tot = float(W["embed"].double().abs().sum() + W["lm_head"].double().abs().sum())
    for L in W["layers"]:
        tot += sum(float(v.double().abs().sum()) for v in L.values())
    assert abs(tot - float(fx["wsum"])) <= 1e-9 * abs(tot), "synthetic weights did not reproduce"
    layers = [load(f"weight_relevance_llama_l{l}.npz") for l in range(cfg["n_layers"])]
    return cfg, W, torch.from_numpy(fx["ids"]), fx, layers


@pytest.fixture(scope="module")
def fp32_runs(mods):
    """the four fp32 engines of the fixture model, each run once on the fixture's two prompts: {(sparse_top, fold_norm): (engine, out)}"""
    E, _ = mods
    cfg, W, ids, fx, _ = _case()
    runs = {}
    for sparse_top in (True, False):
        for fold in (True, False):
            eng = E.LlamaLRP(cfg, W, dtype=F32, mode="efficient", max_seq=ids.shape[1], sparse_top=sparse_top, fold_norm=fold)
            assert eng.folded == fold
            runs[sparse_top, fold] = (eng, eng.explain(ids, weights=NAMES, latent=("mlp",), heads=("out",)))
    return runs


@pytest.mark.parametrize("sparse_top", [True, False])
@pytest.mark.parametrize("fold", [True, False])
def test_engine_fp32_vs_reference(mods, fp32_runs, sparse_top, fold):
    """the bar of the fp32 engine against the fp64 fixtures (test_heads_gpu.py, test_latent_gpu.py): normalised max <= 1e-4"""
    E, _ = mods
    cfg, _, ids, fx, layers = _case()
    eng, out = fp32_runs[sparse_top, fold]
    assert out["idx"].tolist() == fx["idx"].tolist() and out["weight_layers"] == [0, 1, 2]
    shapes = E.weight_shapes(cfg)
    errs = {}
    for n in NAMES:
        assert out["R_W"][n].shape == (3, *shapes[n]) and out["R_W"][n].dtype == F32
        errs[n] = max(nmax(out["R_W"][n][l], layers[l][n]) for l in range(3))
    print(f"[fp32 R_W, sparse_top={sparse_top} fold_norm={fold}] vs reference fp64 (worst layer): " + "  ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert max(errs.values()) <= 1e-4
    # one prompt alone against the per-prompt part of the fixture
    one = eng.explain(ids[1:], weights=NAMES)["R_W"]
    e1 = dict(o=nmax(one["o"], fx["o"][1]), qkv_top=nmax(one["qkv"][2], fx["qkv_top"][1]), down_top=nmax(one["down"][2], fx["down_top"][1]))
    print(f"   prompt 1 alone: {e1}")
    assert max(e1.values()) <= 1e-4


def test_fold_norm_does_not_change_the_weight_relevance(fp32_runs):
    """W diag(gamma) (*) G^T (x / gamma) = W (*) G^T x: the engine with the norm weights folded into the Linears returns the relevance of the
    UNFOLDED weights (fp32 against fp32, two evaluation orders: the bar of the identities below)"""
    for sparse_top in (True, False):
        a, b = fp32_runs[sparse_top, True][1]["R_W"], fp32_runs[sparse_top, False][1]["R_W"]
        errs = {n: _gnmax(a[n], b[n]) for n in NAMES}
        print(f"[fold_norm on vs off, sparse_top={sparse_top}] {errs}")
        assert max(errs.values()) <= 1e-5


def test_qwen3_fp32_vs_reference(mods):
    """QwenLRP inherits the read-out (the q / k head norms sit behind the Linear); the fixture holds layers 0 and 2: weight_layers"""
    from lxt_amd.engine_qwen import QwenLRP
    from tests.golden import hf_models
    fxs = {l: load(f"weight_relevance_qwen3_l{l}.npz") for l in (0, 2)}
    model = hf_models.build_qwen3()
    assert abs(hf_models.wsum(model) - float(fxs[0]["wsum"])) <= 1e-9 * float(fxs[0]["wsum"]), "seeded weights did not reproduce"
    ids = torch.from_numpy(fxs[0]["ids"])
    for sparse_top in (True, False):
        eng = QwenLRP.from_hf(model, dtype=F32, max_seq=ids.shape[1], sparse_top=sparse_top)
        out = eng.explain(ids, weights=NAMES, weight_layers=[0, 2])
        assert out["idx"].tolist() == fxs[0]["idx"].tolist() and out["weight_layers"] == [0, 2]
        errs = {n: max(nmax(out["R_W"][n][i], fxs[l][n]) for i, l in enumerate((0, 2))) for n in NAMES}
        print(f"[fp32 Qwen3 R_W, sparse_top={sparse_top}] vs reference fp64: {errs}")
        assert max(errs.values()) <= 1e-4


# ---- identities ---------------------------------------------------------------------------------------------------------------------
def _identities(out, nq, d):
    """-> (down's column sums vs R_mlp, o's per-head sums vs R_head_out) as (normalised max, cosine)"""
    L = out["R_W"]["down"].shape[0]
    down, mlp = out["R_W"]["down"].sum(1), out["R_mlp"].sum(1)                                  # [L, I]
    o, head = out["R_W"]["o"].sum(1).view(L, nq, d).sum(-1), out["R_head_out"].sum((1, 3))      # [L, nq]
    return (_gnmax(down, mlp), _cosine(down, mlp)), (_gnmax(o, head), _cosine(o, head))


def test_identities_fp32_fixture_model(fp32_runs):
    for key, (eng, out) in fp32_runs.items():
        (e_d, c_d), (e_o, c_o) = _identities(out, eng.cfg["n_heads"], eng.cfg["head_dim"])
        print(f"[identities fp32 sparse_top, fold = {key}] down.sum(0) vs R_mlp {e_d:.2e}   o per head vs R_head_out {e_o:.2e}")
        assert e_d <= 1e-5 and e_o <= 1e-5


CFG8B = dict(hidden=4096, inter=14336, n_layers=2, n_heads=32, n_kv=8, head_dim=128, vocab=4096, rope_theta=5e5, rms_eps=1e-5)


def test_engine_bf16_8b_dims(mods):
    """two layers at the Llama-3-8B dimensions, 12 prompts of S = 256 (3072 rows: the fully fused bf16 layer 0, the sparse top layer 1).  The
    identities, and bf16 against the fp32 engine on the same weights at the project's bf16 bars (test_heads_gpu.py: normalised max <= 5e-2,
    cosine >= 0.995 over a whole tensor).  Measured values: DESIGN.md section 16."""
    E, _ = mods
    H, I, d, B, S = 4096, 14336, 128, 12, 256
    g = torch.Generator(device="cuda").manual_seed(3)
    rn = lambda *s: (torch.randn(*s, generator=g, device="cuda") * 0.02).bfloat16()              # noqa: E731
    nw = lambda: (1.0 + 0.1 * torch.randn(H, generator=g, device="cuda")).bfloat16()            # noqa: E731
    W = dict(embed=rn(4096, H), norm=nw(), lm_head=rn(4096, H),
             layers=[dict(ln1=nw(), ln2=nw(), wq=rn(32 * d, H), wk=rn(8 * d, H), wv=rn(8 * d, H), wo=rn(H, 32 * d), wg=rn(I, H), wu=rn(I, H),
                          wd=rn(H, I)) for _ in range(2)])
    ids = torch.randint(0, 4096, (B, S), generator=torch.Generator().manual_seed(4))
    bf = E.LlamaLRP(CFG8B, W, dtype=BF16, mode="efficient", max_seq=S)
    assert bf._fused(B * S).full and bf.sparse_top and bf.folded
    kw = dict(layer_relevance=True, latent=("trace", "resid", "mlp"), heads=("out", "v"))
    plain = bf.explain(ids, **kw)
    out = bf.explain(ids, weights=NAMES, **kw)
    for k in OTHERS:
        assert torch.equal(out[k], plain[k]), k
    assert "R_W" not in plain
    (e_d, c_d), (e_o, c_o) = _identities(out, 32, d)
    print(f"[bf16 8B dims identities] down.sum(0) vs R_mlp nmax {e_d:.2e} cos {c_d:.5f}   o per head vs R_head_out nmax {e_o:.2e} cos {c_o:.5f}")
    assert e_d <= 5e-2 and c_d >= 0.995 and e_o <= 5e-2 and c_o >= 0.995
    f32 = E.LlamaLRP(CFG8B, W, dtype=F32, mode="efficient", max_seq=S)
    ref = f32.explain(ids, weights=NAMES, target=out["idx"])["R_W"]
    res = {n: (_gnmax(out["R_W"][n], ref[n]), _cosine(out["R_W"][n], ref[n])) for n in NAMES}
    per_layer = {n: [f"{_gnmax(out['R_W'][n][l], ref[n][l]):.1e}" for l in range(2)] for n in NAMES}
    print("[bf16 8B dims R_W] vs fp32 engine (nmax, cosine): " + "  ".join(f"{n} {e:.2e} {c:.5f}" for n, (e, c) in res.items()))
    print(f"   per layer (0: fused layer; 1: sparse top layer): {per_layer}")
    for n in NAMES:
        assert torch.isfinite(out["R_W"][n]).all()
        assert res[n][0] <= 5e-2 and res[n][1] >= 0.995, (n, res[n])


def test_qwen3_bf16_fused_layer_with_head_norms(mods):
    """the fully fused bf16 Qwen3 layer (per-head q / k norms: the qkv read-out sits behind qkv_bwd_pack) against the fp32 engine on the same
    bf16-rounded weights and targets, at the project's bf16 bars (normalised max <= 5e-2, cosine >= 0.995 over a whole tensor)"""
    from lxt_amd.engine_qwen import QwenLRP
    from tests.golden import qwen_models as qm
    model = qm.to_bf16_rotary_fp32(qm.build("qwen3_d128"))
    ids = qm.prompts("qwen3_d128")
    bf = QwenLRP.from_hf(model, max_seq=qm.S)
    assert bf.dtype == BF16 and "qn" in bf.layers[0] and bf._fused(qm.B * qm.S).full
    plain = bf.explain(ids, layer_relevance=True)
    out = bf.explain(ids, layer_relevance=True, weights=NAMES)
    for k in ("R_tok", "logit", "idx", "layer_R"):
        assert torch.equal(out[k], plain[k]), k
    ref = QwenLRP.from_hf(model, dtype=F32, max_seq=qm.S).explain(ids, weights=NAMES, target=out["idx"])["R_W"]
    res = {n: (_gnmax(out["R_W"][n], ref[n]), _cosine(out["R_W"][n], ref[n])) for n in NAMES}
    print("[bf16 Qwen3 d128 fused R_W] vs fp32 engine (nmax, cosine): " + "  ".join(f"{n} {e:.2e} {c:.5f}" for n, (e, c) in res.items()))
    for n in NAMES:
        assert res[n][0] <= 5e-2 and res[n][1] >= 0.995, (n, res[n])


# ---- behaviour ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_left_padded_batch_is_the_sum_of_its_prompts(mods, dtype):
    """fp32: two evaluation orders of the same sums (1e-5, the identities' bar); bf16: the project's bar between two bf16 evaluations of one
    quantity (normalised max 5e-2) -- nothing pins the batched kernels to the single-prompt bits"""
    E, _ = mods
    cfg, W, ids, _, _ = _case()
    S, n1 = ids.shape[1], 30
    eng = E.LlamaLRP(cfg, W, dtype=dtype, mode="efficient", max_seq=S)
    batch = torch.stack([ids[0], torch.cat([torch.zeros(S - n1, dtype=ids.dtype), ids[1, :n1]])])
    out = eng.explain(batch, lengths=[S, n1], weights=NAMES)
    a = eng.explain(ids[:1], weights=NAMES, target=out["idx"][:1])["R_W"]
    b = eng.explain(ids[1:, :n1], weights=NAMES, target=out["idx"][1:])["R_W"]
    errs = {n: _gnmax(out["R_W"][n], a[n] + b[n]) for n in NAMES}
    print(f"[left-padded batch vs the sum of its prompts, {dtype}] {errs}")
    assert max(errs.values()) <= (1e-5 if dtype == F32 else 5e-2)


def test_weights_out_weight_layers_and_nothing_else_moves(mods, monkeypatch):
    E, ops = mods
    cfg, W, ids, _, _ = _case()
    eng = E.LlamaLRP(cfg, W, dtype=BF16, mode="efficient", max_seq=ids.shape[1])
    kw = dict(layer_relevance=True, latent=("trace", "resid", "mlp"), heads=("out", "v"))
    plain = eng.explain(ids, **kw)
    full = eng.explain(ids, weights=NAMES, **kw)
    for k in OTHERS:
        assert torch.equal(full[k], plain[k]), k
    assert "R_W" not in plain and "weight_layers" not in plain
    # weight_layers / a subset of the names: the same bits as the slices of the full result, nothing else
    part = eng.explain(ids, weights=["down", "qkv"], weight_layers=[0, 2])
    assert part["weight_layers"] == [0, 2] and set(part["R_W"]) == {"down", "qkv"}
    for n in ("down", "qkv"):
        assert torch.equal(part["R_W"][n], full["R_W"][n][[0, 2]]), n
    # weights_out: two calls accumulate in place into the first call's tensors
    r0, r1 = eng.explain(ids[:1], weights=NAMES)["R_W"], eng.explain(ids[1:], weights=NAMES)["R_W"]
    acc = {n: t.clone() for n, t in r0.items()}
    res = eng.explain(ids[1:], weights=NAMES, weights_out=acc)
    for n in NAMES:
        assert res["R_W"][n] is acc[n] and torch.equal(acc[n], r0[n] + r1[n]), n
    with pytest.raises(ValueError):
        eng.explain(ids, weights=NAMES, weights_out=dict(acc, o=acc["o"][:1]))
    with pytest.raises(ValueError):
        eng.explain(ids, weights=NAMES, graph=True)
    eng.set_mode("explicit")
    try:
        with pytest.raises(ValueError):
            eng.explain(ids, weights=NAMES)
    finally:
        eng.set_mode("efficient")
    # weights=None launches nothing

    def boom(*a, **k):
        raise AssertionError("wgrad_rel launched without a request")
    monkeypatch.setattr(ops, "wgrad_rel", boom)
    again = eng.explain(ids, **kw)
    for k in OTHERS:
        assert torch.equal(again[k], plain[k]), k
    with pytest.raises(AssertionError):
        eng.explain(ids, weights="o")


def test_mxfp4_engine_equals_the_engine_on_its_dequantised_weights(mods):
    E, _ = mods
    cfg, W, ids, _, _ = _case()
    q = E.LlamaLRP(cfg, W, dtype=BF16, max_seq=ids.shape[1], weight_format="mxfp4")
    plain = E.LlamaLRP(*q.dequantized_weights(), dtype=BF16, max_seq=ids.shape[1])
    a, b = q.explain(ids, weights=NAMES), plain.explain(ids, weights=NAMES)
    assert torch.equal(a["R_tok"], b["R_tok"])
    for n in NAMES:
        assert torch.equal(a["R_W"][n], b["R_W"][n]), n
