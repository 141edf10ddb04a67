"""GPU: answer-span attribution, explain(positions=..., position_weights=..., objective=..., per_position=...) on the fused drivers.
  (i)   the fp32 engines (LlamaLRP, QwenLRP, Qwen3MoeLRP) against tests/golden/span_*.npz -- the REAL lxt.efficient in fp64
        (make_golden_span.py): scattered positions with both objectives, a left-padded batch with zero-weight fill, single positions;
  (ii)  positions=[[S - 1]] on a dense-top engine IS the plain call, bitwise;
  (iii) linearity on the device: the joint call against the weighted sum of single-position calls;
  (iv)  exact zeros above the highest explained row and at pads; a one-hot weight vector against the single-position call;
  (v)   per_position=True: every row of the answer x prompt map against its single-position call, the sum against the joint call, and the
        plain call before and after it, bitwise;
  (vi)  bf16 at the Llama-3-8B layer widths on the fully fused layer against the fp32 engine, measured against the plain call's own error;
  (vii) the refusals raise before the forward runs."""
import pytest
import torch

from oracle import llama as ol
from tests.util import load, nmax

pytestmark = pytest.mark.gpu

MODELS = ("llama", "qwen3", "qwen3_moe")


@pytest.fixture(scope="module")
def engines():
    """{model: (fp32 engine, fixture)}, built once (sparse_top as the class defaults it: a span call must not use it)"""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import lxt_amd.engine as E
    from lxt_amd.engine_qwen import QwenLRP
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    from tests.golden import make_golden_latent as gl
    from tests.golden import moe_engine_models, qwen_models
    fx = {m: load(f"span_{m}.npz") for m in MODELS}
    S = int(fx["llama"]["S"])
    W = ol.random_weights(gl.CFG, seed=gl.WSEED)
    qwen, moe = qwen_models.build("qwen3_d128"), moe_engine_models.build()
    for got, m in ((gl.wsum(W), "llama"), (qwen_models.wsum(qwen), "qwen3"), (qwen_models.wsum(moe), "qwen3_moe")):
        assert abs(got - float(fx[m]["wsum"])) <= 1e-9 * got, f"seeded weights of {m} did not reproduce"
    eng = dict(llama=E.LlamaLRP(gl.CFG, W, dtype=torch.float32, mode="efficient", max_seq=S),
               qwen3=QwenLRP.from_hf(qwen, dtype=torch.float32, max_seq=S),
               qwen3_moe=Qwen3MoeLRP.from_hf(moe, dtype=torch.float32, max_seq=S))
    assert eng["llama"].sparse_top and eng["qwen3"].sparse_top
    return {m: (eng[m], fx[m]) for m in MODELS}


def case(fx, key, t=None):
    """the arguments of one fixture case (t: row t of the stacked case d) and its expected arrays; targets are left to the default rule"""
    g = lambda k: fx[f"{key}/{k}"] if t is None else fx[f"{key}/{k}"][t]          # noqa: E731
    ids, lengths = torch.from_numpy(g("ids")), g("lengths").tolist()
    kw = dict(positions=torch.from_numpy(g("positions")), position_weights=torch.from_numpy(g("weights")).float(), objective=str(g("objective")))
    if min(lengths) < ids.shape[1]:
        kw["lengths"] = lengths
    return ids, kw, {k: g(k) for k in ("target", "logit", "logprob", "R_tok", "layer_R")}


@pytest.mark.parametrize("key", ["a", "b", "c", "d"])
@pytest.mark.parametrize("model", MODELS)
def test_fp32_engines_vs_reference(engines, model, key):
    eng, fx = engines[model]
    for t in (range(fx["d/ids"].shape[0]) if key == "d" else (None,)):
        ids, kw, want = case(fx, key, t)
        heads = ("out",) if (model, key) == ("llama", "a") else None
        out = eng.explain(ids, layer_relevance=True, heads=heads, **kw)
        assert "logits" not in out and out["idx"].cpu().tolist() == want["target"].tolist()          # next token; arg-max at S - 1
        errs = {k: nmax(out[k], want[k]) for k in ("R_tok", "logit", "logprob", "layer_R")}
        if heads:
            errs["R_head_out"] = nmax(out["R_head_out"], fx["a/R_head_out"])
        print(f"[fp32 {model} case {key}{'' if t is None else t}] vs reference fp64: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert max(errs.values()) <= 1e-4
        # exactly 0 at pads and above the highest explained row (a zero-weight slot counts: its row is explained, with seed 0)
        S = ids.shape[1]
        for b in range(ids.shape[0]):
            first = S - kw["lengths"][b] if "lengths" in kw else 0
            assert not out["R_tok"][b, :first].any() and not out["R_tok"][b, int(kw["positions"][b].max()) + 1:].any()


def test_last_position_is_the_plain_call(engines):
    """(ii) on engines with a dense top layer the two calls launch the same kernels on the same values"""
    import lxt_amd.engine as E
    from tests.golden import make_golden_latent as gl
    fx = engines["llama"][1]
    ids, S = torch.from_numpy(fx["a/ids"]), int(fx["S"])
    dense = E.LlamaLRP(gl.CFG, ol.random_weights(gl.CFG, seed=gl.WSEED), dtype=torch.float32, mode="efficient", max_seq=S, sparse_top=False)
    for eng in (dense, engines["qwen3_moe"][0]):          # (Qwen3MoeLRP is always dense there)
        ids_e = ids % eng.cfg["vocab"]
        plain = eng.explain(ids_e, layer_relevance=True)
        span = eng.explain(ids_e, positions=[[S - 1]], layer_relevance=True)
        assert torch.equal(span["R_tok"], plain["R_tok"]) and torch.equal(span["logit"][:, 0], plain["logit"])
        assert torch.equal(span["idx"][:, 0], plain["idx"]) and torch.equal(span["layer_R"], plain["layer_R"])
        lp = torch.log_softmax(plain["logits"].double(), -1).gather(1, plain["idx"].long()[:, None])
        assert nmax(span["logprob"], lp) <= 1e-5


@pytest.mark.parametrize("objective", ["logit", "logprob"])
@pytest.mark.parametrize("model", MODELS)
def test_linearity_zeros_and_per_position(engines, model, objective):
    """(iii), (iv), (v) on one left-padded batch of two prompts, T = 4 with a zero and a negative weight"""
    eng, fx = engines[model]
    ids, S = torch.from_numpy(fx["c/ids"]), int(fx["S"])
    lengths = fx["c/lengths"].tolist()
    pos = torch.tensor([[30, 3, 40, 11], [25, 44, 18, 31]])
    w = torch.tensor([[1.0, -0.5, 0.0, 2.0], [0.25, 1.0, 1.5, 0.0]])
    B, T = pos.shape
    kw = dict(lengths=lengths, objective=objective)
    before = eng.explain(ids, lengths=lengths, layer_relevance=True)
    joint = eng.explain(ids, positions=pos, position_weights=w, layer_relevance=True, latent=("trace", "resid"), **kw)
    tgt = joint["idx"]
    single = [eng.explain(ids, positions=pos[:, t: t + 1], target=tgt[:, t: t + 1], layer_relevance=True, **kw) for t in range(T)]
    # (iii) linearity: R_tok and layer_R of the joint call are the weighted sums of the single-position calls
    for k, wt in (("R_tok", lambda t: w[:, t].cuda()[:, None]), ("layer_R", lambda t: w[:, t].cuda()[None])):
        e = nmax(joint[k], sum(wt(t) * single[t][k].double() for t in range(T)))
        print(f"[{model} {objective}] joint vs weighted sum of single-position calls: {k} {e:.2e}")
        assert e <= 1e-5
    assert all(torch.equal(joint["idx"][:, t], single[t]["idx"][:, 0]) and nmax(joint["logit"][:, t], single[t]["logit"][:, 0]) <= 1e-6 for t in range(T))
    # the read-outs see the explained columns: the head's rows of the trace are non-zero exactly there (zero-weight slots: exactly 0)
    L = len(eng.layers)
    live = torch.zeros(B, S, dtype=torch.bool).scatter_(1, pos, w != 0).cuda()
    assert torch.equal(joint["R_trace"][L] != 0, live) and torch.equal(joint["R_trace"][L].sum(-1), joint["layer_R"][L])
    assert nmax(joint["R_resid"][L].sum(-1), joint["layer_R"][L]) <= 1e-5
    # (iv) exact zeros: pads, and every column above the highest explained row
    for b in range(B):
        assert not joint["R_tok"][b, : S - lengths[b]].any() and not joint["R_tok"][b, int(pos[b].max()) + 1:].any()
        assert joint["R_tok"][b, S - lengths[b]: int(pos[b].max()) + 1].any()
    for t in (1, 2):          # a call whose only non-zero weight is slot t against the single-position call of slot t
        hot = torch.zeros(B, T)
        hot[:, t] = 1.0
        one = eng.explain(ids, positions=pos, position_weights=hot, target=tgt, **kw)
        assert nmax(one["R_tok"], single[t]["R_tok"]) <= 1e-5
    # (v) per_position: T backward passes over one forward.  "logit": the seed is a row of the LM head times w rstd, which no other row of
    # the call enters, and the rows of the other slots are exactly 0 -- the dense gradient is the single-position call's, so the map is
    # BITWISE that call.  "logprob": the seed reads the logits, which the LM-head GEMM forms in another kernel at another row count (B T
    # rows against B): equal to rounding only
    each = eng.explain(ids, positions=pos, position_weights=torch.ones(B, T), target=tgt, per_position=True, **kw)
    assert each["R_tok_each"].shape == (B, T, S) and torch.equal(each["R_tok"], each["R_tok_each"].sum(1))
    for t in range(T):
        if objective == "logit":
            assert torch.equal(each["R_tok_each"][:, t], single[t]["R_tok"]), t
        else:
            assert nmax(each["R_tok_each"][:, t], single[t]["R_tok"]) <= 1e-5
    ones = eng.explain(ids, positions=pos, target=tgt, **kw)
    assert nmax(each["R_tok"], ones["R_tok"]) <= 1e-5 and torch.equal(each["logit"], ones["logit"]) and torch.equal(each["logprob"], ones["logprob"])
    after = eng.explain(ids, lengths=lengths, layer_relevance=True)          # the stash and the arena are not disturbed
    assert all(torch.equal(after[k], before[k]) for k in ("R_tok", "logit", "idx", "layer_R", "logits"))
    with pytest.raises(ValueError):
        eng.explain(ids, positions=pos, per_position=True, layer_relevance=True, **kw)


def test_refusals_launch_nothing(engines, monkeypatch):
    """(vii) every refusal is raised before the forward runs, on all three drivers"""
    for model in MODELS:
        eng, fx = engines[model]
        ids, S, V = torch.from_numpy(fx["a/ids"]), int(fx["S"]), eng.cfg["vocab"]

        def forward(*a, **k):
            raise AssertionError("the forward ran")

        monkeypatch.setattr(eng, "forward", forward)
        for kw in (dict(positions=[[3, 3]]), dict(positions=[[S]]), dict(positions=[[-1]]), dict(positions=[3]), dict(positions=[[3], [4]]),
                   dict(positions=[[3, 4]], position_weights=[[1.0]]), dict(positions=[[3, 4]], target=[[1, V]]),
                   dict(positions=[[3, 4]], target=[1]), dict(positions=[[3]], objective="prob"),
                   dict(positions=[[3]], seed=torch.zeros(1, V)), dict(positions=[[3]], graph=True),
                   dict(positions=[[0, 3]], lengths=[S - 1]), dict(positions=[[3]], per_position=True, layer_relevance=True),
                   dict(position_weights=[[1.0]]), dict(per_position=True), dict(objective="logprob")):
            with pytest.raises(ValueError):
                eng.explain(ids, **kw)
        with pytest.raises(ValueError):
            eng.explain(inputs_embeds=torch.zeros(1, S, eng.cfg["hidden"]), positions=[[3]])
        monkeypatch.undo()
    eng = engines["llama"][0]
    eng.set_mode("explicit")
    try:
        monkeypatch.setattr(eng, "forward", forward)
        with pytest.raises(ValueError):
            eng.explain(ids, positions=[[3]])
    finally:
        monkeypatch.undo()
        eng.set_mode("efficient")


# ---- (vi) the bf16 engine at the Llama-3-8B layer widths ---------------------------------------------------------------------------------
CFG8B = dict(hidden=4096, inter=14336, n_layers=2, n_heads=32, n_kv=8, head_dim=128, vocab=4096, rope_theta=5e5, rms_eps=1e-5)


def test_bf16_8b_widths_fused_layer():
    """bf16 span explanation on the fully fused layer against the fp32 engine on the same weights.  Yardstick: the error of the PLAIN
    last-position bf16 call against fp32, measured here; the span call may be 3 x as far, and must point the same way (cosine >= 0.995)"""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import lxt_amd.engine as E
    H, I, d = 4096, 14336, 128
    g = torch.Generator(device="cuda").manual_seed(3)
    rn = lambda *s: (torch.randn(*s, generator=g, device="cuda") * 0.02).bfloat16()              # noqa: E731
    nw = lambda: (1.0 + 0.1 * torch.randn(H, generator=g, device="cuda")).bfloat16()            # noqa: E731
    W = dict(embed=rn(4096, H), norm=nw(), lm_head=rn(4096, H),
             layers=[dict(ln1=nw(), ln2=nw(), wq=rn(32 * d, H), wk=rn(8 * d, H), wv=rn(8 * d, H), wo=rn(H, 32 * d), wg=rn(I, H), wu=rn(I, H),
                          wd=rn(H, I)) for _ in range(2)])
    bf = E.LlamaLRP(CFG8B, W, dtype=torch.bfloat16, mode="efficient", max_seq=2048)
    f32 = E.LlamaLRP(CFG8B, W, dtype=torch.float32, mode="efficient", max_seq=2048)
    # the smallest (B, S) at which every part of the fused layer applies, read from fused_layer_ok itself
    shapes = sorted(((b, s) for s in (512, 1024, 2048) for b in (1, 2, 3, 4)), key=lambda bs: (bs[0] * bs[1], bs[0]))
    B, S = next(bs for bs in shapes if bf._fused(bs[0] * bs[1]).full)
    ids = torch.randint(0, 4096, (B, S), generator=torch.Generator().manual_seed(4))
    T = 8
    pos = torch.stack([torch.randperm(S - 64, generator=torch.Generator().manual_seed(5 + b))[:T] for b in range(B)])          # (distinct, below S - 64)
    cos = lambda a, b: float(torch.nn.functional.cosine_similarity(a.double().flatten(), b.double().flatten(), dim=0))   # noqa: E731
    plain = bf.explain(ids)
    yard = nmax(plain["R_tok"], f32.explain(ids, target=plain["idx"])["R_tok"])
    for objective in ("logit", "logprob"):
        out = bf.explain(ids, positions=pos, objective=objective, layer_relevance=True)
        ref = f32.explain(ids, positions=pos, objective=objective, layer_relevance=True, target=out["idx"])
        e, c = nmax(out["R_tok"], ref["R_tok"]), cos(out["R_tok"], ref["R_tok"])
        print(f"[bf16 8B widths B={B} S={S} T={T} {objective}] R_tok vs fp32 engine {e:.2e} cosine {c:.5f}; plain last-position call {yard:.2e}; "
              f"logprob {nmax(out['logprob'], ref['logprob']):.2e}")
        assert torch.isfinite(out["R_tok"]).all() and e <= 3 * yard and c >= 0.995
        for b in range(B):
            assert not out["R_tok"][b, int(pos[b].max()) + 1:].any()
    assert torch.equal(bf.explain(ids)["R_tok"], plain["R_tok"])
