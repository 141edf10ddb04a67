"""GPU: answer-span attribution on Gemma3LRP, explain(positions=..., position_weights=..., objective=..., per_position=...) (DESIGN.md
section 23), with the checks tests/test_span_gpu.py makes on the Llama-family drivers:
  (i)   the fp32 engine against tests/golden/span_gemma3.npz -- the REAL lxt.efficient in fp64 (make_golden_span_gemma3.py), cases a - d at
        S = 48 with a window of 32: explained positions on both sides of the window; case a equals the sum of case d's rows;
  (ii)  positions=[[S - 1]] on a dense-top engine IS the plain call, bitwise; self.sparse_top is left as the user set it;
  (iii) linearity on the device, exact zeros, one-hot weights, per_position rows against single-position calls, the plain call before and
        after, and the read-out identities with a span;
  (iv)  the refusals raise before the forward runs."""
import pytest
import torch

from tests.util import load, nmax

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gemma():
    """(fp32 engine with the sparse top layer as the class defaults it, fixture, the seeded HF model)"""
    from lxt_amd.engine_gemma3 import Gemma3LRP
    from tests.golden.hf_models import wsum
    from tests.golden.make_golden_generate_gemma3 import build
    fx, model = load("span_gemma3.npz"), build()
    got = wsum(model)
    assert abs(got - float(fx["wsum"])) <= 1e-9 * got, "the seeded weights did not reproduce"
    eng = Gemma3LRP.from_hf(model, dtype=torch.float32, max_seq=int(fx["S"]))
    assert eng.sparse_top and eng.cfg["window"] == int(fx["window"]) < int(fx["S"])
    return eng, fx, model


def case(fx, key, t=None):
    g = lambda k: fx[f"{key}/{k}"] if t is None else fx[f"{key}/{k}"][t]          # noqa: E731
    ids, lengths = torch.from_numpy(g("ids")), g("lengths").tolist()
    kw = dict(positions=torch.from_numpy(g("positions")), position_weights=torch.from_numpy(g("weights")).float(), objective=str(g("objective")))
    if min(lengths) < ids.shape[1]:
        kw["lengths"] = lengths
    return ids, kw, {k: g(k) for k in ("target", "logit", "logprob", "R_tok", "layer_R")}


@pytest.mark.parametrize("key", ["a", "b", "c", "d"])
def test_fp32_engine_vs_reference(gemma, key):
    eng, fx, _ = gemma
    rows = []
    for t in (range(fx["d/ids"].shape[0]) if key == "d" else (None,)):
        ids, kw, want = case(fx, key, t)
        out = eng.explain(ids, layer_relevance=True, **kw)
        assert "logits" not in out and out["idx"].cpu().tolist() == want["target"].tolist()          # next token; arg-max at S - 1
        errs = {k: nmax(out[k], want[k]) for k in ("R_tok", "logit", "logprob", "layer_R")}
        print(f"[fp32 gemma3 case {key}{'' if t is None else t}] vs reference fp64: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert max(errs.values()) <= 1e-4
        S = ids.shape[1]
        for b in range(ids.shape[0]):
            first = S - kw["lengths"][b] if "lengths" in kw else 0
            assert not out["R_tok"][b, :first].any() and not out["R_tok"][b, int(kw["positions"][b].max()) + 1:].any()
        rows.append(out["R_tok"].double())
    if key == "d":          # case a (weights 1, objective logit) is the sum of its single positions
        ids, kw, _ = case(fx, "a")
        joint = eng.explain(ids, **kw)
        e = nmax(joint["R_tok"], sum(rows))
        print(f"[fp32 gemma3] case a vs the sum of case d's rows: {e:.2e}")
        assert e <= 1e-5
    assert eng.sparse_top


def test_last_position_is_the_plain_call(gemma):
    from lxt_amd.engine_gemma3 import Gemma3LRP
    _, fx, model = gemma
    ids, S = torch.from_numpy(fx["a/ids"]), int(fx["S"])
    dense = Gemma3LRP.from_hf(model, dtype=torch.float32, max_seq=S, sparse_top=False)
    plain = dense.explain(ids, layer_relevance=True)
    span = dense.explain(ids, positions=[[S - 1]], layer_relevance=True)
    assert torch.equal(span["R_tok"], plain["R_tok"]) and torch.equal(span["logit"][:, 0], plain["logit"])
    assert torch.equal(span["idx"][:, 0], plain["idx"]) and torch.equal(span["layer_R"], plain["layer_R"])
    lp = torch.log_softmax(plain["logits"].double(), -1).gather(1, plain["idx"].long()[:, None])
    assert nmax(span["logprob"], lp) <= 1e-5


@pytest.mark.parametrize("objective", ["logit", "logprob"])
def test_linearity_zeros_per_position_and_readouts(gemma, objective):
    """one left-padded batch of two prompts, T = 4 with a zero and a negative weight; positions on both sides of the window"""
    eng, fx, _ = gemma
    ids, S = torch.from_numpy(fx["c/ids"]), int(fx["S"])
    lengths = fx["c/lengths"].tolist()
    pos = torch.tensor([[30, 3, 40, 11], [25, 44, 18, 31]])
    w = torch.tensor([[1.0, -0.5, 0.0, 2.0], [0.25, 1.0, 1.5, 0.0]])
    B, T = pos.shape
    kw = dict(lengths=lengths, objective=objective)
    before = eng.explain(ids, lengths=lengths, layer_relevance=True)
    joint = eng.explain(ids, positions=pos, position_weights=w, layer_relevance=True, latent=("trace", "resid", "mlp"), heads=("out", "v"),
                        attn_map="sum", return_G=True, **kw)
    tgt = joint["idx"]
    single = [eng.explain(ids, positions=pos[:, t: t + 1], target=tgt[:, t: t + 1], layer_relevance=True, **kw) for t in range(T)]
    for k, wt in (("R_tok", lambda t: w[:, t].cuda()[:, None]), ("layer_R", lambda t: w[:, t].cuda()[None])):
        e = nmax(joint[k], sum(wt(t) * single[t][k].double() for t in range(T)))
        print(f"[gemma3 {objective}] joint vs weighted sum of single-position calls: {k} {e:.2e}")
        assert e <= 1e-5
    assert all(torch.equal(joint["idx"][:, t], single[t]["idx"][:, 0]) and nmax(joint["logit"][:, t], single[t]["logit"][:, 0]) <= 1e-6 for t in range(T))
    # the read-outs see the explained columns: the head's rows of the trace are non-zero exactly there (zero-weight slots: exactly 0)
    L = len(eng.layers)
    live = torch.zeros(B, S, dtype=torch.bool).scatter_(1, pos, w != 0).cuda()
    assert torch.equal(joint["R_trace"][L] != 0, live) and torch.equal(joint["R_trace"][L].sum(-1), joint["layer_R"][L])
    assert torch.equal(joint["R_trace"][0], joint["R_tok"])
    assert nmax(joint["R_trace"].sum(-1), joint["layer_R"]) <= 1e-5 and nmax(joint["R_resid"].sum(-1), joint["layer_R"]) <= 1e-5
    assert joint["R_mlp"].shape == (L, B, eng.cfg["inter"]) and bool(joint["R_mlp"].any())
    # a row of the token-to-token map sums to the head read-out, over heads; sum_t v = 1/2 sum_t out (the uniform rule's share): two
    # fp32 evaluations of one quantity through different kernels, at the project's fp32 bar (tests/test_gemma3_readouts_gpu.py)
    e_row = nmax(joint["R_attn"].sum(-1), joint["R_head_out"].sum(2))
    e_v = nmax(joint["R_head_v"].sum(-1), 0.5 * joint["R_head_out"].sum(-1))
    print(f"[gemma3 {objective}] span read-outs: R_attn rows vs R_head_out {e_row:.2e}  sum R_head_v vs 1/2 sum R_head_out {e_v:.2e}")
    assert e_row <= 1e-4 and e_v <= 1e-4
    assert torch.equal(joint["R_head"], joint["R_head_out"].sum(-1))
    assert nmax((joint["emb"].double() * joint["G_emb"].double()).sum(-1), joint["R_tok"]) <= 1e-5
    for b in range(B):
        top = int(pos[b].max()) + 1
        assert not joint["R_tok"][b, : S - lengths[b]].any() and not joint["R_tok"][b, top:].any()
        assert joint["R_tok"][b, S - lengths[b]: top].any()
        assert not joint["R_head_out"][:, b, :, top:].any() and not joint["R_attn"][:, b, top:].any()
    for t in (1, 2):
        hot = torch.zeros(B, T)
        hot[:, t] = 1.0
        one = eng.explain(ids, positions=pos, position_weights=hot, target=tgt, **kw)
        assert nmax(one["R_tok"], single[t]["R_tok"]) <= 1e-5
    # per_position: T backward passes over one forward ("logit": bitwise the single-position call, see tests/test_span_gpu.py)
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
    assert eng.sparse_top
    with pytest.raises(ValueError):
        eng.explain(ids, positions=pos, per_position=True, layer_relevance=True, **kw)


def test_refusals_launch_nothing(gemma, monkeypatch):
    eng, fx, _ = gemma
    ids, S, V = torch.from_numpy(fx["a/ids"]), int(fx["S"]), eng.cfg["vocab"]

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called before the refusal")

    import lxt_amd.ops as ops
    monkeypatch.setattr(ops, "lib", NoLaunch())
    for kw in (dict(positions=[[3, 3]]), dict(positions=[[S]]), dict(positions=[[-1]]), dict(positions=[3]), dict(positions=[[3], [4]]),
               dict(positions=[[3, 4]], position_weights=[[1.0]]), dict(positions=[[3, 4]], target=[[1, V]]),
               dict(positions=[[3, 4]], target=[1]), dict(positions=[[3]], objective="prob"),
               dict(positions=[[0, 3]], lengths=[S - 1]), dict(positions=[[3]], per_position=True, layer_relevance=True),
               dict(position_weights=[[1.0]]), dict(per_position=True), dict(objective="logprob")):
        with pytest.raises(ValueError):
            eng.explain(ids, **kw)
    with pytest.raises(ValueError):
        eng.explain(inputs_embeds=torch.zeros(1, S, eng.cfg["hidden"]), positions=[[3]])
