"""GPU: seeded sampling in generate() / explain_generated() of LlamaLRP, QwenLRP and Gemma3LRP, on the tiny seeded
fp32 models of tests/test_generate_gpu.py and tests/test_gemma3_generate_gpu.py: prompts of lengths (24, 15, 7), 8 - 12 new tokens."""
import numpy as np
import pytest
import torch

from tests import sample_oracle as so
from tests.util import load

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODELS = ("llama", "qwen3", "gemma3")
S, LENGTHS = 24, (24, 15, 7)
GREEDY_KEYS = ("sequences", "new_tokens", "n_new", "logit", "logprob", "lengths")
KW = dict(temperature=0.8, top_k=20, top_p=0.9, min_p=0.02)


@pytest.fixture(scope="module")
def engines():
    """{model: (fp32 engine, prompt ids [3, 24])}"""
    import lxt_amd.engine as E
    from lxt_amd.engine_gemma3 import Gemma3LRP
    from lxt_amd.engine_qwen import QwenLRP
    from tests.golden import make_golden_generate as gg
    from tests.golden.make_golden_generate_gemma3 import build as build_gemma3
    out = {}
    for m in MODELS:
        fx = load(f"generate_{m}.npz")
        if m == "gemma3":
            eng = Gemma3LRP.from_hf(build_gemma3(), dtype=torch.float32, max_seq=96, device=DEV)
        else:
            eng = (E.LlamaLRP if m == "llama" else QwenLRP).from_hf(gg.build(m), dtype=torch.float32, max_seq=96, device=DEV)
        out[m] = (eng, torch.from_numpy(fx["ids"]))
    return out


def same(a, b, keys, what):
    for k in keys:
        assert torch.equal(a[k], b[k]), (what, k)


def dev(v, dtype):
    return torch.tensor(v, dtype=dtype, device=DEV)


@pytest.mark.parametrize("model", MODELS)
def test_every_sampled_token_is_sample_rows_of_that_steps_logits(engines, model):
    import lxt_amd.ops as ops
    eng, ids = engines[model]
    T = 10
    out = eng.generate(ids, T, lengths=LENGTHS, return_logits=True, do_sample=True, seed=123, **KW)
    assert set(out) == set(GREEDY_KEYS) | {"logits", "sample_logprob"}
    assert out["new_tokens"].shape == (3, T) and out["sample_logprob"].shape == (3, T) and out["sample_logprob"].dtype == torch.float32
    seeds, streams = dev([123] * 3, torch.int64), dev([0, 1, 2], torch.int32)
    for t in range(T):
        logits = out["logits"][:, t].contiguous()
        idx, slp, n_kept, _ = ops.sample_rows(logits, seeds=seeds, streams=streams, step=t, **KW)
        assert torch.equal(idx.long(), out["new_tokens"][:, t]) and torch.equal(slp, out["sample_logprob"][:, t]), t
        assert int(n_kept.min()) >= 1 and int(n_kept.max()) <= 20
        lg, lp, _, _ = ops.span_seed(logits, idx)
        assert torch.equal(lg, out["logit"][:, t]) and torch.equal(lp, out["logprob"][:, t]), t          # the model's own, untempered values
    assert bool((out["sample_logprob"] <= 0).all()) and bool(torch.isfinite(out["sample_logprob"]).all())
    assert len({tuple(r) for r in out["new_tokens"].tolist()}) == 3


@pytest.mark.parametrize("model", MODELS)
def test_same_seed_same_tokens_eager_and_graph(engines, model):
    eng, ids = engines[model]
    keys = GREEDY_KEYS + ("logits", "sample_logprob")
    a = eng.generate(ids, 12, lengths=LENGTHS, return_logits=True, do_sample=True, seed=2024, temperature=1.5)
    same(eng.generate(ids, 12, lengths=LENGTHS, return_logits=True, do_sample=True, seed=2024, temperature=1.5), a, keys, "again")
    same(eng.generate(ids, 12, lengths=LENGTHS, return_logits=True, do_sample=True, seed=2024, temperature=1.5, graph=True), a, keys, "capture")
    same(eng.generate(ids, 12, lengths=LENGTHS, return_logits=True, do_sample=True, seed=2024, temperature=1.5, graph=True), a, keys, "replay")
    b = eng.generate(ids, 12, lengths=LENGTHS, do_sample=True, seed=2025, temperature=1.5)
    assert all(not torch.equal(a["new_tokens"][r], b["new_tokens"][r]) for r in range(3)), "another seed, the same continuation"
    # one seed for the batch: prompt b draws from stream b; a list repeating the seed puts every prompt on stream 0
    c = eng.generate(ids, 12, lengths=LENGTHS, do_sample=True, seed=[2024] * 3, temperature=1.5)
    assert torch.equal(c["new_tokens"][0], a["new_tokens"][0]) and not torch.equal(c["new_tokens"][1:], a["new_tokens"][1:])


BATCH_KW = dict(temperature=0.6, top_k=4)
BATCH_SEEDS = [11, 2 ** 40 + 7, 99]


@pytest.mark.parametrize("model", MODELS)
def test_a_prompt_with_its_own_seed_does_not_depend_on_the_batch(engines, model):
    """seed=[s_0, s_1, s_2]: each prompt alone and un-padded with seed=[s_b] gives the tokens of the left-padded batched call.  The padded
    and the un-padded logits differ by fp32 rounding, so the setting and the seeds are chosen such that, per the fp64 oracle on the batched
    call's own logits, no draw sits within 1e-4 of a boundary -- asserted here"""
    eng, ids = engines[model]
    T = 8
    out = eng.generate(ids, T, lengths=LENGTHS, return_logits=True, do_sample=True, seed=BATCH_SEEDS, **BATCH_KW)
    logits = out["logits"].cpu().numpy()
    for b, n in enumerate(LENGTHS):
        for t in range(T):
            ref = so.sample_row(logits[b, t], so.uniform(BATCH_SEEDS[b], t), margin=1e-4, **BATCH_KW)
            assert not ref["near"], (b, t)
            assert ref["token"] == int(out["new_tokens"][b, t]), (b, t)
        alone = eng.generate(ids[b:b + 1, S - n:], T, do_sample=True, seed=[BATCH_SEEDS[b]], **BATCH_KW)
        assert torch.equal(alone["new_tokens"][0], out["new_tokens"][b]), b


@pytest.mark.parametrize("model", MODELS)
def test_top_k_1_sampling_is_greedy_bit_for_bit(engines, model):
    eng, ids = engines[model]
    greedy = eng.generate(ids, 10, lengths=LENGTHS, return_logits=True)
    for kw in (dict(top_k=1), dict(top_k=1, temperature=3.0, top_p=0.5)):
        got = eng.generate(ids, 10, lengths=LENGTHS, return_logits=True, do_sample=True, seed=5, **kw)
        same(got, greedy, GREEDY_KEYS + ("logits",), kw)
    assert set(greedy) == set(GREEDY_KEYS) | {"logits"} and "sample_logprob" not in greedy


@pytest.mark.parametrize("model", ["llama", "gemma3"])
def test_eos_under_sampling(engines, model):
    eng, ids = engines[model]
    T = 12
    free = eng.generate(ids, T, lengths=LENGTHS, do_sample=True, seed=77, **KW)
    tok = free["new_tokens"].cpu().numpy()
    eos = int(tok[0, 3])
    pad = 3 if eos != 3 else 4
    n_want = [int(np.nonzero(tok[b] == eos)[0][0]) + 1 if (tok[b] == eos).any() else T for b in range(3)]
    assert n_want[0] <= 4 and pad != eos
    out = eng.generate(ids, T, lengths=LENGTHS, eos_token_id=eos, pad_token_id=pad, do_sample=True, seed=77, **KW)
    Te = max(n_want)
    assert out["new_tokens"].shape == (3, Te) and out["n_new"].tolist() == n_want and out["lengths"].tolist() == [n + Te for n in LENGTHS]
    assert out["sample_logprob"].shape == (3, Te)
    for b in range(3):
        got = out["new_tokens"][b].cpu().numpy()
        assert np.array_equal(got[: n_want[b]], tok[b, : n_want[b]]) and (got[n_want[b]:] == pad).all(), b
    # every prompt stops at once: the loop ends early
    out = eng.generate(ids, T, lengths=LENGTHS, eos_token_id=[int(tok[b, 1]) for b in range(3)], do_sample=True, seed=77, **KW)
    assert out["new_tokens"].shape[1] <= 2 and max(out["n_new"].tolist()) == out["new_tokens"].shape[1]


@pytest.mark.parametrize("model", MODELS)
def test_explain_generated_sampled_is_generate_then_explain(engines, model):
    eng, ids = engines[model]
    T = 8
    got = eng.explain_generated(ids, T, lengths=LENGTHS, do_sample=True, seed=31, **KW)
    gen = eng.generate(ids, T, lengths=LENGTHS, do_sample=True, seed=31, **KW)
    for k in ("sequences", "new_tokens", "n_new"):
        assert torch.equal(got[k], gen[k]), k
    positions = torch.arange(S - 1, S + T - 1).expand(3, T)
    want = eng.explain(got["sequences"], lengths=gen["lengths"], positions=positions, position_weights=torch.ones(3, T), objective="logprob")
    for k in ("R_tok", "logit", "logprob", "idx"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["idx"].long(), gen["new_tokens"])
    R = got["R_tok"]
    assert R.shape == (3, S + T) and bool((R[:, -1] == 0).all()), "the last column is no explained row"
    for b, n in enumerate(LENGTHS):
        assert bool((R[b, : S - n] == 0).all()) and bool(R[b, S - n: -1].any()), b
    # the sampled answer is not the greedy one, and "mean" weights pass through as before
    assert not torch.equal(gen["new_tokens"], eng.generate(ids, T, lengths=LENGTHS)["new_tokens"])
    m = eng.explain_generated(ids, T, lengths=LENGTHS, position_weights="mean", do_sample=True, seed=31, **KW)
    want = eng.explain(m["sequences"], lengths=gen["lengths"], positions=positions, position_weights=torch.full((3, T), 1.0 / T),
                       objective="logprob")
    assert torch.equal(m["R_tok"], want["R_tok"]) and torch.equal(m["new_tokens"], gen["new_tokens"])


@pytest.mark.parametrize("model", ["qwen3", "gemma3"])
def test_greedy_and_explain_unchanged_by_a_sampled_call_between(engines, model):
    eng, ids = engines[model]
    g0 = {k: v.clone() for k, v in eng.generate(ids, 10, lengths=LENGTHS, return_logits=True).items()}
    gg0 = {k: v.clone() for k, v in eng.generate(ids, 10, lengths=LENGTHS, return_logits=True, graph=True).items()}
    e0 = {k: v.clone() for k, v in eng.explain(ids, lengths=LENGTHS).items()}
    eng.generate(ids, 12, lengths=LENGTHS, do_sample=True, seed=1, **KW)
    eng.generate(ids, 10, lengths=LENGTHS, do_sample=True, seed=1, graph=True, **KW)
    g1, gg1, e1 = (eng.generate(ids, 10, lengths=LENGTHS, return_logits=True), eng.generate(ids, 10, lengths=LENGTHS, return_logits=True, graph=True),
                   eng.explain(ids, lengths=LENGTHS))
    assert set(g1) == set(GREEDY_KEYS) | {"logits"} == set(g0)
    same(g1, g0, tuple(g0), "eager")
    same(gg1, gg0, tuple(gg0), "graph")
    same(gg0, g0, tuple(g0), "graph against eager")
    same(e1, e0, tuple(e0), "explain")


@pytest.mark.parametrize("model", ["llama", "gemma3"])
def test_refusals_raise_before_any_kernel(engines, model, monkeypatch):
    eng, ids = engines[model]

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called before the refusal")

    import lxt_amd.ops as ops
    monkeypatch.setattr(ops, "lib", NoLaunch())
    ok = dict(do_sample=True, seed=3)
    bad = (dict(temperature=0.7), dict(top_k=5), dict(top_p=0.9), dict(min_p=0.1), dict(seed=3), dict(do_sample=True),
           dict(ok, temperature=0.0), dict(ok, temperature=-1.0), dict(ok, temperature=float("nan")), dict(ok, temperature=float("inf")),
           dict(ok, top_k=-1), dict(ok, top_k=1.5), dict(ok, top_p=0.0), dict(ok, top_p=1.01), dict(ok, min_p=-0.01), dict(ok, min_p=1.01),
           dict(do_sample=True, seed=1.0), dict(do_sample=True, seed=[1, 2]), dict(do_sample=True, seed=[1, 2, 3, 4]), dict(do_sample=True, seed="1"),
           dict(ok, force_tokens=torch.zeros(3, 4, dtype=torch.long)))
    for kw in bad:
        with pytest.raises(ValueError):
            eng.generate(ids, 4, lengths=LENGTHS, **kw)
        if "force_tokens" not in kw:
            with pytest.raises(ValueError):
                eng.explain_generated(ids, 4, lengths=LENGTHS, **kw)
