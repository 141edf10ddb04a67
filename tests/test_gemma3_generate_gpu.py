"""GPU: Gemma3LRP.generate() and explain_generated().  Fixture: tests/golden/generate_gemma3.npz, greedy
continuations by HuggingFace alone in fp64, each prompt un-padded (make_golden_generate_gemma3.py); the tiny model's window of 32 is passed
by the two longer prompts during generation."""
import numpy as np
import pytest
import torch

from tests.util import load, nmax

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
S, NEW, LENGTHS = 24, 24, (24, 15, 7)


@pytest.fixture(scope="module")
def tiny():
    """(fp32 engine, fixture), built once from the seeded HF model the fixture was generated on"""
    from lxt_amd.engine_gemma3 import Gemma3LRP
    from tests.golden.hf_models import wsum
    from tests.golden.make_golden_generate_gemma3 import build
    fx, model = load("generate_gemma3.npz"), build()
    got = wsum(model)
    assert abs(got - float(fx["wsum"])) <= 1e-9 * got, "the seeded weights did not reproduce"
    eng = Gemma3LRP.from_hf(model, dtype=F32, max_seq=96, device=DEV)
    assert eng.sparse_top and eng.cfg["window"] == int(fx["window"]) < S + NEW - 1
    return eng, fx


def fx_ids(fx):
    return torch.from_numpy(fx["ids"])


def span_positions(B, S_, T):
    return torch.arange(S_ - 1, S_ + T - 1).expand(B, T)


def first_hit(tokens, eos):
    hit = np.nonzero(np.isin(tokens, eos))[0]
    return int(hit[0]) + 1 if hit.size else len(tokens)


def test_fp32_engine_reproduces_hf_greedy_generation(tiny):
    """one left-padded call with lengths (24, 15, 7) against HF's un-padded fp64 runs: the same tokens, and logits / logit / logprob within
    the project's fp32 bar, 1e-4 max-normalised; each prompt alone gives the same tokens"""
    eng, fx = tiny
    out = eng.generate(fx_ids(fx), NEW, lengths=LENGTHS, return_logits=True)
    tok, ref = torch.from_numpy(fx["tokens"]), torch.from_numpy(fx["logits"])
    e_logits = nmax(out["logits"], ref)
    e_logit = nmax(out["logit"], ref.gather(2, tok[..., None])[..., 0])
    e_lp = nmax(out["logprob"], torch.log_softmax(ref, -1).gather(2, tok[..., None])[..., 0])
    same = bool((out["new_tokens"].cpu() == tok).all())
    print(f"[generate gemma3 fp32 vs HF fp64] tokens equal {same}; max-normalised logits {e_logits:.2e} logit {e_logit:.2e} logprob {e_lp:.2e} "
          f"(fixture margin {float(fx['margin']):.2e})")
    assert same, (out["new_tokens"].cpu() != tok).nonzero().tolist()
    assert e_logits <= 1e-4 and e_logit <= 1e-4 and e_lp <= 1e-4
    assert out["new_tokens"].dtype == torch.int64 and out["sequences"].shape == (3, S + NEW) and out["logits"].shape == ref.shape
    assert torch.equal(out["sequences"][:, :S].cpu(), fx_ids(fx)) and torch.equal(out["sequences"][:, S:], out["new_tokens"])
    assert out["n_new"].tolist() == [NEW] * 3 and out["lengths"].tolist() == [n + NEW for n in LENGTHS]
    for b, n in enumerate(LENGTHS):
        alone = eng.generate(fx_ids(fx)[b:b + 1, S - n:], NEW)
        assert torch.equal(alone["new_tokens"][0].cpu(), tok[b]), b


def test_eos_stops_a_prompt_and_pads_it(tiny):
    eng, fx = tiny
    tok = fx["tokens"]
    eos, pad = int(tok[0, 10]), 3
    n_want = [first_hit(tok[b], [eos]) for b in range(3)]
    assert n_want[0] <= 11 and pad != eos
    out = eng.generate(fx_ids(fx), NEW, lengths=LENGTHS, eos_token_id=eos, pad_token_id=pad)
    T = max(n_want)
    assert out["new_tokens"].shape == (3, T) and out["n_new"].tolist() == n_want and out["lengths"].tolist() == [n + T for n in LENGTHS]
    for b in range(3):
        got = out["new_tokens"][b].cpu().numpy()
        assert np.array_equal(got[: n_want[b]], tok[b, : n_want[b]]) and (got[n_want[b]:] == pad).all(), b
    # teacher forcing: the forced answer comes back, scored through the cache
    forced = torch.from_numpy(tok[:, :6]).roll(1, 0)
    out = eng.generate(fx_ids(fx), 6, lengths=LENGTHS, force_tokens=forced)
    assert torch.equal(out["new_tokens"].cpu(), forced.long())
    ex = eng.explain(out["sequences"], lengths=out["lengths"], positions=span_positions(3, S, 6), objective="logit")
    assert torch.equal(ex["idx"].long(), out["new_tokens"]) and nmax(out["logit"], ex["logit"]) <= 1e-4


def test_fp32_decode_logits_equal_the_prefill_of_the_whole_sequence(tiny):
    """teacher forcing through explain(positions=...) re-computes every step's logit in ONE prefill-shaped forward without a cache: the
    sliding layers of the two paths must keep the same keys"""
    eng, fx = tiny
    out = eng.generate(fx_ids(fx), NEW, lengths=LENGTHS)
    ex = eng.explain(out["sequences"], lengths=out["lengths"], positions=span_positions(3, S, NEW), objective="logit")
    err, err_lp = nmax(out["logit"], ex["logit"]), nmax(out["logprob"], ex["logprob"])
    print(f"[generate gemma3 fp32] decode path vs prefill path: logit {err:.2e} logprob {err_lp:.2e}")
    assert torch.equal(ex["idx"].long(), out["new_tokens"])
    assert err <= 1e-4 and err_lp <= 1e-4


def test_bf16_decode_path_at_4b_dims_is_as_close_to_fp32_as_the_prefill_path():
    """2 layers (one local, one global) at the Gemma-3-4B text dimensions: 8 / 4 heads of d = 256 (the site kernel and the decode attention at
    their real shape), window 1024 < S = 1040, so the local layer slides from the first step on; 8 new tokens, lengths (1040, 700).  Both bf16
    paths score the SAME sequence (the fp32 engine's continuation, forced): the decode path's error against the fp32 engine's logits must be
    within 2 x the prefill path's error against the same values (the rule of test_generate_gpu.py).  Both figures are printed."""
    from lxt_amd.engine_gemma3 import Gemma3LRP
    from tests.golden.hf_models import build_gemma3_4bdims
    S4, T, lens = 1040, 8, (1040, 700)
    model = build_gemma3_4bdims()
    ids = torch.randint(0, 4096, (2, S4), generator=torch.Generator().manual_seed(4))
    f32 = Gemma3LRP.from_hf(model, dtype=F32, max_seq=S4 + T, device=DEV)
    assert f32.cfg["window"] == 1024 and f32.cfg["head_dim"] == 256
    ref = f32.generate(ids, T, lengths=lens)
    del f32
    bf = Gemma3LRP.from_hf(model, dtype=BF16, max_seq=S4 + T, device=DEV)
    dec = bf.generate(ids, T, lengths=lens, force_tokens=ref["new_tokens"])
    assert torch.equal(dec["new_tokens"], ref["new_tokens"])
    pre = bf.explain(ref["sequences"], lengths=ref["lengths"], positions=span_positions(2, S4, T), objective="logit")
    assert torch.equal(pre["idx"].long(), ref["new_tokens"])
    e_dec, e_pre = nmax(dec["logit"], ref["logit"]), nmax(pre["logit"], ref["logit"])
    print(f"[generate gemma3 bf16 4B dims] max-normalised logit error vs the fp32 engine: decode path {e_dec:.3e}, prefill path {e_pre:.3e}")
    assert e_dec <= 2.0 * e_pre, (e_dec, e_pre)
    graph = bf.generate(ids, T, lengths=lens, force_tokens=ref["new_tokens"], graph=True)
    assert torch.equal(graph["logit"], dec["logit"]) and torch.equal(graph["logprob"], dec["logprob"])


KEYS = ("sequences", "new_tokens", "n_new", "logit", "logprob", "logits", "lengths")


def assert_same(a, b, what):
    for k in KEYS:
        assert torch.equal(a[k], b[k]), (what, k)


def test_graph_replay_equals_eager_bit_for_bit(tiny):
    eng, fx = tiny
    ids = fx_ids(fx)
    eager = eng.generate(ids, 12, lengths=LENGTHS, return_logits=True)
    assert_same(eng.generate(ids, 12, lengths=LENGTHS, return_logits=True, graph=True), eager, "capture")
    assert ("decode", 3, S + 12) in eng._graphs.graphs
    assert_same(eng.generate(ids, 12, lengths=LENGTHS, return_logits=True, graph=True), eager, "replay")
    other = torch.roll(ids, 5, 1)                    # the same graph on other token ids (lengths: all columns)
    assert_same(eng.generate(other, 12, return_logits=True, graph=True), eng.generate(other, 12, return_logits=True), "replay, other ids")
    big = eng.generate(ids, 40, lengths=LENGTHS, return_logits=True)          # a larger cap: the caches are re-allocated, the graphs re-captured
    assert_same(eng.generate(ids, 40, lengths=LENGTHS, return_logits=True, graph=True), big, "larger cap")
    assert_same(eng.generate(ids, 12, lengths=LENGTHS, return_logits=True, graph=True), eager, "re-capture")
    assert torch.equal(big["new_tokens"][:, :12], eager["new_tokens"])


def test_explain_generated_is_generate_then_explain(tiny):
    eng, fx = tiny
    ids, T = fx_ids(fx), 10
    got = eng.explain_generated(ids, T, lengths=LENGTHS, layer_relevance=True)
    gen = eng.generate(ids, T, lengths=LENGTHS)
    want = eng.explain(gen["sequences"], lengths=gen["lengths"], positions=span_positions(3, S, T), position_weights=torch.ones(3, T),
                       objective="logprob", layer_relevance=True)
    for k in ("R_tok", "logit", "logprob", "idx", "layer_R"):
        assert torch.equal(got[k], want[k]), k
    for k in ("sequences", "new_tokens", "n_new"):
        assert torch.equal(got[k], gen[k]), k
    assert torch.equal(got["idx"].long(), gen["new_tokens"]) and got["R_tok"].shape == (3, S + T) and "logits" not in got
    R = got["R_tok"]
    assert bool((R[:, -1] == 0).all()), "the last column is no explained row"
    for b, n in enumerate(LENGTHS):
        assert bool((R[b, : S - n] == 0).all()) and bool(R[b, S - n: -1].any()), b
    # with an EOS: the slots after it carry weight 0 (here: equal to the explicit weights), "mean" divides by n_new
    tok = fx["tokens"]
    eos = int(tok[0, 4])
    n_want = [first_hit(tok[b, :T], [eos]) for b in range(3)]
    assert min(n_want) < max(n_want)
    for pw in (None, "mean"):
        got = eng.explain_generated(ids, T, lengths=LENGTHS, eos_token_id=eos, position_weights=pw, objective="logit", per_position=True)
        Te = max(n_want)
        assert got["n_new"].tolist() == n_want and got["new_tokens"].shape == (3, Te)
        w = torch.tensor([[1.0 if t < n_want[b] else 0.0 for t in range(Te)] for b in range(3)])
        if pw == "mean":
            w = w / torch.tensor(n_want, dtype=torch.float32)[:, None]
        want = eng.explain(got["sequences"], lengths=[n + Te for n in LENGTHS], positions=span_positions(3, S, Te), position_weights=w,
                           objective="logit", per_position=True)
        assert torch.equal(got["R_tok"], want["R_tok"]) and torch.equal(got["R_tok_each"], want["R_tok_each"])
        for b in range(3):
            assert not got["R_tok_each"][b, n_want[b]:].any() and bool(got["R_tok_each"][b, : n_want[b]].any()), (pw, b)


def test_plain_explain_is_unchanged_by_a_generate_between(tiny):
    eng, fx = tiny
    ids = fx_ids(fx)
    before = {k: v.clone() for k, v in eng.explain(ids, lengths=LENGTHS, layer_relevance=True, heads=("out",)).items()}
    eng.generate(ids, 30, lengths=LENGTHS, graph=True)
    after = eng.explain(ids, lengths=LENGTHS, layer_relevance=True, heads=("out",))
    assert set(before) == set(after)
    for k in before:
        assert torch.equal(before[k], after[k]), k


def test_refusals_raise_before_any_kernel(tiny, monkeypatch):
    import lxt_amd._lib as L
    eng, fx = tiny
    ids, V = fx_ids(fx), eng.cfg["vocab"]

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called before the refusal")

    import lxt_amd.ops as ops
    monkeypatch.setattr(ops, "lib", NoLaunch())
    bad = (dict(input_ids=None, inputs_embeds=torch.zeros(3, S, eng.cfg["hidden"])), dict(max_new_tokens=0), dict(max_new_tokens=-3),
           dict(max_new_tokens=2.0), dict(max_new_tokens=eng.max_seq - S + 1), dict(lengths=(24, 15)), dict(lengths=(24, 15, 0)),
           dict(lengths=(25, 15, 7)), dict(lengths=(24.0, 15.0, 7.0)), dict(eos_token_id=V), dict(eos_token_id=-1), dict(eos_token_id=[1, V]),
           dict(eos_token_id=[]), dict(eos_token_id=1.5), dict(pad_token_id=V), dict(eos_token_id=2, pad_token_id=-1),
           dict(force_tokens=torch.zeros(3, 3, dtype=torch.long)), dict(force_tokens=torch.full((3, 4), V)))
    for kw in bad:
        args = dict(dict(input_ids=ids, max_new_tokens=4), **kw)
        with pytest.raises(ValueError):
            eng.generate(**args)
        if "inputs_embeds" not in kw and "force_tokens" not in kw:          # (generate's own keywords)
            with pytest.raises(ValueError):
                eng.explain_generated(**args)
    with pytest.raises(ValueError):
        eng.generate(ids + V, 4)
    assert L.lib is not None
