"""GPU: LlamaLRP / QwenLRP.generate() and explain_generated().  Fixtures: tests/golden/generate_*.npz, greedy
continuations by HuggingFace alone in fp64, each prompt un-padded (make_golden_generate.py)."""
import numpy as np
import pytest
import torch

from tests.util import load, nmax

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
MODELS = ("llama", "qwen2", "qwen3")
S, NEW, LENGTHS = 24, 24, (24, 15, 7)


@pytest.fixture(scope="module")
def engines():
    """{model: (fp32 engine, fixture)}, built once from the seeded HF models the fixtures were generated on"""
    import lxt_amd.engine as E
    from lxt_amd.engine_qwen import QwenLRP
    from tests.golden import make_golden_generate as gg
    from tests.golden.hf_models import wsum
    out = {}
    for m in MODELS:
        fx, model = load(f"generate_{m}.npz"), gg.build(m)
        got = wsum(model)
        assert abs(got - float(fx["wsum"])) <= 1e-9 * got, f"seeded weights of {m} did not reproduce"
        cls = E.LlamaLRP if m == "llama" else QwenLRP
        out[m] = (cls.from_hf(model, dtype=F32, max_seq=96, device=DEV), fx)
    return out


def fx_ids(fx):
    return torch.from_numpy(fx["ids"])


def span_positions(B, S_, T):
    return torch.arange(S_ - 1, S_ + T - 1).expand(B, T)


# ---- (i) the fixtures ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_fp32_engine_reproduces_hf_greedy_generation(engines, model):
    """one left-padded call with lengths (24, 15, 7) against HF's un-padded fp64 runs: the same tokens, and logits / logit / logprob within the
    project's fp32 bar, 1e-4 max-normalised"""
    eng, fx = engines[model]
    out = eng.generate(fx_ids(fx), NEW, lengths=LENGTHS, return_logits=True)
    tok, ref = torch.from_numpy(fx["tokens"]), torch.from_numpy(fx["logits"])
    e_logits = nmax(out["logits"], ref)
    e_logit = nmax(out["logit"], ref.gather(2, tok[..., None])[..., 0])
    e_lp = nmax(out["logprob"], torch.log_softmax(ref, -1).gather(2, tok[..., None])[..., 0])
    same = bool((out["new_tokens"].cpu() == tok).all())
    print(f"[generate {model} fp32 vs HF fp64] tokens equal {same}; max-normalised logits {e_logits:.2e} logit {e_logit:.2e} logprob {e_lp:.2e} "
          f"(fixture margin {float(fx['margin']):.2e})")
    assert same, (out["new_tokens"].cpu() != tok).nonzero().tolist()
    assert e_logits <= 1e-4 and e_logit <= 1e-4 and e_lp <= 1e-4
    assert out["new_tokens"].dtype == torch.int64 and out["sequences"].shape == (3, S + NEW) and out["logits"].shape == ref.shape
    assert torch.equal(out["sequences"][:, :S].cpu(), fx_ids(fx)) and torch.equal(out["sequences"][:, S:], out["new_tokens"])
    assert out["n_new"].tolist() == [NEW] * 3 and out["lengths"].tolist() == [n + NEW for n in LENGTHS]
    # each prompt alone and un-padded, as HF ran it: the same tokens
    for b, n in enumerate(LENGTHS):
        alone = eng.generate(fx_ids(fx)[b:b + 1, S - n:], NEW)
        assert torch.equal(alone["new_tokens"][0].cpu(), tok[b]), b


# ---- (ii) EOS -----------------------------------------------------------------------------------------------------------------------------
def first_hit(tokens, eos):
    """tokens [T] -> number of tokens up to and including the first one in eos (T if none)"""
    hit = np.nonzero(np.isin(tokens, eos))[0]
    return int(hit[0]) + 1 if hit.size else len(tokens)


@pytest.mark.parametrize("model", ["llama", "qwen3"])
def test_eos_stops_a_prompt_and_pads_it(engines, model):
    eng, fx = engines[model]
    tok = fx["tokens"]
    eos, pad = int(tok[0, 10]), 3                    # a token prompt 0 emits mid-answer (the others stop too if they emit it: counted below)
    n_want = [first_hit(tok[b], [eos]) for b in range(3)]
    assert n_want[0] <= 11 and pad != eos
    out = eng.generate(fx_ids(fx), NEW, lengths=LENGTHS, eos_token_id=eos, pad_token_id=pad)
    T = max(n_want)
    assert out["new_tokens"].shape == (3, T) and out["n_new"].tolist() == n_want and out["lengths"].tolist() == [n + T for n in LENGTHS]
    for b in range(3):
        got = out["new_tokens"][b].cpu().numpy()
        assert np.array_equal(got[: n_want[b]], tok[b, : n_want[b]]) and (got[n_want[b]:] == pad).all(), b
        assert got[n_want[b] - 1] == eos or n_want[b] == NEW
    # an EOS list that every prompt meets: the loop stops early; pad_token_id defaults to the first EOS id
    eos_l = [int(tok[b, 5 + 2 * b]) for b in range(3)]
    n_want = [first_hit(tok[b], eos_l) for b in range(3)]
    assert max(n_want) < NEW
    out = eng.generate(fx_ids(fx), NEW, lengths=LENGTHS, eos_token_id=eos_l)
    assert out["new_tokens"].shape[1] == max(n_want) < NEW and out["n_new"].tolist() == n_want
    for b in range(3):
        got = out["new_tokens"][b].cpu().numpy()
        assert np.array_equal(got[: n_want[b]], tok[b, : n_want[b]]) and (got[n_want[b]:] == eos_l[0]).all(), b


# ---- (iii) the cache against the engine's own prefill -------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_fp32_decode_logits_equal_the_prefill_of_the_whole_sequence(engines, model):
    """teacher forcing through explain(positions=...) re-computes every step's logit in ONE prefill-shaped forward without a cache"""
    eng, fx = engines[model]
    out = eng.generate(fx_ids(fx), NEW, lengths=LENGTHS)
    ex = eng.explain(out["sequences"], lengths=out["lengths"], positions=span_positions(3, S, NEW), objective="logit")
    err, err_lp = nmax(out["logit"], ex["logit"]), nmax(out["logprob"], ex["logprob"])
    print(f"[generate {model} fp32] decode path vs prefill path: logit {err:.2e} logprob {err_lp:.2e}")
    assert torch.equal(ex["idx"].long(), out["new_tokens"])
    assert err <= 1e-4 and err_lp <= 1e-4


CFG8B = dict(hidden=4096, inter=14336, n_layers=2, n_heads=32, n_kv=8, head_dim=128, vocab=4096, rope_theta=5e5, rms_eps=1e-5)


def test_bf16_decode_path_at_8b_widths_is_as_close_to_fp32_as_the_prefill_path():
    """2 layers at the Llama-3-8B widths (the weight-streaming Linears and the GQA-4 decode kernel at their real shapes), S = 128, 8 new tokens,
    prompts left-padded.  Both bf16 paths score the SAME sequence (the fp32 engine's continuation, forced): the decode path's error against
    the fp32 engine's logits must be within 2 x the prefill path's error against the same values -- one precision class, differently
    blocked sums.  Both figures are printed (DESIGN.md section 21 records them)."""
    import lxt_amd.engine as E
    H, I, d, S8, T = 4096, 14336, 128, 128, 8
    g = torch.Generator(device=DEV).manual_seed(3)
    rn = lambda *s: (torch.randn(*s, generator=g, device=DEV) * 0.02).bfloat16()              # noqa: E731
    nw = lambda: (1.0 + 0.1 * torch.randn(H, generator=g, device=DEV)).bfloat16()            # noqa: E731
    W = dict(embed=rn(4096, H), norm=nw(), lm_head=rn(4096, H),
             layers=[dict(ln1=nw(), ln2=nw(), wq=rn(32 * d, H), wk=rn(8 * d, H), wv=rn(8 * d, H), wo=rn(H, 32 * d), wg=rn(I, H), wu=rn(I, H),
                          wd=rn(H, I)) for _ in range(2)])
    ids = torch.randint(0, 4096, (2, S8), generator=torch.Generator().manual_seed(4))
    lens = (S8, 77)
    f32 = E.LlamaLRP(CFG8B, W, dtype=F32, max_seq=256, device=DEV)
    ref = f32.generate(ids, T, lengths=lens)
    del f32
    bf = E.LlamaLRP(CFG8B, W, dtype=BF16, max_seq=256, device=DEV)
    dec = bf.generate(ids, T, lengths=lens, force_tokens=ref["new_tokens"])
    assert torch.equal(dec["new_tokens"], ref["new_tokens"])
    pre = bf.explain(ref["sequences"], lengths=ref["lengths"], positions=span_positions(2, S8, T), objective="logit")
    assert torch.equal(pre["idx"].long(), ref["new_tokens"])
    e_dec, e_pre = nmax(dec["logit"], ref["logit"]), nmax(pre["logit"], ref["logit"])
    # (slot 0 of the decode path IS the prefill's last row: the two differ from slot 1 on)
    print(f"[generate bf16 8B widths] max-normalised logit error vs the fp32 engine: decode path {e_dec:.3e}, prefill path {e_pre:.3e}; "
          f"own arg-max equals the forced token in {int((bf.generate(ids, T, lengths=lens)['new_tokens'] == ref['new_tokens']).sum())} of {2 * T} slots")
    assert e_dec <= 2.0 * e_pre, (e_dec, e_pre)


# ---- (iv) graph replay -----------------------------------------------------------------------------------------------------------------------
KEYS = ("sequences", "new_tokens", "n_new", "logit", "logprob", "logits", "lengths")


def assert_same(a, b, what):
    for k in KEYS:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("model", ["llama", "qwen2"])
def test_graph_replay_equals_eager_bit_for_bit(engines, model):
    eng, fx = engines[model]
    ids = fx_ids(fx)
    eager = eng.generate(ids, 12, lengths=LENGTHS, return_logits=True)
    assert_same(eng.generate(ids, 12, lengths=LENGTHS, return_logits=True, graph=True), eager, "capture")
    assert ("decode", 3, S + 12, eng.mode) in eng._graphs.graphs
    assert_same(eng.generate(ids, 12, lengths=LENGTHS, return_logits=True, graph=True), eager, "replay")
    other = torch.roll(ids, 5, 1)                    # the same graph on other token ids (lengths: all columns)
    assert_same(eng.generate(other, 12, return_logits=True, graph=True), eng.generate(other, 12, return_logits=True), "replay, other ids")
    big = eng.generate(ids, 40, lengths=LENGTHS, return_logits=True)          # a larger cap: the caches are re-allocated, the graphs re-captured
    assert_same(eng.generate(ids, 40, lengths=LENGTHS, return_logits=True, graph=True), big, "larger cap")
    assert_same(eng.generate(ids, 12, lengths=LENGTHS, return_logits=True, graph=True), eager, "re-capture")
    assert torch.equal(big["new_tokens"][:, :12], eager["new_tokens"])


# ---- (v) explain_generated -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["llama", "qwen3"])
def test_explain_generated_is_generate_then_explain(engines, model):
    eng, fx = engines[model]
    ids, T = fx_ids(fx), 10
    got = eng.explain_generated(ids, T, lengths=LENGTHS, layer_relevance=True)
    gen = eng.generate(ids, T, lengths=LENGTHS)
    want = eng.explain(gen["sequences"], lengths=gen["lengths"], positions=span_positions(3, S, T), position_weights=torch.ones(3, T),
                       objective="logprob", layer_relevance=True)
    for k in ("R_tok", "logit", "logprob", "idx", "layer_R"):
        assert torch.equal(got[k], want[k]), k
    for k in ("sequences", "new_tokens", "n_new"):
        assert torch.equal(got[k], gen[k]), k
    assert torch.equal(got["idx"].long(), gen["new_tokens"]) and got["R_tok"].shape == (3, S + T)
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


# ---- (vi) a plain explanation before and after ---------------------------------------------------------------------------------------------
def test_plain_explain_is_unchanged_by_a_generate_between(engines):
    eng, fx = engines["qwen3"]
    ids = fx_ids(fx)
    before = {k: v.clone() for k, v in eng.explain(ids, lengths=LENGTHS, layer_relevance=True).items()}
    g_before = {k: v.clone() for k, v in eng.explain(ids, graph=True).items()}
    eng.generate(ids, 30, lengths=LENGTHS, graph=True)
    after, g_after = eng.explain(ids, lengths=LENGTHS, layer_relevance=True), eng.explain(ids, graph=True)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    for k in g_before:
        assert torch.equal(g_before[k], g_after[k]), ("graph", k)


# ---- (vii) MXFP4 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_mxfp4_engine_generates_what_its_dequantised_weights_generate(dtype):
    from lxt_amd.engine import LlamaLRP
    from tests.util import llama_case
    cfg, W, _, _ = llama_case("d128")                 # H 512, I 1024, 2 layers, 4 + 1 heads of 128
    q = LlamaLRP(cfg, W, weight_format="mxfp4", dtype=dtype, device=DEV, max_seq=128)
    plain = LlamaLRP(*q.dequantized_weights(), dtype=dtype, device=DEV, max_seq=128)
    ids = torch.randint(0, cfg["vocab"], (3, 40), generator=torch.Generator().manual_seed(9))
    for kw in (dict(), dict(graph=True)):
        a = q.generate(ids, 12, lengths=(40, 21, 9), return_logits=True, **kw)
        b = plain.generate(ids, 12, lengths=(40, 21, 9), return_logits=True, **kw)
        assert_same(a, b, kw)


# ---- (viii) refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_raise_before_any_kernel(engines, monkeypatch):
    import lxt_amd._lib as L
    eng, fx = engines["llama"]
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


def test_moe_driver_states_that_it_does_not_generate():
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    for name in ("generate", "explain_generated"):
        with pytest.raises(NotImplementedError, match="dense"):
            getattr(Qwen3MoeLRP, name)(None, None, 4)
