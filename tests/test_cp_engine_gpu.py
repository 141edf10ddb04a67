"""GPU: CP-LRP on the fused drivers, LlamaLRP / QwenLRP(rule="cp").
  (i)    the fp32 engines against tests/golden/cp_{llama,qwen2,qwen3}.npz -- the REAL lxt.efficient cp_LRP maps in fp64 (make_golden_cp.py) --
         with sparse_top and fold_norm both ways: the left-padded batch and the span case with both objectives.  Bar: 1e-4 normalised max
         error, the bar tests/test_span_gpu.py and tests/test_hf_gpu.py hold fp32 engines to against fp64 reference fixtures on these
         models.  R_tok is exactly 0 at pads; sum R_tok equals the fixture's own sum (CP-LRP is not conservative through a biased Linear or
         the detached gate, so the reference is the yardstick, not the logit);
  (ii)   the same HF models under lxt_amd.efficient.monkey_patch with the CP maps (the drop-in path), one fresh process;
  (iii)  rule="attnlrp" after set_rule("cp") and back is bitwise the untouched engine; graph=True is bitwise eager;
  (iv)   the served read-outs: layer_relevance, latent, return_G, target and seed;
  (v)    bf16 at the Llama-3-8B layer widths, S = 256, against the fp32 CP engine;
  (vi)   explain_generated: the rule does not change the tokens, and R_tok is explain(sequences, positions=...) by hand;
  (vii)  the refusals raise before a kernel runs."""
import os
import subprocess
import sys

import pytest
import torch

from tests.util import load, nmax

pytestmark = pytest.mark.gpu

MODELS = ("llama", "qwen2", "qwen3")
BAR = 1e-4          # test_span_gpu.py::test_fp32_engines_vs_reference, test_hf_gpu.py::test_model_family_maps
S, LENGTHS = 24, (24, 15, 7)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _engine(name, **kw):
    import lxt_amd.engine as E
    from lxt_amd.engine_qwen import QwenLRP
    from tests.golden.hf_models import wsum
    from tests.golden.make_golden_generate import build
    fx, model = load(f"cp_{name}.npz"), build(name)
    got = wsum(model)
    assert abs(got - float(fx["wsum"])) <= 1e-9 * got, f"seeded weights of {name} did not reproduce"
    kw = dict(dict(dtype=torch.float32, max_seq=64), **kw)
    return (E.LlamaLRP if name == "llama" else QwenLRP).from_hf(model, **kw), fx


@pytest.fixture(scope="module")
def engines():
    """{model: (fp32 engine with rule="cp" and the class defaults, fixture)}"""
    _need_gpu()
    return {m: _engine(m, rule="cp") for m in MODELS}


@pytest.mark.parametrize("fold_norm", [False, True])
@pytest.mark.parametrize("sparse_top", [True, False])
@pytest.mark.parametrize("model", MODELS)
def test_fp32_engines_vs_reference(engines, model, sparse_top, fold_norm):
    if (sparse_top, fold_norm) == (True, False):
        eng, fx = engines[model]
        assert eng.sparse_top and not eng.folded
    else:
        eng, fx = _engine(model, rule="cp", sparse_top=sparse_top, fold_norm=fold_norm)
    ids = torch.from_numpy(fx["ids"])
    out = eng.explain(ids, lengths=list(LENGTHS), layer_relevance=True)
    assert out["idx"].cpu().tolist() == fx["idx"].tolist()
    errs = {k: nmax(out[k], fx[k]) for k in ("R_tok", "logit", "layer_R")}
    R, Rfx = out["R_tok"].double().cpu(), torch.from_numpy(fx["R_tok"])
    # the sum's bar is the element bar on what is summed: |sum a - sum b| <= sum |a - b| <= n BAR max |b|
    e_sum = float((R.sum(1) - Rfx.sum(1)).abs().max() / (S * Rfx.abs().max()))
    print(f"[cp fp32 {model} sparse_top={sparse_top} fold_norm={fold_norm}] batch vs reference fp64: "
          + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f"  sum R_tok {e_sum:.2e}  (the reference's own fp32: {float(fx['err32']):.1e})")
    assert max(errs.values()) <= BAR and e_sum <= BAR
    for b, n in enumerate(LENGTHS):
        assert not out["R_tok"][b, : S - n].any() and out["R_tok"][b, S - n:].any()
    for objective in ("logit", "logprob"):
        g = lambda k: fx[f"span_{objective}/{k}"]          # noqa: E731
        sp = eng.explain(ids[:1], positions=torch.from_numpy(g("positions")), position_weights=torch.from_numpy(g("weights")).float(),
                         objective=objective, layer_relevance=True)
        assert sp["idx"].cpu().tolist() == g("target").tolist()
        errs = {k: nmax(sp[k], g(k)) for k in ("R_tok", "logit", "logprob", "layer_R")}
        print(f"[cp fp32 {model} sparse_top={sparse_top} fold_norm={fold_norm}] span {objective} vs reference fp64: "
              + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert max(errs.values()) <= BAR


def test_engine_vs_dropin():
    _need_gpu()
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "cp_dropin_worker.py")], capture_output=True, text=True, timeout=600, cwd=root)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("model", MODELS)
def test_rule_round_trip_and_graph(engines, model):
    fx = engines[model][1]
    ids = torch.from_numpy(fx["ids"])
    fresh, _ = _engine(model)
    eng, _ = _engine(model)
    assert fresh.rule == eng.rule == "attnlrp"
    want = fresh.explain(ids, lengths=list(LENGTHS), layer_relevance=True)
    eng.set_rule("cp")
    cp = eng.explain(ids, lengths=list(LENGTHS), layer_relevance=True)
    assert torch.equal(cp["logits"], want["logits"]) and nmax(cp["R_tok"], want["R_tok"]) > 1e-3          # the model's forward; another rule
    assert torch.equal(cp["R_tok"], engines[model][0].explain(ids, lengths=list(LENGTHS))["R_tok"])
    g1 = eng.explain(ids, graph=True, layer_relevance=True)
    g1 = {k: v.clone() for k, v in g1.items()}
    eager = eng.explain(ids, layer_relevance=True)
    assert all(torch.equal(g1[k], eager[k]) for k in ("R_tok", "logit", "idx", "layer_R"))
    assert any(key[5] == "cp" for key in eng._graphs.graphs if key[0] != "decode")
    eng.set_rule("attnlrp")
    assert not eng._graphs.graphs
    back = eng.explain(ids, lengths=list(LENGTHS), layer_relevance=True)
    assert all(torch.equal(back[k], want[k]) for k in ("R_tok", "logit", "idx", "layer_R", "logits"))


@pytest.mark.parametrize("model", MODELS)
def test_served_readouts(engines, model):
    eng, fx = engines[model]
    ids, L = torch.from_numpy(fx["ids"]), len(eng.layers)
    plain = eng.explain(ids, lengths=list(LENGTHS))
    out = eng.explain(ids, lengths=list(LENGTHS), layer_relevance=True, return_G=True, latent=("trace", "resid", "mlp"))
    assert torch.equal(out["R_tok"], plain["R_tok"])
    assert out["R_trace"].shape == (L + 1, 3, S) and torch.equal(out["R_trace"][0], out["R_tok"])
    assert nmax(out["R_trace"].sum(-1), out["layer_R"]) <= 1e-5 and nmax(out["R_resid"].sum(-1), out["layer_R"]) <= 1e-5
    assert out["R_mlp"].shape == (L, 3, eng.cfg["inter"]) and torch.isfinite(out["R_mlp"]).all() and out["R_mlp"].any()
    assert nmax((out["G_emb"] * out["emb"]).sum(-1), out["R_tok"]) <= 1e-5
    tgt = (plain["idx"] + 1) % eng.cfg["vocab"]
    by_target = eng.explain(ids, lengths=list(LENGTHS), target=tgt)
    seed = torch.zeros(3, eng.cfg["vocab"]).scatter_(1, tgt.cpu().long()[:, None], 1.0)
    by_seed = eng.explain(ids, lengths=list(LENGTHS), seed=seed)
    assert nmax(by_seed["R_tok"], by_target["R_tok"]) <= 1e-5 and nmax(by_target["R_tok"], plain["R_tok"]) > 1e-3


CFG8B = dict(hidden=4096, inter=14336, n_layers=2, n_heads=32, n_kv=8, head_dim=128, vocab=4096, rope_theta=5e5, rms_eps=1e-5)


def test_bf16_8b_widths():
    """bf16 CP-LRP at the 8B layer widths, two layers, S = 256, against the fp32 CP engine on the same weights.  Yardstick, as in
    tests/test_span_gpu.py::test_bf16_8b_widths_fused_layer: the error of the plain AttnLRP bf16 call against its fp32 engine on the same
    prompt, measured here; CP may be 3 x as far and must point the same way (cosine >= 0.995)"""
    _need_gpu()
    import lxt_amd.engine as E
    H, I, d = 4096, 14336, 128
    g = torch.Generator(device="cuda").manual_seed(3)
    rn = lambda *s: (torch.randn(*s, generator=g, device="cuda") * 0.02).bfloat16()              # noqa: E731
    nw = lambda: (1.0 + 0.1 * torch.randn(H, generator=g, device="cuda")).bfloat16()            # noqa: E731
    W = dict(embed=rn(4096, H), norm=nw(), lm_head=rn(4096, H),
             layers=[dict(ln1=nw(), ln2=nw(), wq=rn(32 * d, H), wk=rn(8 * d, H), wv=rn(8 * d, H), wo=rn(H, 32 * d), wg=rn(I, H), wu=rn(I, H),
                          wd=rn(H, I)) for _ in range(2)])
    bf = E.LlamaLRP(CFG8B, W, dtype=torch.bfloat16, max_seq=256)
    f32 = E.LlamaLRP(CFG8B, W, dtype=torch.float32, max_seq=256)
    ids = torch.randint(0, 4096, (1, 256), generator=torch.Generator().manual_seed(4))
    cos = lambda a, b: float(torch.nn.functional.cosine_similarity(a.double().flatten(), b.double().flatten(), dim=0))   # noqa: E731
    plain = bf.explain(ids)
    yard = nmax(plain["R_tok"], f32.explain(ids, target=plain["idx"])["R_tok"])
    bf.set_rule("cp")
    f32.set_rule("cp")
    for lengths in (None, [200]):
        out = bf.explain(ids, lengths=lengths, target=plain["idx"])
        ref = f32.explain(ids, lengths=lengths, target=plain["idx"])
        e, c = nmax(out["R_tok"], ref["R_tok"]), cos(out["R_tok"], ref["R_tok"])
        print(f"[cp bf16 8B widths B=1 S=256 lengths={lengths}] R_tok vs fp32 CP engine {e:.2e} cosine {c:.5f}; AttnLRP plain call {yard:.2e}")
        assert torch.isfinite(out["R_tok"]).all() and e <= 3 * yard and c >= 0.995
    assert torch.equal(bf.explain(ids, target=plain["idx"])["R_tok"], bf.explain(ids, target=plain["idx"])["R_tok"])


@pytest.mark.parametrize("case", ["qwen2_d64", "qwen3_d128"])
def test_mxfp4_engine_equals_the_engine_on_its_dequantised_weights(case):
    """weight_format="mxfp4" under rule="cp": the V rows of the qkv dgrad are a row slice of the dequantised scratch layer, so the quantised
    engine is bit for bit the plain engine on the weights it dequantises to (tests/test_mxfp4_gpu.py's check, under the other rule)"""
    _need_gpu()
    from lxt_amd.engine_qwen import QwenLRP
    from tests.golden import qwen_models as qm
    q = QwenLRP.from_hf(qm.to_bf16_rotary_fp32(qm.build(case)), max_seq=256, weight_format="mxfp4", rule="cp")
    plain = QwenLRP(*q.dequantized_weights(), max_seq=256, rule="cp")
    assert q.weight_format == "mxfp4" and plain.weight_format is None and q.rule == plain.rule == "cp"
    ids = qm.prompts(case)[:3, :192]
    for kw in (dict(layer_relevance=True), dict(lengths=[192, 100, 17], latent=("trace", "resid", "mlp"))):
        a, b = q.explain(ids, **kw), plain.explain(ids, **kw)
        for k in ("R_tok", "logit", "idx", "layer_R", "R_trace", "R_resid", "R_mlp"):
            assert (k in a) == (k in b) and (k not in a or torch.equal(a[k], b[k])), (case, k)
        assert torch.isfinite(a["R_tok"]).all() and a["R_tok"].any()


@pytest.mark.parametrize("model", MODELS)
def test_explain_generated(engines, model):
    eng, fx = engines[model]
    ids, T = torch.from_numpy(fx["ids"]), 6
    base, _ = _engine(model)
    want = base.generate(ids, T, lengths=list(LENGTHS))
    out = eng.explain_generated(ids, T, lengths=list(LENGTHS), objective="logprob")
    assert torch.equal(out["new_tokens"], want["new_tokens"]) and torch.equal(out["sequences"], want["sequences"])
    pos = torch.arange(S - 1, S + T - 1).expand(3, T)
    hand = eng.explain(out["sequences"], lengths=want["lengths"], positions=pos, objective="logprob")
    assert torch.equal(out["R_tok"], hand["R_tok"]) and torch.equal(out["idx"].long(), want["new_tokens"].long())
    assert nmax(out["R_tok"], base.explain(out["sequences"], lengths=want["lengths"], positions=pos, objective="logprob")["R_tok"]) > 1e-3


def test_refusals_launch_nothing(engines, monkeypatch):
    import lxt_amd.engine as E
    import lxt_amd.ops as ops
    eng, fx = engines["llama"]
    ids = torch.from_numpy(fx["ids"])

    def ran(*a, **k):
        raise AssertionError("a kernel of the model ran")

    monkeypatch.setattr(eng, "forward", ran)
    for name in ("attn_bwd_dv", "gated_cp_bwd_il", "attn_fwd", "linear_fwd", "linear_dgrad"):
        monkeypatch.setattr(ops, name, ran)
    for kw in (dict(heads=("out",)), dict(attn_map="sum"), dict(attn_map=[(0, 1)]), dict(weights=("o",))):
        with pytest.raises(ValueError):
            eng.explain(ids, **kw)
    with pytest.raises(ValueError):
        eng.set_mode("explicit")
    assert eng.mode == "efficient" and eng.rule == "cp"
    with pytest.raises(ValueError):
        eng.set_rule("lrp")
    assert eng.rule == "cp"
    for kw in (dict(rule="lrp"), dict(rule="cp", mode="explicit"), dict(rule=None)):
        with pytest.raises(ValueError):
            E.LlamaLRP(eng.cfg, None, dtype=torch.float32, **kw)
