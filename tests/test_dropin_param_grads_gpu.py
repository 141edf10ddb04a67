"""GPU: parameter gradients of TRAINABLE models under lxt_amd.efficient.monkey_patch: after logit.backward() every
parameter has the .grad the reference leaves, from lrp_wgrad / lrp_colsum_affine, and the frozen path is what it was.
  (1) Llama fp32, two prompts without zero_grad: w * w.grad of every decoder Linear against weight_relevance_llama_l*.npz, every parameter
      has a gradient, the norm weights' against param_grads_llama.npz;
  (2) Qwen2 / Qwen3 / Gemma-3 / BERT / GPT-2 in a worker process each (tests/param_grad_worker.py) against param_grads_<family>*.npz;
  (3) the input relevance of a frozen and of a trainable Llama is bitwise equal (per-module patches, fp32 and bf16);
  (4) bf16 gradients against the fp32 model on the same bf16-rounded weights at the project's bf16 bar;
  (5) a foreign (not adopted) nn.Linear / nn.LayerNorm with trainable parameters keeps ATen's forward and gradients bit for bit.
The Llama model is patched in this process (other GPU tests patch modeling_llama here as well); the other families run in workers."""
import os
import subprocess
import sys
import warnings

import pytest
import torch

from oracle import llama as ol
from tests.golden.hf_models import build_llama_from_weights
from tests.golden.make_golden_param_grads import CFG, WSEED, build, explain
from tests.util import load, nmax, t

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
FP32_BAR, BF16_BAR, BF16_COS = 1e-4, 5e-2, 0.995              # the project's bars (test_engine_fp32_vs_reference, test_engine_bf16_8b_dims)


@pytest.fixture(scope="module")
def patched():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from transformers.models.llama import modeling_llama
    from lxt_amd.efficient import monkey_patch, patches
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        monkey_patch(modeling_llama)
    return patches


def _trainable(model, flag=True):
    for p in model.parameters():
        p.requires_grad_(flag)
    return model


def _input_relevance(model, ids, target=None):
    """the quickstart protocol on a detached embedding -> (idx, e.grad); parameter gradients (if any) stay on the model"""
    e = model.get_input_embeddings()(ids[None]).detach().requires_grad_()
    last = model(inputs_embeds=e, use_cache=False).logits[0, -1]
    idx = int(last.argmax()) if target is None else target
    last[idx].backward()
    return idx, e.grad


def _count_calls(monkeypatch, names=("wgrad", "colsum_affine")):
    """-> {name: calls} of the library wrappers behind the parameter gradients (the gradients must come from liblrp_hip.so, not from ATen)"""
    from lxt_amd import ops
    calls = dict.fromkeys(names, 0)

    def spy(name, fn):
        def wrapped(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapped
    for name in names:
        monkeypatch.setattr(ops, name, spy(name, getattr(ops, name)))
    return calls


def test_llama_fp32_every_parameter_gets_the_reference_gradient(patched, monkeypatch):
    fx, prompts = load("param_grads_llama.npz"), load("weight_relevance_llama_prompts.npz")
    calls = _count_calls(monkeypatch)
    model = build("llama").cuda()
    assert all(p.requires_grad for p in model.parameters())
    for b, row in enumerate(t(fx["ids"]).cuda()):
        idx, logit = explain(model, row, zero=False)                                     # the second prompt ADDS to the first one's gradients
        assert idx == int(fx["idx"][b]) == int(prompts["idx"][b]) and abs(logit - float(fx["logit"][b])) < 1e-4
    named = dict(model.named_parameters())
    missing = [n for n, p in named.items() if p.grad is None]
    assert not missing, missing                                                          # (the norm weights on the parent commit)
    n_lin, n_norm = 7 * CFG["n_layers"] + 1, 2 * CFG["n_layers"] + 1                     # decoder Linears + the head; layer norms + the final norm
    assert calls == dict(wgrad=2 * n_lin, colsum_affine=2 * n_norm), calls               # one library launch per parameter and prompt, none on ATen
    assert all(p.grad.shape == p.shape and p.grad.dtype == p.dtype and p.grad.device == p.device for p in named.values())
    rel = lambda lin: (lin.weight * lin.weight.grad).detach()                            # noqa: E731
    worst = 0.0
    for l, L in enumerate(model.model.layers):
        ref = load(f"weight_relevance_llama_l{l}.npz")
        a, m = L.self_attn, L.mlp
        got = dict(qkv=torch.cat([rel(a.q_proj), rel(a.k_proj), rel(a.v_proj)]), o=rel(a.o_proj),
                   gate_up=torch.cat([rel(m.gate_proj), rel(m.up_proj)]), down=rel(m.down_proj))
        for n, v in got.items():
            err = nmax(v, ref[n])
            print(f"[llama fp32 trainable] layer {l} {n}: w * w.grad vs the reference, normalised max {err:.2e}")
            worst = max(worst, err)
    for k, g in fx.items():
        if k.startswith("g:"):
            err = nmax(named[k[2:]].grad, g)
            print(f"[llama fp32 trainable] {k[2:]}: grad vs the reference, normalised max {err:.2e}")
            worst = max(worst, err)
    assert worst <= FP32_BAR, worst


@pytest.mark.parametrize("family", ["qwen2", "qwen3", "gemma3", "bert", "gpt2"])
def test_family_parameter_gradients(family):
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "param_grad_worker.py"), family], capture_output=True, text=True,
                       timeout=600, cwd=root)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_frozen_path_is_untouched(patched, monkeypatch, dtype):
    """the per-module patches of a frozen and of a trainable model run the same forward and dgrad kernels: bitwise equal input relevance"""
    monkeypatch.setattr(patched, "FUSE_LAYER", False)
    monkeypatch.setattr(patched, "FUSE_MLP", False)
    W = ol.random_weights(CFG, seed=WSEED)
    ids = t(load("param_grads_llama.npz")["ids"])[0].cuda()
    frozen = build_llama_from_weights(CFG, W, dtype=dtype, rotary_fp32=True).cuda()
    assert not any(p.requires_grad for p in frozen.parameters())
    idx, g_frozen = _input_relevance(frozen, ids)
    assert all(p.grad is None for p in frozen.parameters())
    train = _trainable(build_llama_from_weights(CFG, W, dtype=dtype, rotary_fp32=True).cuda())
    idx2, g_train = _input_relevance(train, ids)
    assert idx == idx2 and torch.isfinite(g_frozen).all() and float(g_frozen.abs().max()) > 0
    assert torch.equal(g_frozen, g_train)
    assert all(p.grad is not None for n, p in train.named_parameters() if "embed_tokens" not in n)      # (the embedding was detached)


def _cosine(a, b):
    return float(torch.nn.functional.cosine_similarity(a.double().flatten(), b.double().flatten(), dim=0))


def test_llama_bf16_gradients_vs_fp32_on_the_rounded_weights(patched, monkeypatch):
    """hidden 128 (a multiple of 8; every Linear of this config is on lrp_wgrad's bf16 grid); the fp32 model carries the bf16-rounded weights"""
    calls = _count_calls(monkeypatch)
    W = ol.random_weights(CFG, seed=WSEED)
    Wr = ol.cast_weights(ol.cast_weights(W, BF16), F32)
    ids = t(load("param_grads_llama.npz")["ids"])[0].cuda()
    m32 = _trainable(build_llama_from_weights(CFG, Wr, dtype=F32).cuda())
    idx, _ = _input_relevance(m32, ids)
    m16 = _trainable(build_llama_from_weights(CFG, Wr, dtype=BF16, rotary_fp32=True).cuda())
    _input_relevance(m16, ids, target=idx)
    ref = dict(m32.named_parameters())
    worst, cos = 0.0, 1.0
    for n, p in m16.named_parameters():
        if "embed_tokens" in n:
            continue
        assert p.grad is not None and p.grad.dtype == BF16 and p.grad.shape == p.shape and torch.isfinite(p.grad).all(), n
        if p.dim() == 2:
            e, c = nmax(p.grad.float(), ref[n].grad), _cosine(p.grad.float(), ref[n].grad)
            print(f"[llama bf16 trainable] {n}: normalised max {e:.2e} cosine {c:.5f}")
            worst, cos = max(worst, e), min(cos, c)
    assert calls["wgrad"] == 2 * (7 * CFG["n_layers"] + 1), calls                        # both models' Linears on lrp_wgrad
    assert worst <= BF16_BAR and cos >= BF16_COS, (worst, cos)


def test_foreign_modules_keep_aten(patched):
    """nn.Linear / nn.LayerNorm are patched class-wide; an instance outside an adopted model runs torch's own forward, trainable or not"""
    F = torch.nn.functional
    torch.manual_seed(3)
    lin, ln = torch.nn.Linear(64, 48).cuda(), torch.nn.LayerNorm(48).cuda()
    with torch.no_grad():
        ln.weight.normal_(1.0, 0.1)
        ln.bias.normal_(0.0, 0.1)
    assert not lin.__dict__.get("_lrp_owned") and all(p.requires_grad for p in list(lin.parameters()) + list(ln.parameters()))
    x = torch.randn(5, 7, 64, device="cuda")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                                  # (the one-time notice about un-adopted LayerNorms)
        xa = x.clone().requires_grad_()
        ya = ln(lin(xa))
        ya.square().sum().backward()
    got = [xa.grad] + [p.grad.clone() for p in (lin.weight, lin.bias, ln.weight, ln.bias)]
    xb = x.clone().requires_grad_()
    ps = [p.detach().clone().requires_grad_() for p in (lin.weight, lin.bias, ln.weight, ln.bias)]
    yb = F.layer_norm(F.linear(xb, ps[0], ps[1]), (48,), ps[2], ps[3], ln.eps)
    yb.square().sum().backward()
    assert torch.equal(ya, yb)
    for a, b in zip(got, [xb.grad] + [p.grad for p in ps]):
        assert torch.equal(a, b)
