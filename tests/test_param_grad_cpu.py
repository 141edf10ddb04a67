"""CPU: the parameter-gradient fixtures (tests/golden/make_golden_param_grads.py: the REAL lxt.efficient in fp64, every parameter trainable)
load, name their protocol and describe the models the GPU tests rebuild; the Llama one is the model of the weight_relevance_llama_* fixtures."""
import os

import numpy as np
import pytest
import torch

from tests.util import GOLDEN, load

FILES = ["llama", "qwen2", "qwen2_top", "qwen3", "qwen3_top", "gemma3", "gemma3_top", "bert", "gpt2", "gpt2_top"]
# what each family's fixture is there for (a name fragment, dimensions of the arrays)
EXERCISES = dict(qwen2=("q_proj.bias", 1), qwen3=("q_norm.weight", 1), gemma3=("pre_feedforward_layernorm.weight", 1), bert=("LayerNorm.bias", 1),
                 gpt2=("c_attn.weight", 2), gpt2_top=("mlp.c_proj.weight", 2))


@pytest.mark.parametrize("name", FILES)
def test_fixture_loads(name):
    path = os.path.join(GOLDEN, f"param_grads_{name}.npz")
    assert os.path.getsize(path) < (1 << 20)
    fx = load(f"param_grads_{name}.npz")
    assert "lxt.efficient.monkey_patch" in str(fx["protocol"]) and "fp64" in str(fx["protocol"]) and "requires_grad" in str(fx["protocol"])
    grads = {k[2:]: v for k, v in fx.items() if k.startswith("g:")}
    assert grads and all(v.dtype == np.float32 and np.isfinite(v).all() for v in grads.values())
    assert fx["ids"].ndim == 2 and np.isfinite(fx["logit"]).all() and float(fx["wsum"]) > 0
    assert sum(float(np.abs(v).max()) > 0 for v in grads.values()) == len(grads)           # no parameter is dead
    if name in EXERCISES:
        frag, dim = EXERCISES[name]
        hits = [v for k, v in grads.items() if frag in k]
        assert hits and all(v.ndim == dim for v in hits), frag
    if name.endswith("_top"):
        main = load(f"param_grads_{name[:-4]}.npz")
        assert np.array_equal(main["ids"], fx["ids"]) and int(main["idx"]) == int(fx["idx"]) and float(main["logit"]) == float(fx["logit"])


def test_gpt2_gradients_are_in_the_stored_layout():
    """HF's Conv1D keeps W as [in, out]: c_attn of n_embd 128 is [128, 384], and so is its gradient"""
    fx = load("param_grads_gpt2.npz")
    assert fx["g:transformer.h.0.attn.c_attn.weight"].shape == (128, 384) and fx["g:transformer.h.0.mlp.c_fc.weight"].shape == (128, 512)
    assert fx["g:transformer.h.0.mlp.c_proj.weight"].shape == (512, 128) and fx["g:transformer.h.0.attn.c_attn.bias"].shape == (384,)


def test_llama_fixture_is_the_weight_relevance_model():
    from oracle import llama as ol
    fx, wr = load("param_grads_llama.npz"), load("weight_relevance_llama_prompts.npz")
    assert np.array_equal(fx["ids"], wr["ids"]) and np.array_equal(fx["idx"], wr["idx"]) and np.array_equal(fx["logit"], wr["logit"])
    assert int(fx["wseed"]) == int(wr["wseed"]) and np.array_equal(fx["iseeds"], wr["iseeds"])
    cfg = {k: (float(v) if k in ("rope_theta", "rms_eps") else int(v)) for k, v in zip(wr["cfg_keys"].tolist(), wr["cfg_vals"].tolist())}
    W = ol.random_weights(cfg, seed=int(fx["wseed"]))
    names = [k[2:] for k in fx if k.startswith("g:")]
    assert len(names) == 2 * cfg["n_layers"] + 1                                           # the norm weights, nothing else
    for l, Lw in enumerate(W["layers"]):
        for key, norm in (("ln1", "input_layernorm"), ("ln2", "post_attention_layernorm")):
            n = f"model.layers.{l}.{norm}.weight"
            g = torch.from_numpy(fx[f"g:{n}"]).double()
            per = torch.from_numpy(fx[f"p0:{n}"]).double() + torch.from_numpy(fx[f"p1:{n}"]).double()
            # "g:" is the fp64 sum over the two prompts, each of the three stored with one fp32 rounding
            assert float((g - per).abs().max()) <= 3 * 2.0 ** -24 * float(torch.from_numpy(fx[f"p0:{n}"]).abs().max() + torch.from_numpy(fx[f"p1:{n}"]).abs().max())
            rel = float((Lw[key].double() * g).sum())                                      # the relevance of the norm's weight vector
            assert np.isfinite(rel) and rel != 0.0, n
    rel = float((W["norm"].double() * torch.from_numpy(fx["g:model.norm.weight"]).double()).sum())
    assert np.isfinite(rel) and rel != 0.0
