"""CPU: the decode site entry of include/lrp_hip_decode_site.h is declared, exported and validates its arguments before any launch (host
pointers only); the generate_gemma3 / span_gemma3 fixtures hold what their generators assert; Gemma3LRP carries the span and generation
keywords of LlamaLRP."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests.util import load

EINVAL, EALIGN, ESHAPE = -1, -2, -3
NAME = "lrp_decode_qknorm_rope_append"


def test_site_symbol_declared_in_its_own_header_and_exported():
    import lxt_amd._lib as L
    decls = L.parse_header()
    raw = ctypes.CDLL(L.LIB_PATH)
    assert NAME in decls, f"{NAME} is not declared in a header lrp_hip.h includes"
    assert hasattr(raw, NAME), f"{NAME} declared but not exported"
    assert decls[NAME][0] == "int" and len(decls[NAME][1]) == 24
    inc = os.path.dirname(L.HEADER_PATH)
    with open(L.HEADER_PATH) as f:
        top = f.read()
    with open(os.path.join(inc, "lrp_hip_decode_site.h")) as f:
        site = f.read()
    assert '#include "lrp_hip_decode_site.h"' in top and NAME in site and NAME + "(" not in top
    assert L.lib.lrp_version() == 8


def test_site_argument_ladder_without_gpu():
    """NULL -> EINVAL, shapes -> ESHAPE, the 16-byte grid -> EALIGN, in that order and all of it before a launch: the pointers are host
    integers that no kernel may ever see"""
    import lxt_amd._lib as L
    lib, F32, BF16 = L.lib, L.F32, L.BF16
    P = 4096          # "pointers" on the 16-byte grid

    def call(qk=P, ldqk=6 * 64, v=P, ldv=2 * 64, wq=P, wk=P, cos=P, sin=P, rows=64, pos=P, q_rot=P, ldq=4 * 64, kc=P, vc=P, ldc=2 * 64, B=2,
             cap=16, nq=4, nk=2, d=64, dtype=BF16):
        return lib.lrp_decode_qknorm_rope_append(qk, ldqk, v, ldv, wq, wk, 1e-6, 1.0, cos, sin, rows, pos, q_rot, ldq, kc, vc, ldc, B, cap, nq,
                                                 nk, d, dtype, None)

    for name in ("qk", "v", "wq", "wk", "cos", "sin", "pos", "q_rot", "kc", "vc"):
        assert call(**{name: None}) == EINVAL, name
    for kw in (dict(B=-1), dict(nq=0), dict(nk=0), dict(cap=0), dict(rows=0), dict(dtype=7)):
        assert call(**kw) == EINVAL, kw
    # (NULL wins over a bad shape, a bad shape over a bad alignment)
    assert call(wq=None, d=3) == EINVAL and call(d=3, kc=P + 2) == ESHAPE and call(d=24, wk=P + 8) == ESHAPE
    # head dims: what lrp_decode_rope_append AND lrp_head_rmsnorm_fwd take -- whole 16-byte vectors, a power of two of them, d <= 256
    for kw in (dict(d=0), dict(d=63), dict(d=260), dict(d=4), dict(d=12), dict(d=24), dict(d=48), dict(d=96), dict(d=512),
               dict(d=12, dtype=F32), dict(d=2, dtype=F32), dict(d=512, dtype=F32),
               dict(ldqk=6 * 64 - 8), dict(ldv=2 * 64 - 8), dict(ldq=4 * 64 - 8), dict(ldc=2 * 64 - 8)):
        assert call(**kw) == ESHAPE, kw
    # (every accepted call here has B = 0: nothing may launch on these pointers)
    for d in (8, 16, 32, 64, 128, 256):
        assert call(d=d, ldqk=6 * d, ldv=2 * d, ldq=4 * d, ldc=2 * d, B=0) == 0, d
    for d in (4, 8, 16, 32, 64, 128, 256):
        assert call(d=d, dtype=F32, ldqk=6 * d, ldv=2 * d, ldq=4 * d, ldc=2 * d, B=0) == 0, d
    for name in ("qk", "v", "wq", "wk", "q_rot", "kc", "vc", "cos", "sin"):
        assert call(**{name: P + 8}) == EALIGN, name
    assert call(pos=P + 2) == EALIGN and call(pos=P + 4, B=0) == 0
    for kw in (dict(ldqk=6 * 64 + 4), dict(ldv=2 * 64 + 4), dict(ldq=4 * 64 + 4), dict(ldc=2 * 64 + 4)):
        assert call(**kw) == EALIGN, kw
    assert call(ldc=2 * 64 + 2, dtype=F32) == EALIGN and call(ldc=2 * 64 + 4, dtype=F32, B=0) == 0
    assert call(B=0) == 0                                    # nothing to do, nothing launched


def test_ops_wrapper_refuses_host_tensors_and_foreign_weights():
    import lxt_amd.ops as ops
    q, kc = torch.zeros(2, 4 * 32), torch.zeros(2, 8, 2 * 32)
    pos, w, tab = torch.zeros(1, dtype=torch.int32), torch.zeros(32), torch.zeros(8, 32)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.decode_qknorm_rope_append(torch.zeros(2, 6 * 32), torch.zeros(2, 2 * 32), w, w, 1e-6, tab, tab, pos, q, kc, kc.clone(), 4, 2, 32, 1.0)


def test_generate_fixture_holds_what_the_generator_asserts():
    from tests.golden import make_golden_generate as gg
    from tests.golden import make_golden_generate_gemma3 as g3
    from tests.golden.hf_models import wsum
    fx = load("generate_gemma3.npz")
    B, S, T = gg.B, gg.S, gg.NEW
    V = fx["logits"].shape[-1]
    assert fx["ids"].shape == (B, S) and fx["tokens"].shape == (B, T) and fx["logits"].shape == (B, T, V) and fx["logits"].dtype == np.float64
    assert tuple(fx["lengths"]) == gg.LENGTHS == (24, 15, 7)
    assert np.array_equal(fx["ids"], g3.prompts(V).numpy()), "the seeded prompts did not reproduce"
    assert np.array_equal(fx["logits"].argmax(-1), fx["tokens"])
    top2 = np.sort(fx["logits"], -1)[..., -2:]
    margin = float((top2[..., 1] - top2[..., 0]).min())
    assert margin == float(fx["margin"]) and margin >= 2e-4
    assert min(len(set(row.tolist())) for row in fx["tokens"]) >= 12          # (no continuation collapsed to a few repeated tokens)
    model = g3.build()
    got = wsum(model)
    assert abs(got - float(fx["wsum"])) <= 1e-9 * got, "the seeded weights did not reproduce"
    # the norm weights are not HF's zeros, and the two longer prompts grow past the window
    assert float(model.model.layers[0].self_attn.q_norm.weight.abs().max()) > 0 and float(model.model.norm.weight.abs().max()) > 0
    w = int(fx["window"])
    assert w == model.config.sliding_window and sorted(n + T > w for n in gg.LENGTHS) == [False, True, True]
    # HF in fp32 reproduces the fp64 tokens (the shortest prompt: the whole protocol on 7 + 24 tokens)
    toks, logits = gg.greedy(model, torch.from_numpy(fx["ids"])[2, S - 7:], T)
    assert np.array_equal(toks, fx["tokens"][2])
    assert np.abs(logits - fx["logits"][2]).max() <= 1e-5 * np.abs(fx["logits"][2]).max()


def test_span_fixture_holds_what_the_generator_asserts():
    from tests.golden import make_golden_span as gs
    fx = load("span_gemma3.npz")
    S = int(fx["S"])
    assert S == gs.S == 48 and int(fx["window"]) == 32
    assert fx["a/positions"].tolist() == [list(gs.POS_A)] and fx["c/positions"].tolist() == [list(p) for p in gs.POS_C]
    assert fx["c/lengths"].tolist() == list(gs.LENGTHS_C) and str(fx["b/objective"]) == "logprob" and str(fx["a/objective"]) == "logit"
    assert fx["d/R_tok"].shape == (len(gs.POS_A), 1, S)
    # positions on both sides of the window
    assert min(gs.POS_A) < int(fx["window"]) <= max(gs.POS_A)
    # linearity of the reference itself: case a is the sum of case d's rows
    lin = np.abs(fx["d/R_tok"].sum(0) - fx["a/R_tok"]).max() / np.abs(fx["a/R_tok"]).max()
    lin_l = np.abs(fx["d/layer_R"].sum(0) - fx["a/layer_R"]).max() / np.abs(fx["a/layer_R"]).max()
    assert lin <= 1e-10 and lin_l <= 1e-10, (lin, lin_l)
    # pads are 0 and nothing lies above the highest explained column
    for b, n in enumerate(gs.LENGTHS_C):
        assert not fx["c/R_tok"][b, : S - n].any() and not fx["c/R_tok"][b, max(gs.POS_C[b]) + 1:].any() and fx["c/R_tok"][b].any()
    assert np.allclose(fx["a/logprob"], fx["b/logprob"]) and fx["a/target"].tolist() == fx["b/target"].tolist()


def test_gemma3_driver_carries_the_keywords():
    from lxt_amd.engine import LlamaLRP
    from lxt_amd.engine_gemma3 import Gemma3LRP
    ex = inspect.signature(Gemma3LRP.explain).parameters
    for k, default in (("positions", None), ("position_weights", None), ("objective", "logit"), ("per_position", False)):
        assert k in ex and ex[k].default == default, k
    assert "span" in inspect.signature(Gemma3LRP.explain_emb).parameters
    assert inspect.signature(Gemma3LRP.explain_emb).parameters["span"].default is None
    for name in ("generate", "explain_generated"):
        assert list(inspect.signature(getattr(Gemma3LRP, name)).parameters) == list(inspect.signature(getattr(LlamaLRP, name)).parameters), name
        mine, theirs = inspect.signature(getattr(Gemma3LRP, name)).parameters, inspect.signature(getattr(LlamaLRP, name)).parameters
        assert all(mine[k].default == theirs[k].default for k in mine), name


def test_span_and_generate_refusals_need_no_device():
    """readout_requests stays the first check; then the span request, then the inputs: a stub without weights raises the request's
    ValueError"""
    from lxt_amd.engine_gemma3 import Gemma3LRP
    stub = Gemma3LRP.__new__(Gemma3LRP)
    stub.cfg, stub.dtype, stub.max_seq = dict(hidden=64, inter=128, vocab=32, head_dim=32, n_heads=2), torch.float32, 16
    ids = torch.zeros(1, 8, dtype=torch.long)
    with pytest.raises(ValueError, match="latent"):
        stub.explain(ids, latent="neurons", positions=[[9]])
    for kw in (dict(positions=[[8]]), dict(positions=[[1, 1]]), dict(objective="prob"), dict(per_position=True), dict(position_weights=[[1.0]]),
               dict(positions=[[1]], per_position=True, layer_relevance=True), dict(positions=[[1, 2]], target=[[1, 32]])):
        with pytest.raises(ValueError):
            stub.explain(ids, **kw)
    for kw in (dict(max_new_tokens=0), dict(max_new_tokens=9), dict(lengths=[9]), dict(eos_token_id=32), dict(inputs_embeds=torch.zeros(1, 8, 64))):
        with pytest.raises(ValueError):
            stub.generate(**dict(dict(input_ids=ids, max_new_tokens=2), **kw))
