"""CPU: lrp_sample_rows (include/lrp_hip_sample.h) is declared in its own header, exported, and validates its arguments before any launch
(host integers as pointers); ops.sample_rows refuses host tensors; the numpy restatement of the definition (tests/sample_oracle.py) keeps
HF's kept sets and reproduces the Philox known-answer vector; engine.sample_request refuses what it must without a device; the drivers
carry the six sampling keywords."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests import sample_oracle as so

EINVAL, EALIGN, ESHAPE = -1, -2, -3
NAME = "lrp_sample_rows"
SAMPLING_KW = (("do_sample", False), ("temperature", 1.0), ("top_k", 0), ("top_p", 1.0), ("min_p", 0.0), ("seed", None))


def test_symbol_declared_in_its_own_header_and_exported():
    import lxt_amd._lib as L
    decls = L.parse_header()
    raw = ctypes.CDLL(L.LIB_PATH)
    assert NAME in decls, f"{NAME} is not declared in a header lrp_hip.h includes"
    assert hasattr(raw, NAME), f"{NAME} declared but not exported"
    assert decls[NAME][0] == "int" and len(decls[NAME][1]) == 17
    assert decls[NAME][1][8] == "int64_t*"
    inc = os.path.dirname(L.HEADER_PATH)
    with open(L.HEADER_PATH) as f:
        top = f.read()
    with open(os.path.join(inc, "lrp_hip_sample.h")) as f:
        mine = f.read()
    assert '#include "lrp_hip_sample.h"' in top and NAME in mine and NAME + "(" not in top
    assert L.lib.lrp_version() == 8


def test_argument_ladder_without_gpu():
    """EINVAL, then ESHAPE, then EALIGN, all before a launch: the pointers are host integers that no kernel may ever see, and every accepted
    call has B = 0"""
    import lxt_amd._lib as L
    P = 4096

    def call(logits=P, ld=100, B=2, V=100, T=1.0, top_k=0, top_p=1.0, min_p=0.0, seeds=P, streams=P, step=0, u_in=None, idx=P, slp=P, n_kept=P,
             u_out=P):
        return L.lib.lrp_sample_rows(logits, ld, B, V, T, top_k, top_p, min_p, seeds, streams, step, u_in, idx, slp, n_kept, u_out, None)

    assert call(logits=None) == EINVAL and call(idx=None) == EINVAL and call(seeds=None, u_in=None) == EINVAL
    for kw in (dict(B=-1), dict(V=0), dict(T=0.0), dict(T=-1.0), dict(T=float("inf")), dict(T=float("nan")), dict(top_k=-1), dict(top_p=0.0),
               dict(top_p=-0.5), dict(top_p=float("nan")), dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=float("nan")), dict(step=-1)):
        assert call(**kw) == EINVAL, kw
    # (a bad value wins over a bad shape, a bad shape over a bad alignment)
    assert call(T=0.0, ld=99) == EINVAL and call(ld=99) == ESHAPE and call(ld=99, idx=P + 2) == ESHAPE
    for name in ("logits", "streams", "idx", "slp", "n_kept", "u_out"):
        assert call(**{name: P + 2}) == EALIGN, name
    assert call(u_in=P + 1) == EALIGN and call(seeds=P + 4) == EALIGN
    # accepted: nothing to do, nothing launched -- off the 16-byte grid, a pitch, every optional pointer absent, either source of u
    assert call(B=0) == 0 and call(B=0, logits=P + 4, ld=101) == 0
    assert call(B=0, streams=None, slp=None, n_kept=None, u_out=None) == 0
    assert call(B=0, seeds=None, u_in=P) == 0 and call(B=0, seeds=P + 8, u_in=P + 4) == 0
    assert call(B=0, T=0.05, top_k=10 ** 6, top_p=5.0, min_p=1.0, step=2 ** 31 - 1) == 0


def test_ops_wrapper_refuses_host_tensors_and_bad_arguments():
    import lxt_amd.ops as ops
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.sample_rows(torch.zeros(2, 8), seeds=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.sample_rows(torch.zeros(8), seeds=torch.zeros(1, dtype=torch.int64))


def test_philox_known_answer():
    """the restatement, written from the round function, reproduces the Random123 vector the issue quotes from memory -- and two more of that
    suite, so that a restatement that ignored its key or its counter could not pass"""
    assert so.philox4x32_10((0, 0), (0, 0, 0, 0)) == so.KNOWN_ANSWER_ZERO
    ones = 0xFFFFFFFF
    assert so.philox4x32_10((ones, ones), (ones, ones, ones, ones)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert so.philox4x32_10((0xA4093822, 0x299F31D0), (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344)) == (0xD16CFE09, 0x94FDCCEB, 0x5001E420,
                                                                                                           0x24126EA1)
    us = [so.uniform(0x1234567887654321, t, s) for t in range(4) for s in range(3)]
    assert all(0.0 <= u < 1.0 and np.float32(u) == u for u in us) and len(set(us)) == len(us)
    assert so.uniform(-1, 0) == so.uniform(2 ** 64 - 1, 0)


SETTINGS = (dict(temperature=0.7, top_k=20), dict(temperature=1.0, top_p=0.9), dict(temperature=0.6, min_p=0.05),
            dict(temperature=0.7, top_k=20, top_p=0.8, min_p=0.02), dict(temperature=5.0, top_k=50, top_p=0.95), dict(temperature=0.05, top_p=0.5))


def hf_kept(row, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0):
    from transformers.generation import logits_process as lp
    ws = [lp.TemperatureLogitsWarper(float(np.float32(temperature)))]
    if top_k:
        ws.append(lp.TopKLogitsWarper(top_k))
    if top_p < 1:
        ws.append(lp.TopPLogitsWarper(float(np.float32(top_p))))
    if min_p:
        ws.append(lp.MinPLogitsWarper(float(np.float32(min_p))))
    s = torch.from_numpy(row)[None]
    for w in ws:
        s = w(None, s)
    return (s[0] > -float("inf")).numpy()


def test_oracle_kept_sets_equal_hf_warpers():
    """fp64 rows through HF's Temperature / TopK / TopP / MinP warpers in HF's order: the kept sets are the oracle's, with ties across the
    k-th place and -inf entries among the rows"""
    rng, n = np.random.default_rng(11), 0
    for V in (257, 5000):
        for kw in SETTINGS:
            for kind in range(4):
                row = 3.0 * rng.standard_normal(V)
                if kind == 2:
                    row = np.round(row * 4) / 4
                if kind == 3:
                    row[rng.random(V) < 0.3] = -np.inf
                if kind == 2 and "top_p" in kw:
                    continue          # (HF's top-p breaks a tie group by sort order; the definition keeps or drops it whole)
                got = so.sample_row(row, 0.5, **kw)
                assert np.array_equal(got["kept"], hf_kept(row, **kw)), (V, kw, kind)
                assert got["n_kept"] == int(got["kept"].sum()) and got["kept"][got["token"]]
                n += 1
    assert n >= 40


def test_oracle_draw_is_the_inverse_cdf():
    row = np.log(np.array([0.1, 0.2, 0.3, 0.4]))
    for u, tok in ((0.0, 0), (0.0999, 0), (0.1001, 1), (0.2999, 1), (0.3001, 2), (0.6001, 3), (1 - 2.0 ** -24, 3)):
        assert so.sample_row(row, u)["token"] == tok, u
    r = so.sample_row(row, 0.35, top_k=2)          # kept {2, 3}: 3/7, 4/7
    assert r["n_kept"] == 2 and r["token"] == 2 and abs(r["logprob"] - np.log(3 / 7)) < 1e-12
    assert so.sample_row(row, 0.5, top_p=0.5)["n_kept"] == 2 and so.sample_row(row, 0.5, top_p=0.4)["n_kept"] == 2
    assert so.sample_row(row, 0.5, top_p=0.39)["n_kept"] == 1 and so.sample_row(row, 0.9, min_p=0.6)["n_kept"] == 2
    tie = np.array([1.0, 3.0, 3.0, 0.0])
    assert [so.sample_row(tie, u, top_k=1)["token"] for u in (0.0, 0.7)] == [1, 1] and so.sample_row(tie, 0.7, top_k=1)["n_kept"] == 2
    assert so.sample_row(np.array([0.0, 0.0]), 0.5)["near"] and not so.sample_row(np.array([0.0, 0.0]), 0.0)["near"]


def test_sample_request():
    from lxt_amd.engine import sample_request as sr
    assert sr(False, 1.0, 0, 1.0, 0.0, None, 3, None) is None
    for kw in (dict(temperature=0.7), dict(top_k=5), dict(top_p=0.9), dict(min_p=0.1), dict(seed=1)):
        a = dict(dict(do_sample=False, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, seed=None, B=3, force_tokens=None), **kw)
        with pytest.raises(ValueError):
            sr(**a)
    ok = dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.9, min_p=0.05, seed=7, B=3, force_tokens=None)
    for kw in (dict(seed=None), dict(force_tokens=[[1], [2], [3]]), dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")),
               dict(temperature=float("nan")), dict(top_k=-1), dict(top_k=2.0), dict(top_k=True), dict(top_p=0.0), dict(top_p=1.5),
               dict(min_p=-0.1), dict(min_p=1.1), dict(seed=1.5), dict(seed=[1, 2]), dict(seed=[1, 2, 3.0]), dict(seed="7"), dict(seed=True)):
        with pytest.raises(ValueError):
            sr(**dict(ok, **kw))
    s = sr(**ok)
    assert (s.temperature, s.top_k, s.top_p, s.min_p) == (0.7, 20, 0.9, 0.05)
    assert s.seeds.dtype == torch.int64 and s.seeds.tolist() == [7, 7, 7] and s.streams.dtype == torch.int32 and s.streams.tolist() == [0, 1, 2]
    assert not s.seeds.is_cuda and not s.streams.is_cuda
    s = sr(**dict(ok, seed=[5, 2 ** 63 + 1, -1]))
    assert s.seeds.tolist() == [5, -2 ** 63 + 1, -1] and s.streams.tolist() == [0, 0, 0]
    assert sr(**dict(ok, top_p=1.0, min_p=1.0, top_k=0)).top_p == 1.0


def test_drivers_carry_the_sampling_keywords():
    from lxt_amd.engine import LlamaLRP, greedy_decode
    from lxt_amd.engine_gemma3 import Gemma3LRP
    from lxt_amd.engine_qwen import QwenLRP
    for cls in (LlamaLRP, QwenLRP, Gemma3LRP):
        for name, after in (("generate", "force_tokens"), ("explain_generated", "position_weights")):
            names = list(inspect.signature(getattr(cls, name)).parameters)
            i = names.index(after)
            assert tuple(names[i + 1: i + 7]) == tuple(k for k, _ in SAMPLING_KW), (cls.__name__, name)
            par = inspect.signature(getattr(cls, name)).parameters
            assert all(par[k].default == d and type(par[k].default) is type(d) for k, d in SAMPLING_KW), (cls.__name__, name)
    par = inspect.signature(greedy_decode).parameters
    assert list(par)[-1] == "sampler" and par["sampler"].default is None


def test_generate_refuses_sampling_requests_without_a_device():
    """a stub without weights: the request's ValueError comes first"""
    from lxt_amd.engine_gemma3 import Gemma3LRP
    stub = Gemma3LRP.__new__(Gemma3LRP)
    stub.cfg, stub.dtype, stub.max_seq = dict(hidden=64, inter=128, vocab=32, head_dim=32, n_heads=2), torch.float32, 16
    ids = torch.zeros(1, 8, dtype=torch.long)
    for kw in (dict(do_sample=True), dict(temperature=0.5), dict(seed=3), dict(do_sample=True, seed=3, temperature=0.0),
               dict(do_sample=True, seed=3, force_tokens=[[1, 2]]), dict(do_sample=True, seed=[1, 2])):
        with pytest.raises(ValueError):
            stub.generate(input_ids=ids, max_new_tokens=2, **kw)
        if "force_tokens" not in kw:
            with pytest.raises(ValueError):
                stub.explain_generated(input_ids=ids, max_new_tokens=2, **kw)
