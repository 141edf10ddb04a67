"""CPU: lrp_token_hist_init / lrp_logit_penalty (include/lrp_hip_penalty.h) are declared in their own header, exported, and validate their
arguments before any launch (host integers as pointers); the ops wrappers refuse host tensors and wrong dtypes; engine.penalty_request
refuses what it must without a device; the drivers carry the four keywords; the numpy restatement (tests/penalty_oracle.py) equals HF's
RepetitionPenaltyLogitsProcessor in fp64.  HF has no presence / frequency processor: those two are checked against the stated formula
(x - frequency_penalty * count - presence_penalty on generated columns, the OpenAI / vLLM definition) only."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests import penalty_oracle as po

EINVAL, EALIGN, ESHAPE = -1, -2, -3
NAMES = ("lrp_token_hist_init", "lrp_logit_penalty")
PENALTY_KW = (("repetition_penalty", 1.0), ("presence_penalty", 0.0), ("frequency_penalty", 0.0), ("logit_bias", None))
INF, NAN = float("inf"), float("nan")


def test_symbols_declared_in_their_own_header_and_exported():
    import lxt_amd._lib as L
    decls = L.parse_header()
    raw = ctypes.CDLL(L.LIB_PATH)
    inc = os.path.dirname(L.HEADER_PATH)
    with open(L.HEADER_PATH) as f:
        top = f.read()
    with open(os.path.join(inc, "lrp_hip_penalty.h")) as f:
        mine = f.read()
    assert '#include "lrp_hip_penalty.h"' in top
    for name in NAMES:
        assert name in decls, f"{name} is not declared in a header lrp_hip.h includes"
        assert hasattr(raw, name), f"{name} declared but not exported"
        assert decls[name][0] == "int" and name in mine and name + "(" not in top
    assert len(decls[NAMES[0]][1]) == 9 and len(decls[NAMES[1]][1]) == 14
    assert decls[NAMES[0]][1][0] == "int64_t*" and decls[NAMES[1]][1][9:12] == ["float"] * 3
    assert L.lib.lrp_version() == 8


def test_hist_init_argument_ladder_without_gpu():
    import lxt_amd._lib as L
    P = 4096

    def call(ids=P, ld_ids=10, lo=P, B=2, S=10, V=100, hist=P, ld_hist=100):
        return L.lib.lrp_token_hist_init(ids, ld_ids, lo, B, S, V, hist, ld_hist, None)

    assert call(ids=None) == EINVAL and call(hist=None) == EINVAL
    for kw in (dict(B=-1), dict(S=-1), dict(V=0), dict(V=-5)):
        assert call(**kw) == EINVAL, kw
    assert call(ld_ids=9) == ESHAPE and call(ld_hist=99) == ESHAPE
    assert call(V=0, ld_hist=-1) == EINVAL and call(ld_ids=9, hist=P + 2) == ESHAPE
    assert call(ids=P + 4) == EALIGN and call(lo=P + 2) == EALIGN and call(hist=P + 1) == EALIGN
    assert call(B=0) == 0 and call(B=0, lo=None) == 0 and call(B=0, hist=P + 4, ld_hist=101, ids=P + 8, ld_ids=11) == 0 and call(B=0, S=0) == 0


def test_logit_penalty_argument_ladder_without_gpu():
    """EINVAL, then ESHAPE, then EALIGN, all before a launch: the pointers are host integers that no kernel may ever see, and every accepted
    call has B = 0"""
    import lxt_amd._lib as L
    P, Q, H = 4096, 8192, 16384

    def call(logits=P, ld=100, out=Q, ld_out=100, B=2, V=100, hist=H, ld_hist=100, last=P, rp=1.1, pp=0.5, fp=0.25, bias=P):
        return L.lib.lrp_logit_penalty(logits, ld, out, ld_out, B, V, hist, ld_hist, last, rp, pp, fp, bias, None)

    assert call(logits=None) == EINVAL and call(out=None) == EINVAL and call(hist=None) == EINVAL and call(out=P) == EINVAL
    for kw in (dict(B=-1), dict(V=0), dict(rp=0.0), dict(rp=-1.0), dict(rp=INF), dict(rp=NAN), dict(pp=INF), dict(pp=-INF), dict(pp=NAN),
               dict(fp=INF), dict(fp=-INF), dict(fp=NAN)):
        assert call(**kw) == EINVAL, kw
    # (a bad value wins over a bad shape, a bad shape over a bad alignment)
    assert call(rp=0.0, ld=99) == EINVAL
    for kw in (dict(ld=99), dict(ld_out=99), dict(ld_hist=99), dict(ld=99, out=Q + 2)):
        assert call(**kw) == ESHAPE, kw
    for name, base in (("logits", P), ("out", Q), ("hist", H), ("last", P), ("bias", P)):
        assert call(**{name: base + 2}) == EALIGN, name
    # accepted: nothing to do, nothing launched -- off the 16-byte grid, pitches, the optional pointers absent, negative penalties
    assert call(B=0) == 0 and call(B=0, logits=P + 4, out=Q + 8, hist=H + 12, ld=101, ld_out=102, ld_hist=103) == 0
    assert call(B=0, last=None, bias=None) == 0 and call(B=0, rp=1.0, pp=0.0, fp=0.0) == 0 and call(B=0, rp=0.5, pp=-2.0, fp=-0.1) == 0


def test_ops_wrappers_refuse_host_tensors_and_wrong_dtypes():
    import lxt_amd.ops as ops
    ids, hist, logits = torch.zeros(2, 5, dtype=torch.int64), torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, 8)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.token_hist_init(ids, None, 8)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.logit_penalty(logits, hist)
    with pytest.raises(TypeError):
        ops.token_hist_init(ids.int(), None, 8)
    with pytest.raises(ValueError):
        ops.token_hist_init(ids[0], None, 8)
    with pytest.raises(TypeError):
        ops.logit_penalty(logits.double(), hist)
    with pytest.raises(TypeError):
        ops.logit_penalty(logits, hist.long())
    with pytest.raises(TypeError):
        ops.logit_penalty(logits, hist.float())
    with pytest.raises(ValueError):
        ops.logit_penalty(logits[0], hist)
    with pytest.raises(ValueError):
        ops.logit_penalty(logits[:, ::2], hist)


def test_penalty_request():
    from lxt_amd.engine import penalty_request as pr
    V = 16
    assert pr(1.0, 0.0, 0.0, None, V, None) is None and pr(1, 0, 0, None, V, None) is None
    assert pr(1.0, 0.0, 0.0, None, V, [[1, 2]]) is None and pr(1.0, 0.0, 0.0, {}, V, None) is None
    ok = dict(repetition_penalty=1.1, presence_penalty=0.5, frequency_penalty=0.25, logit_bias={3: -INF, 5: 2.0}, vocab=V, force_tokens=None)
    bad = (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=INF), dict(repetition_penalty=NAN),
           dict(repetition_penalty="1.1"), dict(repetition_penalty=True), dict(presence_penalty=INF), dict(presence_penalty=NAN),
           dict(presence_penalty=None), dict(frequency_penalty=-INF), dict(frequency_penalty=NAN), dict(logit_bias={-1: 1.0}),
           dict(logit_bias={V: 1.0}), dict(logit_bias={1.0: 1.0}), dict(logit_bias={True: 1.0}), dict(logit_bias={2: NAN}),
           dict(logit_bias={2: INF}), dict(logit_bias={2: "x"}), dict(logit_bias={j: -INF for j in range(V)}),
           dict(logit_bias=torch.full((V,), -INF)), dict(logit_bias=torch.zeros(V + 1)), dict(logit_bias=torch.zeros(1, V)),
           dict(logit_bias=torch.zeros(V, dtype=torch.float64)), dict(logit_bias=torch.full((V,), NAN)), dict(logit_bias=torch.full((V,), INF)),
           dict(logit_bias=[0.0] * V), dict(force_tokens=[[1, 2]]))
    for kw in bad:
        with pytest.raises(ValueError):
            pr(**dict(ok, **kw))
    # every single non-neutral setting is refused next to force_tokens
    for kw in (dict(repetition_penalty=1.3), dict(presence_penalty=1.0), dict(frequency_penalty=0.5), dict(logit_bias={1: 1.0})):
        with pytest.raises(ValueError):
            pr(**dict(dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None, vocab=V,
                           force_tokens=[[1, 2]]), **kw))
    s = pr(**ok)
    assert (s.repetition_penalty, s.presence_penalty, s.frequency_penalty) == (1.1, 0.5, 0.25)
    assert s.bias.dtype == torch.float32 and s.bias.shape == (V,) and not s.bias.is_cuda
    assert s.bias[3] == -INF and s.bias[5] == 2.0 and float(s.bias.nan_to_num(neginf=0).abs().sum()) == 2.0
    t = torch.arange(V, dtype=torch.float32)
    assert torch.equal(pr(1.0, 0.0, 0.0, t, V, None).bias, t) and pr(1.0, 0.0, 0.0, t, V, None).repetition_penalty == 1.0
    assert pr(0.5, -1.0, -0.5, None, V, None).bias is None and pr(1.0, 0.0, 0.0, {2: -INF}, V, None).bias[2] == -INF


def test_drivers_carry_the_penalty_keywords():
    from lxt_amd.engine import LlamaLRP, explain_answer, generate_cached, greedy_decode
    from lxt_amd.engine_gemma3 import Gemma3LRP
    from lxt_amd.engine_qwen import QwenLRP
    for cls in (LlamaLRP, QwenLRP, Gemma3LRP):
        for name in ("generate", "explain_generated"):
            par = inspect.signature(getattr(cls, name)).parameters
            names = list(par)
            i = names.index("seed")
            assert tuple(names[i + 1: i + 5]) == tuple(k for k, _ in PENALTY_KW), (cls.__name__, name)
            for k, d in PENALTY_KW:
                assert par[k].default == d and type(par[k].default) is type(d), (cls.__name__, name, k)
        assert list(inspect.signature(cls.generate).parameters)[-1] == "logit_bias"
        names = list(inspect.signature(cls.explain_generated).parameters)
        assert names[-2:] == ["logit_bias", "readout_kw"]
        for name in ("generate", "explain_generated"):
            assert list(inspect.signature(getattr(cls, name)).parameters) == list(inspect.signature(getattr(LlamaLRP, name)).parameters)
    for fn in (generate_cached, explain_answer):
        par = inspect.signature(fn).parameters
        assert tuple(list(par)[-4:]) == tuple(k for k, _ in PENALTY_KW)
        assert all(par[k].default == d for k, d in PENALTY_KW)
    par = inspect.signature(greedy_decode).parameters
    assert "penalty" in par and par["penalty"].default is None


def test_generate_refuses_penalty_requests_without_a_device():
    """a stub without weights: the request's ValueError comes first"""
    from lxt_amd.engine import LlamaLRP
    from lxt_amd.engine_gemma3 import Gemma3LRP
    for cls in (LlamaLRP, Gemma3LRP):
        stub = cls.__new__(cls)
        stub.cfg, stub.dtype, stub.max_seq = dict(hidden=64, inter=128, vocab=32, head_dim=32, n_heads=2), torch.float32, 16
        ids = torch.zeros(1, 8, dtype=torch.long)
        for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=NAN), dict(presence_penalty=INF), dict(frequency_penalty=NAN),
                   dict(logit_bias={32: 1.0}), dict(logit_bias={0: NAN}), dict(logit_bias=torch.zeros(31)),
                   dict(logit_bias={j: -INF for j in range(32)}), dict(repetition_penalty=1.3, force_tokens=[[1, 2]])):
            with pytest.raises(ValueError):
                stub.generate(input_ids=ids, max_new_tokens=2, **kw)
            if "force_tokens" not in kw:
                with pytest.raises(ValueError):
                    stub.explain_generated(input_ids=ids, max_new_tokens=2, **kw)


def test_moe_driver_still_does_not_generate():
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    stub = Qwen3MoeLRP.__new__(Qwen3MoeLRP)
    with pytest.raises(NotImplementedError):
        stub.generate(torch.zeros(1, 4, dtype=torch.long), 2, repetition_penalty=1.3)
    with pytest.raises(NotImplementedError):
        stub.explain_generated(torch.zeros(1, 4, dtype=torch.long), 2, presence_penalty=1.0)


def hf_rows(rng, V):
    """fp64 rows with negative, zero, -0, -inf and repeated entries"""
    row = 3.0 * rng.standard_normal(V)
    row[rng.random(V) < 0.1] = 0.0
    row[rng.random(V) < 0.05] = -0.0
    row[rng.random(V) < 0.1] = -np.inf
    row[: V // 4] = np.round(row[: V // 4])
    return row


def test_oracle_repetition_branch_equals_hf_processor():
    """HF's RepetitionPenaltyLogitsProcessor over input_ids = prompt + generated tokens (a token may occur several times, in either part)
    against the fp64 evaluation of the oracle, bit for bit"""
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    rng, n = np.random.default_rng(5), 0
    for V in (33, 257, 5000):
        for rp in (1.3, 1.05, 0.8):
            rows = np.stack([hf_rows(rng, V) for _ in range(3)])
            prompt = rng.integers(0, V, (3, 12))
            prompt[:, 3] = prompt[:, 7]                       # a repeated prompt token
            gen = rng.integers(0, V, (3, 6))
            gen[:, 0], gen[:, 1], gen[:, 2] = prompt[:, 0], gen[:, 5], gen[:, 5]          # prompt and generated; generated three times
            for b in range(3):                                # make sure every kind of entry is penalised somewhere
                neg_inf = np.nonzero(np.isneginf(rows[b]))[0]
                zero = np.nonzero(rows[b] == 0)[0]
                prompt[b, 1], prompt[b, 2] = neg_inf[0], zero[0]
            hist = po.hist_init(prompt, None, V)
            for t in range(gen.shape[1]):
                po.bump(hist, gen[:, t])
            got = po.penalise(rows, hist, rp=rp, dtype=np.float64)
            ids = torch.from_numpy(np.concatenate([prompt, gen], 1))
            want = RepetitionPenaltyLogitsProcessor(rp)(ids, torch.from_numpy(rows.copy())).numpy()
            assert np.array_equal(got.view(np.int64), want.view(np.int64)), (V, rp)
            assert not np.array_equal(got, rows)
            n += 1
    assert n == 9


def test_oracle_presence_and_frequency_follow_the_stated_formula():
    """x - fp * count - pp on generated columns only (prompt-only columns are untouched by these two), then the bias; fp32 rounding is per
    operation, including a count beyond 2^24"""
    V = 8
    hist = np.zeros((1, V), np.int32)
    hist[0, 1] = po.SEEN
    hist[0, 2] = 3
    hist[0, 3] = po.SEEN + 1
    hist[0, 4] = 2 ** 24 + 1
    x = np.array([[1.0, 2.0, 3.0, -4.0, 5.0, -np.inf, 0.0, -0.0]])
    got = po.penalise(x, hist, pp=0.5, fp=0.25, dtype=np.float64)
    assert got[0].tolist() == [1.0, 2.0, 3.0 - 0.75 - 0.5, -4.0 - 0.25 - 0.5, 5.0 - 0.25 * (2 ** 24 + 1) - 0.5, -np.inf, 0.0, -0.0]
    g32 = po.penalise(x, hist, pp=0.5, fp=0.25, dtype=np.float32)
    assert g32.dtype == np.float32 and g32[0, 4] == np.float32(np.float32(5.0) - np.float32(0.25) * np.float32(2 ** 24)) - np.float32(0.5)
    both = po.penalise(x, hist, rp=2.0, pp=0.5, fp=0.25, bias=np.array([0, 0, 1, 0, 0, 0, -np.inf, 0.0]), dtype=np.float64)
    assert both[0].tolist() == [1.0, 1.0, 1.5 - 0.75 - 0.5 + 1, -8.0 - 0.25 - 0.5, 2.5 - 0.25 * (2 ** 24 + 1) - 0.5, -np.inf, -np.inf, -0.0]
    # the table: pads are no history, ids outside [0, V) are skipped, an out-of-range last is ignored, the count saturates
    h = po.hist_init(np.array([[7, 1, 2, 99, -3], [5, 5, 6, 0, 1]]), np.array([1, 2]), V)
    assert h[0].tolist() == [0, po.SEEN, po.SEEN, 0, 0, 0, 0, 0] and h[1].tolist() == [po.SEEN, po.SEEN, 0, 0, 0, 0, po.SEEN, 0]
    po.bump(h, np.array([1, V]))
    po.bump(h, np.array([-1, 3]))
    assert h[0, 1] == po.SEEN + 1 and h[1].tolist() == [po.SEEN, po.SEEN, 0, 1, 0, 0, po.SEEN, 0]
    h[0, 0] = po.CMAX
    assert po.bump(h, np.array([0, 0]))[0, 0] == po.CMAX
