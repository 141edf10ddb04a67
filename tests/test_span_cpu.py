"""CPU: answer-span attribution, explain(positions=...) -- what can be checked without a device.
  (1) engine.position_request: every refusal raises ValueError, a good request comes back normalised in slot order;
  (2) the default target: input_ids[b, p + 1] for p < S - 1, and only the slots at p = S - 1 are left to the arg-max;
  (3) the fixtures tests/golden/span_*.npz (the REAL lxt.efficient in fp64, make_golden_span.py) are self-consistent: case a's R_tok is the
      sum of case d's single-position rows to 1e-10 -- linearity of the modified backward in its seed, on the reference itself;
  (4) the three explain() signatures carry the keywords, and the C ABI declares lrp_span_seed."""
import inspect

import numpy as np
import pytest
import torch

import lxt_amd.engine as E
from tests.util import load, nmax

B, S, V = 2, 8, 50
IDS = torch.arange(B * S).reshape(B, S) % V
CPU = torch.device("cpu")


def req(positions, position_weights=None, objective="logit", per_position=False, **kw):
    kw.setdefault("input_ids", IDS)
    return E.position_request(positions, position_weights, objective, per_position, B, S, V, CPU, **kw)


@pytest.mark.parametrize("name,args,kw", [
    ("duplicate", ([[1, 1], [2, 3]],), {}),
    ("above range", ([[1, S], [2, 3]],), {}),
    ("negative", ([[-1, 2], [2, 3]],), {}),
    ("on a pad column", ([[4, 7], [1, 7]],), dict(lengths=[8, 6])),
    ("one-dimensional", ([1, 2],), {}),
    ("wrong batch", ([[1, 2]],), {}),
    ("T = 0", ([[], []],), {}),
    ("float positions", ([[1.0, 2.0], [2.0, 3.0]],), {}),
    ("ragged", ([[1, 2], [3]],), {}),
    ("weights shape", ([[1, 2], [2, 3]], [[1.0], [1.0]]), {}),
    ("weights not finite", ([[1, 2], [2, 3]], [[1.0, float("nan")], [1.0, 1.0]]), {}),
    ("target shape", ([[1, 2], [2, 3]],), dict(target=[3, 4])),
    ("target above the vocabulary", ([[1, 2], [2, 3]],), dict(target=[[3, V], [1, 2]])),
    ("target negative", ([[1, 2], [2, 3]],), dict(target=[[3, -1], [1, 2]])),
    ("no target with inputs_embeds", ([[1, 2], [2, 3]],), dict(input_ids=None)),
    ("unknown objective", ([[1, 2], [2, 3]], None, "prob"), {}),
    ("with seed", ([[1, 2], [2, 3]],), dict(seed=torch.zeros(B, V))),
    ("with graph", ([[1, 2], [2, 3]],), dict(graph=True)),
    ("explicit placement", ([[1, 2], [2, 3]],), dict(mode="explicit")),
    ("per_position with a read-out", ([[1, 2], [2, 3]], None, "logit", True), dict(readouts=True)),
    ("weights without positions", (None, [[1.0, 1.0], [1.0, 1.0]]), {}),
    ("per_position without positions", (None, None, "logit", True), {}),
    ("objective without positions", (None, None, "logprob"), {}),
])
def test_position_request_refuses(name, args, kw):
    with pytest.raises(ValueError):
        req(*args, **kw)


def test_position_request_normalises():
    assert req(None) is None
    r = req([[7, 0, 3], [2, 6, 7]], [[1.0, 0.0, -2.0], [0.5, 0.5, 0.5]], "logprob", lengths=[8, 6])
    assert r.T == 3 and r.objective == "logprob" and not r.per_position and r.w_each is None
    assert r.rows.dtype == torch.int64 and r.rows.tolist() == [7, 0, 3, S + 2, S + 6, S + 7]          # slot order, not sorted
    assert r.idx.dtype == torch.int32 and r.w.dtype == torch.float32 and r.w.tolist() == [1.0, 0.0, -2.0, 0.5, 0.5, 0.5]
    # a tensor request with explicit targets: nothing is left to the arg-max
    t = req(torch.tensor([[7], [0]]), target=torch.tensor([[4], [49]]))
    assert t.auto is None and t.idx.tolist() == [4, 49] and t.w.tolist() == [1.0, 1.0]
    p = req([[1, 5], [2, 3]], [[2.0, 3.0], [4.0, 5.0]], per_position=True)
    assert p.per_position and p.w_each.shape == (2, 4)
    assert p.w_each.tolist() == [[2.0, 0.0, 4.0, 0.0], [0.0, 3.0, 0.0, 5.0]]                        # pass t keeps slot t of every prompt
    assert torch.equal(p.w_each.sum(0), p.w)


def test_default_target_is_the_next_token():
    r = req([[7, 0, 3], [2, 6, 7]])
    nxt = lambda b, p: int(IDS[b, p + 1])          # noqa: E731
    assert r.idx.tolist()[1:5] == [nxt(0, 0), nxt(0, 3), nxt(1, 2), nxt(1, 6)]
    assert r.auto.tolist() == [0, 5]               # the two slots at column S - 1: the only ones the arg-max fills
    assert req([[1, 2], [3, 4]]).auto is None


@pytest.mark.parametrize("model", ["llama", "qwen3", "qwen3_moe"])
def test_fixtures_are_linear_in_the_seed(model):
    fx = load(f"span_{model}.npz")
    a, d = fx["a/R_tok"], fx["d/R_tok"]
    T = fx["a/positions"].shape[1]
    assert d.shape == (T, 1, int(fx["S"])) and fx["d/positions"][:, 0, 0].tolist() == fx["a/positions"][0].tolist()
    e_tok, e_lay = nmax(d.sum(0), a), nmax(fx["d/layer_R"].sum(0), fx["a/layer_R"])
    print(f"[{model}] reference fp64: sum of single-position R_tok vs joint {e_tok:.1e}, layer_R {e_lay:.1e}")
    assert e_tok <= 1e-10 and e_lay <= 1e-10
    # teacher forcing in the fixtures themselves, exact zeros above the highest explained row and at pads
    ids, pos, tgt = fx["c/ids"], fx["c/positions"], fx["c/target"]
    assert np.array_equal(tgt, np.take_along_axis(ids, pos + 1, 1))
    for b, n in enumerate(fx["c/lengths"].tolist()):
        assert not fx["c/R_tok"][b, : ids.shape[1] - n].any() and not fx["c/R_tok"][b, pos[b][fx["c/weights"][b] != 0].max() + 1:].any()
    assert np.array_equal(fx["a/logit"], fx["b/logit"]) and np.array_equal(fx["a/target"], fx["b/target"])


def test_signatures_and_abi():
    from lxt_amd import _lib
    from lxt_amd.engine_qwen import QwenLRP
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    for cls in (E.LlamaLRP, QwenLRP, Qwen3MoeLRP):
        par = inspect.signature(cls.explain).parameters
        assert [par[k].default for k in ("positions", "position_weights", "objective", "per_position")] == [None, None, "logit", False]
    ret, types = _lib.DECLS["lrp_span_seed"]
    assert ret == "int" and len(types) == 15 and hasattr(_lib.lib, "lrp_span_seed")
    # host-side argument checks of the entry (no device needed: they return before any launch)
    f = _lib.lib.lrp_span_seed
    assert f(None, 8, None, None, None, 1, 8, 0, None, 0, 0, None, None, None, None) == -1
    assert f(16, 8, 16, None, None, 0, 8, 0, None, 0, 0, 16, 16, None, None) == 0                 # R = 0: LRP_OK
    assert f(16, 8, 16, None, None, -1, 8, 0, None, 0, 0, 16, 16, None, None) == -1
    assert f(16, 8, 16, None, None, 0, 8, 2, None, 0, 0, 16, 16, None, None) == -1                # unknown objective
    assert f(16, 8, 16, None, None, 0, 8, 1, None, 8, 0, 16, 16, None, None) == -1                # logprob without a seed buffer
    assert f(16, 8, 16, None, None, 0, 8, 1, 16, 8, 7, 16, 16, None, None) == -1                  # unknown seed dtype
    assert f(16, 8, 16, None, None, 0, 8, 0, None, 0, 0, 16, 16, 16, None) == -1                  # rs without rstd
    assert f(16, 7, 16, None, None, 0, 8, 0, None, 0, 0, 16, 16, None, None) == -3                # pitch below V
    assert f(16, 8, 16, None, None, 0, 8, 1, 16, 7, 1, 16, 16, None, None) == -3
    assert f(18, 8, 16, None, None, 0, 8, 0, None, 0, 0, 16, 16, None, None) == -2                # logits off 4 bytes
