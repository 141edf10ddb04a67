"""CPU: the per-weight relevance of a Qwen3-MoE (include/lrp_hip_moe_wgrad.h, csrc/moe_wgrad.hip, Qwen3MoeLRP.explain(moe_weights=...)) -- the
three entries are declared, exported and refuse bad calls before any launch; the wrapper refuses CPU tensors; moe_weight_request raises
before any device work; the committed reference fixtures (make_golden_moe_weight_relevance.py) tie the new quantity to R_expert of
qwen3_moe_experts_*.npz and are consistent with their own totals.  Numerics on the device: tests/test_moe_wgrad_gpu.py."""
import ctypes
import inspect
import re

import numpy as np
import pytest
import torch

from tests.util import load

I64, VP, IP, FP = "int64_t", "void*", "int*", "float*"
TAIL = ["int", "int", "int", "int", "int", I64, I64, "int", "int", "int", VP]          # T k E N K ldg ldx mode accumulate dtype stream
SIGS = {
    "lrp_moe_wgrad_rel_ok": ["int", "int", "int", "int", "int", I64, I64, "int", "int", "int"],
    "lrp_moe_wgrad_rel": [VP, VP, VP, VP, IP, FP] + TAIL,
    "lrp_moe_wgrad_rel_q": [VP, VP, VP, VP, VP, IP, FP] + TAIL,
}
NAMES = ("qkv", "o", "router", "gate_up", "down")
GATE_UP, DOWN = 0, 1


def test_header_is_included_and_symbols_are_declared_and_exported():
    import lxt_amd._lib as L
    main = open(L.HEADER_PATH).read()
    assert '#include "lrp_hip_moe_wgrad.h"' in main
    raw = ctypes.CDLL(L.LIB_PATH)
    for name, args in SIGS.items():
        assert L.DECLS[name] == ("int", args), name
        assert hasattr(raw, name), name
    own = re.sub(r"/\*.*?\*/", "", main, flags=re.S)          # lrp_hip.h's own prototype count and the ABI version do not move
    assert len(re.findall(r"\b(?:int64_t|int|const char\*)\s+lrp_\w+\s*\([^)]*\)\s*;", own)) == 89 and L.lib.lrp_version() == 8


A = 1 << 12          # an aligned fake device address: every call below is rejected before a launch
OK = dict(G=A, X=A, W=A, w=A, plan=A, out=A, T=5, k=2, E=4, N=64, K=128, ldg=64, ldx=128, mode=DOWN, accumulate=0, dtype=None, stream=None)
PRED = ("T", "k", "E", "N", "K", "ldg", "ldx", "mode", "dtype")


def test_argument_validation_without_gpu():
    import lxt_amd._lib as L
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    ok = dict(OK, dtype=L.BF16)

    def call(q=False, **kw):
        a = {**ok, **kw}
        if q:          # codes in W's place, scales behind them
            return L.lib.lrp_moe_wgrad_rel_q(a["G"], a["X"], a["W"], a.get("scales", A), *[a[k] for k in list(OK)[3:]])
        return L.lib.lrp_moe_wgrad_rel(*[a[k] for k in OK])

    def pred(q=0, **kw):
        a = {**ok, **kw}
        return L.lib.lrp_moe_wgrad_rel_ok(*[a[k] for k in PRED], q)

    assert pred() == 1 and pred(mode=GATE_UP) == 1 and pred(q=1) == 1 and pred(T=1, k=1, E=1) == 1
    assert pred(dtype=L.F32, N=3, K=5, ldg=4, ldx=8) == 1
    # NULL operands, an unknown mode or dtype
    for kw in (dict(G=None), dict(X=None), dict(W=None), dict(plan=None), dict(out=None), dict(w=None), dict(dtype=7), dict(mode=2), dict(mode=-1)):
        assert call(**kw) == EINVAL, kw
        assert call(q=True, **kw) == EINVAL, kw
    assert call(q=True, scales=None) == EINVAL
    assert call(mode=GATE_UP, w=None) not in (EINVAL, EALIGN, ESHAPE)          # the gate_up mode does not read w
    assert pred(dtype=7) == EINVAL and pred(mode=2) == EINVAL
    # sizes: bf16 N / K off the grid of 8, pitches below the width, E > 1024, sizes < 1, too many row tiles; _q: K off the grid of 128
    shape = (dict(T=0), dict(k=0), dict(E=0), dict(N=0), dict(K=0), dict(N=60), dict(K=124), dict(ldg=56), dict(ldx=120), dict(E=1025),
             dict(T=1 << 29, k=2), dict(N=128 * 65536, ldg=128 * 65536))
    for kw in shape:
        assert call(**kw) == ESHAPE and pred(**kw) == ESHAPE, kw
        assert call(q=True, **kw) == ESHAPE, kw
    assert pred(E=1024) == 1
    for K in (64, 192, 136):
        assert call(q=True, K=K, ldx=256) == ESHAPE and pred(q=1, K=K, ldx=256) == ESHAPE and pred(K=K, ldx=256) == 1, K
    assert pred(q=1, K=256, ldx=256) == 1
    # pitches off 16 bytes
    for kw in (dict(ldg=68), dict(ldx=132), dict(dtype=L.F32, ldg=66), dict(dtype=L.F32, ldx=130)):
        assert call(**kw) == EALIGN and pred(**kw) == EALIGN, kw
    # bases off 16 bytes (plan / scales: 4; w: its element size)
    for kw in (dict(G=A + 8), dict(X=A + 2), dict(W=A + 8), dict(out=A + 4), dict(plan=A + 2), dict(w=A + 1)):
        assert call(**kw) == EALIGN, kw
        assert call(q=True, **kw) == EALIGN, kw
    assert call(q=True, scales=A + 2) == EALIGN and call(dtype=L.F32, w=A + 2) == EALIGN
    # the shape is judged before the pointers' alignment
    assert call(N=60, G=A + 8) == ESHAPE
    # what is fine passes every check (and then fails at the launch or not at all: there may be no device here)
    for kw in (dict(), dict(mode=GATE_UP), dict(ldg=72, ldx=136), dict(dtype=L.F32, N=3, K=5, ldg=4, ldx=8), dict(w=A + 2)):
        assert call(**kw) not in (EINVAL, EALIGN, ESHAPE), kw
    assert call(q=True, scales=A + 4) not in (EINVAL, EALIGN, ESHAPE)


def test_wrapper_refuses_cpu_tensors_and_bad_operands():
    from lxt_amd import ops
    assert "moe_wgrad_rel" in dir(ops) and list(inspect.signature(ops.moe_wgrad_rel).parameters) == ["G", "X", "W", "plan", "mode", "w", "out",
                                                                                                     "accumulate"]
    plan = ops.MoePlan.__new__(ops.MoePlan)          # (a plan's constructor launches; the wrapper's own checks come first)
    plan.T, plan.k, plan.E, plan.buf = 4, 2, 3, torch.zeros(64, dtype=torch.int32)
    G, X, W = torch.zeros(8, 64, dtype=torch.bfloat16), torch.zeros(4, 128, dtype=torch.bfloat16), torch.zeros(3, 64, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.moe_wgrad_rel(G, X, W, plan, "gate_up")
    with pytest.raises(ValueError, match="mode"):
        ops.moe_wgrad_rel(G, X, W, plan, "up")
    with pytest.raises(TypeError):
        ops.moe_wgrad_rel(G, X, W, None, "gate_up")
    with pytest.raises(ValueError):
        ops.moe_wgrad_rel(G[:4], X, W, plan, "gate_up")          # G must hold the plan's rows
    with pytest.raises(ValueError):
        ops.moe_wgrad_rel(G, X, W[:2], plan, "gate_up")          # E of the plan
    with pytest.raises(ValueError):
        ops.moe_wgrad_rel(G, X, W[0], plan, "gate_up")


CFG = dict(hidden=128, moe_inter=128, n_experts=8, n_heads=4, n_kv=2, head_dim=32, moe_layers=(True, False, True))


def test_moe_weight_request():
    from lxt_amd.engine_qwen_moe import MOE_WEIGHTS, moe_weight_request, moe_weight_shapes
    req = lambda w, l=None, o=None, dtype=torch.bfloat16, mode="efficient", graph=False, cfg=CFG: moe_weight_request(w, l, o, cfg, dtype, mode, graph)      # noqa: E731
    assert MOE_WEIGHTS == NAMES and req(None) == ((), (), ())
    assert moe_weight_shapes(CFG) == dict(qkv=(256, 128), o=(128, 128), router=(8, 128), gate_up=(8, 256, 128), down=(8, 128, 128))
    assert req("down") == (("down",), (0, 1, 2), (0, 2)) and req(["down", "qkv", "down"], [1, 2]) == (("qkv", "down"), (1, 2), (2,))
    assert req(NAMES, (0, 2)) == (NAMES, (0, 2), (0, 2)) and req((), [0]) == ((), (), ()) and req("o", []) == ((), (), ())
    assert req(["qkv", "o"], [1]) == (("qkv", "o"), (1,), ())          # the dense layer has an attention half
    for bad in ("up", ["o", "gate"], 3, [None]):
        with pytest.raises(ValueError):
            req(bad)
    for bad in ([3], [-1], [1, 0], [1, 1], 2, ["a"], [0.5]):
        with pytest.raises(ValueError):
            req("o", bad)
    for name in ("router", "gate_up", "down"):
        with pytest.raises(ValueError, match="sparse"):
            req(["o", name], [1])
    with pytest.raises(ValueError, match="efficient"):
        req("o", mode="explicit")
    with pytest.raises(ValueError, match="graph"):
        req("o", graph=True)
    with pytest.raises(ValueError):
        req(None, [0])
    with pytest.raises(ValueError):
        req(None, None, {})
    with pytest.raises(ValueError, match="multiples of 8"):
        req("router", cfg=dict(CFG, n_experts=6))
    assert req("router", dtype=torch.float32, cfg=dict(CFG, n_experts=6)) == (("router",), (0, 1, 2), (0, 2))
    good = dict(o=torch.zeros(3, 128, 128), down=torch.zeros(2, 8, 128, 128))
    assert req(["o", "down"], None, good) == (("o", "down"), (0, 1, 2), (0, 2))
    for bad in (dict(o=good["o"]), dict(good, qkv=torch.zeros(3, 256, 128)), dict(good, down=torch.zeros(3, 8, 128, 128)),
                dict(good, o=good["o"].double()), dict(good, down=torch.zeros(2, 8, 128, 128).transpose(2, 3)), [good["o"], good["down"]]):
        with pytest.raises(ValueError, match="weights_out"):
            req(["o", "down"], None, bad)


def test_explain_signature_and_the_old_keyword():
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    assert {"moe_weights", "weight_layers", "weights_out", "weights"} <= set(inspect.signature(Qwen3MoeLRP.explain).parameters)
    stub = Qwen3MoeLRP.__new__(Qwen3MoeLRP)
    with pytest.raises(ValueError, match="routed experts"):
        stub.explain(torch.zeros(1, 4, dtype=torch.long), weights="o")


def _tiny():
    head = load("moe_weight_relevance_tiny.npz")
    gu = np.stack([np.concatenate([load(f"moe_weight_relevance_tiny_gate_up_l{l}_e{a}.npz")["gate_up"] for a in (0, 4)]) for l in head["moe"]])
    dn = np.stack([load(f"moe_weight_relevance_tiny_down_l{l}.npz")["down"] for l in head["moe"]])
    return head, gu, dn


@pytest.mark.parametrize("case", ["tiny", "fanout"])
def test_fixture_totals_equal_the_expert_relevance(case):
    """per expert, sum (gate_up_proj (*) grad)[e] = sum (down_proj (*) grad)[e] = sum_b R_expert[l, b, e] of the committed expert fixture (the
    identity rule on the activation and the uniform rules conserve relevance).  Bar 1e-9 of the largest value: the deviation the generator
    measured is 4.4e-11, the activation rule's 1e-10 stabiliser; an expert without rows is exactly 0"""
    head, fe = load(f"moe_weight_relevance_{case}.npz"), load(f"qwen3_moe_experts_{case}.npz")
    assert head["idx"].tolist() == fe["idx"].tolist() and np.array_equal(head["logit"], fe["logit"])
    moe = head["moe"].tolist()
    R = fe["R_expert"].sum(1)[moe]                                       # [L', E]
    counts = np.stack([np.bincount(fe["expert_index"][l].reshape(-1), minlength=R.shape[1]) for l in moe])
    assert np.array_equal(counts, head["counts"]) and head["gate_up_total"].dtype == np.float64
    for name in ("gate_up_total", "down_total"):
        dev = float(np.abs(head[name] - R).max() / np.abs(R).max())
        print(f"[{case}] {name} vs sum_b R_expert: {dev:.1e} of the largest value")
        assert dev <= 1e-9
        assert bool((head[name][counts == 0] == 0).all())
    if case == "fanout":
        assert bool((counts == 0).any()) and bool((head["chosen_rows"][:, :2] == [0, 1]).all())
        assert np.array_equal(np.take_along_axis(counts, head["chosen"], 1), head["chosen_rows"])
        assert bool((head["chosen_rows"][:, 2] == counts.max(1)).all())


def test_fixture_matrices_sum_to_the_totals():
    """the fp32 matrices against the fp64 totals: storage rounds every entry by at most 2^-24 of itself, so a sum moves by at most
    2^-24 sum |entries|; the bar is 2^-23 sum |entries| per expert"""
    head, gu, dn = _tiny()
    assert gu.shape == (2, 8, 256, 128) and dn.shape == (2, 8, 128, 128) and gu.dtype == np.float32 and dn.dtype == np.float32
    assert head["router"].shape == (2, 8, 128) and head["qkv"].shape == (3, 256, 128) and head["o"].shape == (3, 128, 128)
    for name, m in (("gate_up_total", gu), ("down_total", dn)):
        m = m.astype(np.float64)
        assert bool((np.abs(m.sum((2, 3)) - head[name]) <= 2.0 ** -23 * np.abs(m).sum((2, 3))).all()), name
    fo = load("moe_weight_relevance_fanout.npz")
    assert fo["gate_up_rowsum"].shape == (2, 128, 256) and fo["down_rowsum"].shape == (2, 128, 128)
    for j, l in enumerate(fo["moe"].tolist()):
        lay = load(f"moe_weight_relevance_fanout_l{l}.npz")
        for name, tot, rs in (("gate_up", "gate_up_total", "gate_up_rowsum"), ("down", "down_total", "down_rowsum")):
            m = lay[name].astype(np.float64)                             # [3, N, K]: the chosen experts
            e = fo["chosen"][j]
            assert bool((np.abs(m.sum((1, 2)) - fo[tot][j, e]) <= 2.0 ** -23 * np.abs(m).sum((1, 2))).all()), (name, l)
            # a row sum was formed in fp64 and rounded once; the stored entries carry a rounding each
            assert bool((np.abs(m.sum(2) - fo[rs][j, e]) <= 2.0 ** -23 * np.abs(m).sum(2) + 2.0 ** -24 * np.abs(fo[rs][j, e])).all()), (name, l)
            assert bool((m[0] == 0).all()) and bool((fo[rs][j, e[0]] == 0).all())          # the expert without rows
