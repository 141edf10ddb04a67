"""CPU: the per-weight relevance read-out (include/lrp_hip_wgrad.h, csrc/wgrad.hip, explain(weights=...)) -- the entry and its predicate are
declared, exported and refuse bad calls before any launch; weight_request raises before any device work; the drivers that do not serve the
keyword refuse it; the committed fixtures equal an fp64 restatement of W (*) sum_t G^T x by plain autograd; the row map inverts
interleave_gate_up.  Numerics on the device: tests/test_wgrad_gpu.py."""
import ctypes
import inspect
import re

import numpy as np
import pytest
import torch

from oracle import llama as ol
from tests.util import load

I64, VP, IP, FP = "int64_t", "void*", "int*", "float*"
SIGS = {
    "lrp_wgrad_rel_ok": ["int", "int", "int", I64, I64, I64, I64, "int"],
    "lrp_wgrad_rel": [VP, VP, VP, FP, FP, IP, "int", "int", "int", I64, I64, I64, I64, "int", "int", VP],
}
NAMES = ("qkv", "o", "gate_up", "down")


def test_header_is_included_and_symbols_are_declared_and_exported():
    import lxt_amd._lib as L
    main = open(L.HEADER_PATH).read()
    assert '#include "lrp_hip_wgrad.h"' in main
    raw = ctypes.CDLL(L.LIB_PATH)
    for name, args in SIGS.items():
        assert L.DECLS[name] == ("int", args), name
        assert hasattr(raw, name), name
    own = re.sub(r"/\*.*?\*/", "", main, flags=re.S)          # lrp_hip.h's own prototype count and the ABI version do not move
    assert len(re.findall(r"\b(?:int64_t|int|const char\*)\s+lrp_\w+\s*\([^)]*\)\s*;", own)) == 89 and L.lib.lrp_version() == 8


A = 1 << 12          # an aligned fake device address: every call below is rejected before a launch
OK = dict(G=A, X=A, W=A, out=A, rs=A, rmap=A, M=5, N=64, K=128, ldg=64, ldx=128, ldw=128, ldo=128, accumulate=0, dtype=None, stream=None)


def test_argument_validation_without_gpu():
    import lxt_amd._lib as L
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    ok = dict(OK, dtype=L.BF16)
    call = lambda **kw: L.lib.lrp_wgrad_rel(*{**ok, **kw}.values())      # noqa: E731
    pred = lambda **kw: L.lib.lrp_wgrad_rel_ok(*[{**ok, **kw}[k] for k in ("M", "N", "K", "ldg", "ldx", "ldw", "ldo", "dtype")])      # noqa: E731
    assert pred() == 1 and pred(M=1) == 1 and pred(dtype=L.F32, N=3, K=5, ldg=3, ldx=5, ldw=5, ldo=5) == 1
    for kw in (dict(G=None), dict(X=None), dict(W=None), dict(out=None), dict(dtype=7)):
        assert call(**kw) == EINVAL, kw
    assert pred(dtype=7) == EINVAL
    shape = (dict(M=0), dict(N=0), dict(K=0), dict(N=60, ldg=64), dict(K=124), dict(ldg=56), dict(ldx=120), dict(ldw=120), dict(ldo=120),
             dict(N=128 * 65536, ldg=128 * 65536))
    for kw in shape:
        assert call(**kw) == ESHAPE and pred(**kw) == ESHAPE, kw
    for kw in (dict(ldg=68), dict(ldx=132), dict(ldw=132), dict(ldo=130)):
        assert call(**kw) == EALIGN and pred(**kw) == EALIGN, kw
    for kw in (dict(G=A + 8), dict(X=A + 2), dict(W=A + 8), dict(out=A + 4), dict(rs=A + 2), dict(rmap=A + 1)):
        assert call(**kw) == EALIGN, kw
    # the shape is judged before the pointers' alignment; fp32 takes any size and any pitch >= the width, bases on the 4-byte grid
    assert call(N=60, G=A + 8) == ESHAPE
    f32 = dict(dtype=L.F32, N=3, K=5, ldg=3, ldx=7, ldw=5, ldo=9)
    assert pred(**f32) == 1 and call(**f32, G=A + 2) == EALIGN and call(**dict(f32, ldx=4)) == ESHAPE
    # what is fine passes every check (and then fails at the launch or not at all: there may be no device here)
    for kw in (dict(rs=None, rmap=None), dict(ldo=132), dict(ldg=72), f32):
        assert call(**kw) not in (EINVAL, EALIGN, ESHAPE), kw


def test_wrapper_refuses_cpu_tensors_and_bad_operands():
    from lxt_amd import ops
    G, X, W = torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(4, 128, dtype=torch.bfloat16), torch.zeros(64, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.wgrad_rel(G, X, W)
    with pytest.raises(ValueError):
        ops.wgrad_rel(G, X[:3], W)
    with pytest.raises(ValueError):
        ops.wgrad_rel(G, X, W.T)
    assert ops.wgrad_rel_ok(4, 64, 128, 64, 128, 128, 128, torch.bfloat16) and not ops.wgrad_rel_ok(4, 64, 128, 64, 128, 128, 128, torch.float16)


CFG = dict(hidden=128, inter=256, n_layers=3, n_heads=2, n_kv=1, head_dim=64, vocab=512)


def test_weight_request():
    from lxt_amd.engine import weight_request, weight_shapes, WEIGHTS
    req = lambda w, l=None, o=None, dtype=torch.bfloat16, mode="efficient", graph=False, cfg=CFG: weight_request(w, l, o, cfg, 3, dtype, mode, graph)      # noqa: E731
    assert WEIGHTS == NAMES and req(None) == ((), ())
    assert req("down") == (("down",), (0, 1, 2)) and req(["down", "qkv", "down"], [1]) == (("qkv", "down"), (1,))
    assert req(NAMES, (0, 2)) == (NAMES, (0, 2)) and req((), [0]) == ((), ()) and req("o", []) == ((), ())
    assert weight_shapes(CFG) == dict(qkv=(256, 128), o=(128, 128), gate_up=(512, 128), down=(128, 256))
    for bad in ("up", ["o", "gate"], 3, [None]):
        with pytest.raises(ValueError):
            req(bad)
    for bad in ([3], [-1], [1, 0], [1, 1], 2, ["a"], [0.5]):
        with pytest.raises(ValueError):
            req("o", bad)
    with pytest.raises(ValueError, match="efficient"):
        req("o", mode="explicit")
    with pytest.raises(ValueError, match="graph"):
        req("o", graph=True)
    with pytest.raises(ValueError):
        req(None, [0])
    with pytest.raises(ValueError):
        req(None, None, {})
    with pytest.raises(ValueError, match="multiples of 8"):
        req("down", cfg=dict(CFG, inter=100))
    assert req("down", dtype=torch.float32, cfg=dict(CFG, inter=100)) == (("down",), (0, 1, 2))
    good = dict(o=torch.zeros(2, 128, 128), down=torch.zeros(2, 128, 256))
    assert req(["o", "down"], [0, 2], good) == (("o", "down"), (0, 2))
    for bad in (dict(o=good["o"]), dict(good, qkv=torch.zeros(2, 256, 128)), dict(good, o=torch.zeros(3, 128, 128)),
                dict(good, o=good["o"].double()), dict(good, down=torch.zeros(2, 256, 128).transpose(1, 2)), [good["o"], good["down"]]):
        with pytest.raises(ValueError, match="weights_out"):
            req(["o", "down"], [0, 2], bad)


def test_drivers_that_do_not_serve_the_keyword():
    from lxt_amd.engine import LlamaLRP
    from lxt_amd.engine_bert import BertLRP
    from lxt_amd.engine_gemma3 import Gemma3LRP
    from lxt_amd.engine_gemma3_mm import Gemma3MMLRP
    from lxt_amd.engine_qwen import QwenLRP
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    for cls in (LlamaLRP, QwenLRP):
        assert {"weights", "weight_layers", "weights_out"} <= set(inspect.signature(cls.explain).parameters)
    for cls in (BertLRP, Gemma3LRP, Gemma3MMLRP):
        assert "weights" not in inspect.signature(cls.explain).parameters
    stub = Qwen3MoeLRP.__new__(Qwen3MoeLRP)          # the refusal is the first thing explain does: nothing of the object is needed
    with pytest.raises(ValueError, match="routed experts"):
        stub.explain(torch.zeros(1, 4, dtype=torch.long), weights="o")


def test_row_map_inverts_interleave_gate_up():
    from lxt_amd import ops
    I, H = 96, 8
    wg, wu = torch.arange(I * H, dtype=torch.float32).view(I, H), -torch.arange(I * H, dtype=torch.float32).view(I, H) - 1
    stored = ops.interleave_gate_up(wg, wu)
    m = ops.gate_up_row_map(I, "cpu")
    assert m.dtype == torch.int32 and sorted(m.tolist()) == list(range(2 * I)) and ops.gate_up_row_map(I, "cpu") is m
    hf = torch.empty_like(stored).index_copy_(0, m.long(), stored)          # stored row s lands in row m[s]: what the kernel does
    assert torch.equal(hf, torch.cat([wg, wu]))
    with pytest.raises(ValueError):
        ops.gate_up_row_map(48, "cpu")


def _autograd_weight_relevance(cfg, W, ids):
    """W (*) sum_t G^T x of every decoder Linear by plain autograd in fp64: the Llama forward restated with torch ops, each Linear an explicit
    x @ W.T on a leaf; the reference's efficient rules as gradient surgery -- the norms' 1 / rms and the activation's ratio silu(g) / (g + 1e-10)
    held constant (identity rule), the gradient halved at the gated product and at v, quartered at q and k (uniform rule, ref
    lxt/efficient/patches.py) -- arg-max logit of the last position seeded with 1"""
    dd = lambda t: t.double()                       # noqa: E731
    H, nq, nk, d = cfg["hidden"], cfg["n_heads"], cfg["n_kv"], cfg["head_dim"]
    S = ids.numel()
    half = lambda x: x * 0.5 + (x * 0.5).detach()            # noqa: E731  (value x, gradient 1/2)
    quarter = lambda x: x * 0.25 + (x * 0.75).detach()       # noqa: E731
    norm = lambda x, w: x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + cfg["rms_eps"]).detach() * dd(w)      # noqa: E731
    inv = 1.0 / (cfg["rope_theta"] ** (torch.arange(0, d, 2, dtype=torch.float32) / d))          # (HF forms the rotary tables in fp32 whatever the model's dtype)
    fr = torch.arange(S, dtype=torch.float32)[:, None] * inv[None]
    cos, sin = torch.cat((fr, fr), -1).cos().double()[:, None], torch.cat((fr, fr), -1).sin().double()[:, None]
    rope = lambda x: x * cos + torch.cat((-x[..., d // 2:], x[..., : d // 2]), -1) * sin      # noqa: E731
    leaves = []
    h = dd(W["embed"])[ids]
    for L in W["layers"]:
        P = {k: dd(L[k]).clone().requires_grad_() for k in ("wq", "wk", "wv", "wo", "wg", "wu", "wd")}
        leaves.append(P)
        x = norm(h, L["ln1"])
        q, k, v = (x @ P["wq"].T).view(S, nq, d), (x @ P["wk"].T).view(S, nk, d), (x @ P["wv"].T).view(S, nk, d)
        q, k = rope(q), rope(k)
        k, v = k.repeat_interleave(nq // nk, 1), v.repeat_interleave(nq // nk, 1)
        sc = torch.einsum("ihd,jhd->hij", quarter(q), quarter(k)) * d ** -0.5
        sc = sc.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
        pr = torch.softmax(sc, -1, dtype=torch.float32).double()          # (HF's eager attention takes the softmax in fp32 whatever the dtype)
        o = torch.einsum("hij,jhd->ihd", pr, half(v)).reshape(S, nq * d)
        h = h + o @ P["wo"].T
        x = norm(h, L["ln2"])
        g, u = x @ P["wg"].T, x @ P["wu"].T
        act = g * (torch.nn.functional.silu(g) / (g + 1e-10)).detach()          # identity rule on the activation: silu(g) = g * const
        h = h + (half(act) * half(u)) @ P["wd"].T
    logits = norm(h[-1], W["norm"]) @ dd(W["lm_head"]).T
    idx = int(logits.argmax())
    logits[idx].backward()
    rel = lambda P, k: (P[k] * P[k].grad).detach()            # noqa: E731
    return idx, [dict(qkv=torch.cat([rel(P, "wq"), rel(P, "wk"), rel(P, "wv")]), o=rel(P, "wo"), gate_up=torch.cat([rel(P, "wg"), rel(P, "wu")]),
                      down=rel(P, "wd")) for P in leaves]


def test_fixture_equals_an_fp64_autograd_restatement():
    fx = load("weight_relevance_llama_prompts.npz")
    cfg = {k: (float(v) if k in ("rope_theta", "rms_eps") else int(v)) for k, v in zip(fx["cfg_keys"].tolist(), fx["cfg_vals"].tolist())}
    W = ol.random_weights(cfg, seed=int(fx["wseed"]))
    ids = torch.from_numpy(fx["ids"])
    runs = [_autograd_weight_relevance(cfg, W, row) for row in ids]
    assert [r[0] for r in runs] == fx["idx"].tolist()
    worst = 0.0
    for l in range(cfg["n_layers"]):
        lay = load(f"weight_relevance_llama_l{l}.npz")
        for n in NAMES:
            ref = runs[0][1][l][n] + runs[1][1][l][n]
            got = torch.from_numpy(lay[n]).double()
            assert got.shape == ref.shape and lay[n].dtype == np.float32
            worst = max(worst, float((got - ref).abs().max() / ref.abs().max()))
    for b in range(2):
        top = runs[b][1][-1]
        for key, ref in (("qkv_top", top["qkv"]), ("down_top", top["down"])):
            worst = max(worst, float((torch.from_numpy(fx[key][b]).double() - ref).abs().max() / ref.abs().max()))
        for l in range(cfg["n_layers"]):
            ref = runs[b][1][l]["o"]
            worst = max(worst, float((torch.from_numpy(fx["o"][b, l]).double() - ref).abs().max() / ref.abs().max()))
    print(f"fixture (fp32 storage of the reference's fp64 values) vs the autograd restatement: normalised max {worst:.2e}")
    # the fp32 storage rounds by 2^-24; HF's eager attention takes its softmax in fp32 on BOTH sides, on scores that differ in their last fp64
    # bit, so the probabilities of the two runs carry independent fp32 roundings (exp, sum, divide: a few 2^-24 each) in each of the three
    # layers: 16 x 2^-24.  A wrong rule or factor anywhere shows at 1e-2 and above
    assert worst <= 2.0 ** -20
