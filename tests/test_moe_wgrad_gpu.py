"""GPU: per-weight relevance of a Qwen3-MoE (Qwen3MoeLRP.explain(moe_weights=...)).
  (1) lrp_moe_wgrad_rel against an fp64 torch restatement on the rounded inputs: bf16 / fp32, both modes, padded pitches, experts of
      0 / 1 / 63 / 64 / 65 / 130 rows and a skipped slot, accumulate, the zero-row rule; the MXFP4 entry bit-identical to the plain one on the
      dequantised tensor; bitwise repeatable; the refusals;
  (2) the fp32 engine against tests/golden/moe_weight_relevance_*.npz (the REAL lxt.efficient in fp64, make_golden_moe_weight_relevance.py),
      the conservation identity against R_expert of the same call, a left-padded batch, weights_out, weight_layers, nothing else moves,
      moe_weights=None launches nothing, the MXFP4 engine equals the engine on its dequantised experts;
  (3) the bf16 engine on the planted-routing model against the fp32 engine, kernel by kernel and with the fused attention half."""
import functools

import numpy as np
import pytest
import torch

from tests.golden import moe_engine_models as mm
from tests.golden.moe_models import build_qwen3_moe, inputs
from tests.util import load, nmax

pytestmark = pytest.mark.gpu

NAMES = ("qkv", "o", "router", "gate_up", "down")
BF16, F32 = torch.bfloat16, torch.float32
BAR = 1e-4          # the project's fp32 read-out bar (tests/test_qwen_moe_engine_gpu.py)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a HIP device")
    from lxt_amd import ops
    return ops


def _gnmax(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _cosine(a, b):
    return float(torch.nn.functional.cosine_similarity(a.double().flatten(), b.double().flatten(), dim=0))


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
E_, K_SLOTS, T_ = 6, 2, 162
COUNTS = [0, 1, 63, 64, 65, 130]          # rows per expert: none, one, one short of a tile, a tile, one over, two tiles and two rows


def _routing():
    """idx [T, k]: expert 5 in slot 0 of tokens 0 .. 129 and expert 4 on the other 32; slot 1: expert 4 (33), 3 (64), 2 (63), 1 (1) and one
    skipped slot (idx = E) -- a token never meets an expert twice -- then the tokens are shuffled"""
    c0 = torch.tensor([5] * 130 + [4] * 32)
    c1 = torch.tensor([4] * 33 + [3] * 64 + [2] * 63 + [1] + [E_])
    idx = torch.stack([c0, c1], 1)[torch.randperm(T_, generator=torch.Generator().manual_seed(5))]
    assert torch.bincount(idx.flatten(), minlength=E_ + 1).tolist() == COUNTS + [1]
    return idx.cuda()


def _padded(rows, cols, pad, dtype, gen, scale=1.0):
    """a [rows, cols] view of [rows, cols + pad] storage"""
    return (torch.randn(rows, cols + pad, generator=gen, device="cuda") * scale).to(dtype)[:, :cols]


def _problem(dtype, mode, N, K, gen):
    v, R = 16 // dtype.itemsize, T_ * K_SLOTS
    gr, xr = (R, T_) if mode == "gate_up" else (T_, R)
    G, X = _padded(gr, N, 3 * v, dtype, gen), _padded(xr, K, v, dtype, gen)
    W = (torch.randn(E_, N, K, generator=gen, device="cuda") * 0.05).to(dtype)
    w = (torch.rand(T_, K_SLOTS, generator=gen, device="cuda") + 0.1).to(dtype) if mode == "down" else None
    return G, X, W, w


def _ref(G, X, W, w, idx, mode):
    """-> (fp64 restatement on the rounded inputs, |W| sum_p |s G X|, rows per expert), from idx alone: the plan rows of an expert are its
    (token, slot) pairs in ascending order"""
    flat = idx.flatten()
    order = torch.sort(flat, stable=True).indices          # plan row -> t k + slot (skipped slots, idx = E, sort last)
    cnt = torch.bincount(flat, minlength=E_ + 1)[:E_].tolist()
    ref, mag, p0 = torch.zeros(W.shape, dtype=torch.float64, device="cuda"), torch.zeros(W.shape, dtype=torch.float64, device="cuda"), 0
    for e, n in enumerate(cnt):
        rows, src = torch.arange(p0, p0 + n, device="cuda"), order[p0:p0 + n]
        tok = src // K_SLOTS
        if mode == "gate_up":
            Gd, Xd = G[rows].double(), X[tok].double()
        else:
            Gd, Xd = G[tok].double() * (0.5 * w.flatten()[src].double())[:, None], X[rows].double()
        ref[e], mag[e] = W[e].double() * (Gd.T @ Xd), W[e].double().abs() * (Gd.abs().T @ Xd.abs())
        p0 += n
    return ref, mag, order, cnt


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("mode", ["gate_up", "down"])
def test_moe_wgrad_rel_vs_fp64(ops, dtype, mode):
    """N = 136, K = 264: off the 128 tile, on the grid of 8, two tiles each way.  Elementwise bar (tests/test_wgrad_gpu.py's):
    |W| sum_p |s G X| (2 rows_e 2^-24 [+ 2^-8 where the scale is folded into a bf16 operand: the down mode])"""
    N, K = 136, 264
    gen = torch.Generator(device="cuda").manual_seed(11 + (mode == "down"))
    idx = _routing()
    plan = ops.MoePlan(idx, E_)
    G, X, W, w = _problem(dtype, mode, N, K, gen)
    ref, mag, order, cnt = _ref(G, X, W, w, idx, mode)
    live = sum(cnt)
    assert cnt == COUNTS and torch.equal(plan.views()[2][:live].long(), order[:live])          # the restatement walks the plan's rows
    rows = torch.tensor(cnt, dtype=torch.float64, device="cuda")[:, None, None]
    fold = 2.0 ** -8 if dtype == BF16 and mode == "down" else 0.0
    out = torch.full((E_, N, K), float("nan"), device="cuda")
    assert ops.moe_wgrad_rel(G, X, W, plan, mode, w=w, out=out) is out
    err, bar = (out.double() - ref).abs(), mag * (2 * rows * 2.0 ** -24 + fold)
    worst = float((err / bar.clamp_min(1e-300)).max())
    print(f"[moe_wgrad_rel {dtype} {mode}] max err / bar {worst:.3f}  normalised max {float(err.max() / ref.abs().max()):.2e}")
    assert out.dtype == F32 and bool(torch.isfinite(out).all()) and bool((err <= bar).all()), worst
    assert bool((out[0] == 0).all())                                    # the expert without rows: exact zeros over the NaN prefill
    # bitwise repeatable
    again = ops.moe_wgrad_rel(G, X, W, plan, mode, w=w)
    assert torch.equal(again, out) and torch.equal(again, ops.moe_wgrad_rel(G, X, W, plan, mode, w=w))
    # accumulate: a second call over the same plan doubles the result; the zero-row expert's block keeps its bits
    acc = out.clone()
    acc[0] = torch.randn(N, K, generator=gen, device="cuda")
    before = acc[0].clone()
    assert ops.moe_wgrad_rel(G, X, W, plan, mode, w=w, out=acc, accumulate=True) is acc
    assert torch.equal(acc[0].view(torch.int32), before.view(torch.int32))
    err2, bar2 = (acc.double() - 2 * ref).abs()[1:], (2 * mag * (4 * rows * 2.0 ** -24 + fold))[1:]
    assert bool((err2 <= bar2).all()), float((err2 / bar2.clamp_min(1e-300)).max())


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("mode", ["gate_up", "down"])
def test_moe_wgrad_rel_mxfp4_is_bit_identical(ops, dtype, mode):
    """K = 256 (the format's rows of scale bytes sit on the 4-byte grid), N = 136"""
    N, K = 136, 256
    gen = torch.Generator(device="cuda").manual_seed(21)
    idx = _routing()
    plan = ops.MoePlan(idx, E_)
    G, X, W, w = _problem(dtype, mode, N, K, gen)
    q = ops.MoeQuantWeight(W)
    deq = q.dequant(dtype)
    assert not torch.equal(deq, W)
    a, b = ops.moe_wgrad_rel(G, X, q, plan, mode, w=w), ops.moe_wgrad_rel(G, X, deq, plan, mode, w=w)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    base = torch.randn(E_, N, K, generator=gen, device="cuda")
    a2 = ops.moe_wgrad_rel(G, X, q, plan, mode, w=w, out=base.clone(), accumulate=True)
    b2 = ops.moe_wgrad_rel(G, X, deq, plan, mode, w=w, out=base.clone(), accumulate=True)
    assert torch.equal(a2, b2) and torch.equal(a2[0], base[0])


def test_moe_wgrad_rel_refusals(ops):
    gen = torch.Generator(device="cuda").manual_seed(0)
    idx = _routing()
    plan = ops.MoePlan(idx, E_)
    G, X, W, w = _problem(BF16, "down", 64, 128, gen)
    R = T_ * K_SLOTS
    with pytest.raises(RuntimeError, match="LRP_ESHAPE"):               # N off the grid of 8
        ops.moe_wgrad_rel(G[:, :60], X, W[:, :60].contiguous(), plan, "down", w=w)
    with pytest.raises(RuntimeError, match="LRP_ESHAPE"):               # K off the grid of 8
        ops.moe_wgrad_rel(G, X[:, :124], W[:, :, :124].contiguous(), plan, "down", w=w)
    with pytest.raises(RuntimeError, match="LRP_EALIGN"):               # a row pitch off the 16-byte grid
        ops.moe_wgrad_rel(_padded(T_, 64, 4, BF16, gen), X, W, plan, "down", w=w)
    with pytest.raises(RuntimeError, match="LRP_EALIGN"):               # a base off the 16-byte grid
        ops.moe_wgrad_rel(G, torch.zeros(R * 136 + 4, device="cuda", dtype=BF16)[4:].view(R, 136)[:, :128], W, plan, "down", w=w)
    with pytest.raises(TypeError):
        ops.moe_wgrad_rel(G, X.float(), W, plan, "down", w=w)
    with pytest.raises(TypeError):
        ops.moe_wgrad_rel(G, X, W.float(), plan, "down", w=w)
    with pytest.raises(TypeError):
        ops.moe_wgrad_rel(G, X, W, plan, "down", w=w.float())
    with pytest.raises(ValueError):
        ops.moe_wgrad_rel(G, X, W, plan, "down")                         # the down mode needs the routing weights
    with pytest.raises(ValueError):
        ops.moe_wgrad_rel(G, X, W, plan, "down", w=w, accumulate=True)
    with pytest.raises(ValueError):
        ops.moe_wgrad_rel(G, X, W, plan, "gate_up")                      # G / X swapped roles: the shapes are the other mode's
    with pytest.raises(ValueError):
        ops.moe_wgrad_rel(G, X, W, plan, "both", w=w)
    with pytest.raises(ValueError):
        ops.moe_wgrad_rel(G, X, W.transpose(1, 2).contiguous().transpose(1, 2), plan, "down", w=w)
    with pytest.raises(RuntimeError):
        ops.moe_wgrad_rel(G.cpu(), X.cpu(), W.cpu(), plan, "down", w=w.cpu())


# ---- the fp32 engine against the reference -----------------------------------------------------------------------------------------------
def keep(out):
    return {k: ({n: t.clone() for n, t in v.items()} if isinstance(v, dict) else v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def fp32_case(case):
    """one fp32 engine per case and its explanation with every matrix and the expert read-out, shared by the tests below"""
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    eng = Qwen3MoeLRP.from_hf(build_qwen3_moe(case), dtype=F32, device="cuda", max_seq=128)
    ids = inputs(case)[0]
    return eng, ids, keep(eng.explain(ids, moe_weights=NAMES, experts=True))


def _tiny_fixture():
    head = load("moe_weight_relevance_tiny.npz")
    gu = np.stack([np.concatenate([load(f"moe_weight_relevance_tiny_gate_up_l{l}_e{a}.npz")["gate_up"] for a in (0, 4)]) for l in head["moe"]])
    dn = np.stack([load(f"moe_weight_relevance_tiny_down_l{l}.npz")["down"] for l in head["moe"]])
    return head, dict(qkv=head["qkv"], o=head["o"], router=head["router"], gate_up=gu, down=dn)


def _identity(out, moe):
    """the per-expert totals of gate_up and of down against sum_b R_expert of the same call -> normalised max of each"""
    R = out["R_expert"].double().sum(1)[moe]
    return {n: _gnmax(out["R_W"][n].double().sum((2, 3)), R) for n in ("gate_up", "down")}


def test_fp32_engine_vs_reference_tiny(ops):
    eng, ids, out = fp32_case("tiny")
    head, ref = _tiny_fixture()
    assert out["idx"].tolist() == head["idx"].tolist() and out["weight_layers"] == [0, 1, 2] and out["weight_layers_moe"] == head["moe"].tolist()
    errs = {}
    for n in NAMES:
        assert out["R_W"][n].shape == ref[n].shape and out["R_W"][n].dtype == F32, n
        errs[n] = max(nmax(out["R_W"][n][j], ref[n][j]) for j in range(ref[n].shape[0]))          # per matrix: the worst layer
    print("[fp32 R_W tiny] vs reference fp64 (worst layer): " + "  ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert max(errs.values()) <= BAR
    ident = _identity(out, head["moe"].tolist())
    print(f"[fp32 tiny] per-expert totals vs R_expert.sum(1) of the same call: {ident}")
    assert max(ident.values()) <= BAR


def test_fp32_engine_vs_reference_fanout(ops):
    """E = 128: judged on the row sums of every expert and on the full matrices of three experts per layer (0 rows, 1 row, the most loaded)"""
    eng, ids, out = fp32_case("fanout")
    head, dense = load("moe_weight_relevance_fanout.npz"), load("moe_weight_relevance_fanout_dense.npz")
    moe = head["moe"].tolist()
    assert out["idx"].tolist() == head["idx"].tolist() and out["weight_layers_moe"] == moe
    R = out["R_W"]
    errs = {n: max(nmax(R[n][j], dense[n][j]) for j in range(dense[n].shape[0])) for n in ("qkv", "o", "router")}
    for n in ("gate_up", "down"):
        assert R[n].shape[:2] == (len(moe), 128)
        errs[n + "_rowsum"] = max(nmax(R[n][j].double().sum(-1), head[n + "_rowsum"][j]) for j in range(len(moe)))
    empty = torch.from_numpy(head["counts"] == 0).cuda()
    assert bool(empty.any()) and bool((R["gate_up"][empty] == 0).all()) and bool((R["down"][empty] == 0).all())
    for j, l in enumerate(moe):
        lay, chosen = load(f"moe_weight_relevance_fanout_l{l}.npz"), head["chosen"][j].tolist()
        assert head["chosen_rows"][j, 0] == 0 and head["chosen_rows"][j, 1] == 1
        for n in ("gate_up", "down"):
            assert bool((R[n][j, chosen[0]] == 0).all()) and not lay[n][0].any()
            for i in (1, 2):
                errs[f"{n}_l{l}_rows{head['chosen_rows'][j, i]}"] = nmax(R[n][j, chosen[i]], lay[n][i])
    print("[fp32 R_W fanout] vs reference fp64: " + "  ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert max(errs.values()) <= BAR
    ident = _identity(out, moe)
    print(f"[fp32 fanout] per-expert totals vs R_expert.sum(1) of the same call: {ident}")
    assert max(ident.values()) <= BAR


def test_left_padded_batch_is_the_sum_of_its_prompts(ops):
    """fp32: two evaluation orders of the same sums (1e-5, the dense test's bar)"""
    eng, ids, _ = fp32_case("tiny")
    S, n1 = ids.shape[1], 41
    other = torch.randint(1, 256, (n1,), generator=torch.Generator().manual_seed(77))
    batch = torch.stack([ids[0], torch.cat([torch.zeros(S - n1, dtype=ids.dtype), other])])
    out = eng.explain(batch, lengths=[S, n1], moe_weights=NAMES)
    a = eng.explain(ids, moe_weights=NAMES, target=out["idx"][:1])["R_W"]
    b = eng.explain(other[None], moe_weights=NAMES, target=out["idx"][1:])["R_W"]
    errs = {n: _gnmax(out["R_W"][n], a[n] + b[n]) for n in NAMES}
    print(f"[left-padded batch vs the sum of its prompts, fp32] {errs}")
    assert max(errs.values()) <= 1e-5


OTHERS = ("R_tok", "logit", "idx", "logits", "layer_R", "R_trace", "R_resid", "R_expert", "expert_index", "R_block", "R_head_out")


def test_weights_out_weight_layers_and_nothing_else_moves(ops, monkeypatch):
    eng, ids, full = fp32_case("tiny")
    kw = dict(experts=True, layer_relevance=True, latent=("trace", "resid"), heads=("out",))
    plain = keep(eng.explain(ids, **kw))
    with_w = eng.explain(ids, moe_weights=NAMES, **kw)
    for k in OTHERS:
        assert torch.equal(with_w[k], plain[k]), k
    assert not {"R_W", "weight_layers", "weight_layers_moe"} & set(plain)
    for n in NAMES:
        assert torch.equal(with_w["R_W"][n], full["R_W"][n]), n
    # weight_layers / a subset of the names: the same bits as the slices of the full result
    part = eng.explain(ids, moe_weights=["down", "qkv", "router"], weight_layers=[1, 2])
    assert part["weight_layers"] == [1, 2] and part["weight_layers_moe"] == [2] and set(part["R_W"]) == {"down", "qkv", "router"}
    assert torch.equal(part["R_W"]["qkv"], full["R_W"]["qkv"][[1, 2]])
    assert torch.equal(part["R_W"]["down"], full["R_W"]["down"][[1]]) and torch.equal(part["R_W"]["router"], full["R_W"]["router"][[1]])
    dense_only = eng.explain(ids, moe_weights=["qkv", "o"], weight_layers=[1])
    assert dense_only["weight_layers_moe"] == [] and torch.equal(dense_only["R_W"]["o"], full["R_W"]["o"][[1]])
    # weights_out: two calls accumulate in place into the first call's tensors
    other = torch.randint(0, 256, ids.shape, generator=torch.Generator().manual_seed(78))
    r1 = keep(eng.explain(other, moe_weights=NAMES))["R_W"]
    acc = {n: t.clone() for n, t in full["R_W"].items()}
    res = eng.explain(other, moe_weights=NAMES, weights_out=acc)
    for n in NAMES:
        assert res["R_W"][n] is acc[n] and torch.equal(acc[n], full["R_W"][n] + r1[n]), n
    # refusals, before any kernel
    with pytest.raises(ValueError, match="routed experts"):
        eng.explain(ids, weights="o")
    with pytest.raises(ValueError, match="graph"):
        eng.explain(ids, moe_weights=NAMES, graph=True)
    with pytest.raises(ValueError, match="sparse"):
        eng.explain(ids, moe_weights="router", weight_layers=[1])
    with pytest.raises(ValueError, match="weights_out"):
        eng.explain(ids, moe_weights=NAMES, weights_out=dict(acc, down=acc["down"][:1]))
    with pytest.raises(ValueError):
        eng.explain(ids, weight_layers=[0])
    # moe_weights=None launches nothing

    def boom(*a, **k):
        raise AssertionError("a wgrad kernel launched without a request")
    monkeypatch.setattr(ops, "wgrad_rel", boom)
    monkeypatch.setattr(ops, "moe_wgrad_rel", boom)
    again = eng.explain(ids, **kw)
    for k in OTHERS:
        assert torch.equal(again[k], plain[k]), k
    with pytest.raises(AssertionError):
        eng.explain(ids, moe_weights="o")
    with pytest.raises(AssertionError):
        eng.explain(ids, moe_weights="down")


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_mxfp4_engine_equals_the_engine_on_its_dequantised_experts(ops, dtype):
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    ids = inputs("tiny")[0]
    q = Qwen3MoeLRP.from_hf(build_qwen3_moe("tiny"), dtype=dtype, device="cuda", max_seq=64, weight_format="mxfp4")
    ctl = Qwen3MoeLRP(*q.dequantized_weights(), dtype=dtype, device="cuda", max_seq=64)
    assert isinstance(q.layers[0]["wgu_e"], ops.MoeQuantWeight) and torch.is_tensor(ctl.layers[0]["wgu_e"])
    a, b = q.explain(ids, moe_weights=NAMES), ctl.explain(ids, moe_weights=NAMES)
    assert torch.equal(a["R_tok"], b["R_tok"])
    for n in NAMES:
        assert torch.equal(a["R_W"][n], b["R_W"][n]) and bool(torch.isfinite(a["R_W"][n]).all()), n


# ---- bf16: the planted-routing model (tests/golden/moe_engine_models.py) -------------------------------------------------------------------
FUSED_B = 384          # tests/test_qwen_moe_engine_gpu.py: the smallest batch whose attention-half GEMMs reach the fused kernels


@functools.lru_cache(maxsize=None)
def planted():
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    model, ids = mm.build(), mm.inputs()
    f32 = Qwen3MoeLRP.from_hf(model, dtype=F32, device="cuda", max_seq=mm.S)
    bf = Qwen3MoeLRP.from_hf(model, dtype=BF16, device="cuda", max_seq=mm.S)
    return ids, f32, bf


def test_bf16_engine_against_the_fp32_engine(ops):
    """per matrix over the whole tensor, the bars tests/test_wgrad_gpu.py uses for this quantity in bf16: normalised max <= 5e-2, cosine >=
    0.995.  Some experts hold more than 64 rows (asserted): the multi-tile loop runs in the engine too"""
    ids, f32, bf = planted()
    assert not bf._attn_fused(ids.numel())
    out = bf.explain(ids, moe_weights=NAMES, experts=True)
    ref = f32.explain(ids, moe_weights=NAMES, experts=True, target=out["idx"])
    assert torch.equal(out["expert_index"], ref["expert_index"])
    rows = torch.bincount(out["expert_index"][0].flatten(), minlength=8)
    assert int(rows.max()) > 64, rows.tolist()
    res = {n: (_gnmax(out["R_W"][n], ref["R_W"][n]), _cosine(out["R_W"][n], ref["R_W"][n])) for n in NAMES}
    print(f"[bf16 planted R_W, rows per expert of layer 0 {rows.tolist()}] vs fp32 engine (nmax, cosine): "
          + "  ".join(f"{n} {e:.2e} {c:.5f}" for n, (e, c) in res.items()))
    for n in NAMES:
        assert bool(torch.isfinite(out["R_W"][n]).all())
        assert res[n][0] <= 5e-2 and res[n][1] >= 0.995, (n, res[n])


def test_bf16_engine_fused_attention_half(ops):
    """the request at FUSED_B prompts, where the attention half of every layer runs fused_attn_bwd (asserted) and hands qkv / o to the sink
    there, against the kernel-by-kernel path: the same prompts in two halves that stay below the fused kernels' gate (asserted), accumulated
    through weights_out.  The same bf16 bars"""
    ids, f32, bf = planted()
    more = torch.randint(0, 256, (FUSED_B - ids.shape[0], ids.shape[1]), generator=torch.Generator().manual_seed(11))
    batch = torch.cat([ids, more])
    assert bf._attn_fused(batch.numel()) and not bf._attn_fused(batch.numel() // 2)
    out = bf.explain(batch, moe_weights=NAMES)
    for n in NAMES:
        assert bool(torch.isfinite(out["R_W"][n]).all()), n
    h = FUSED_B // 2
    acc = bf.explain(batch[:h], moe_weights=NAMES, target=out["idx"][:h])["R_W"]
    bf.explain(batch[h:], moe_weights=NAMES, target=out["idx"][h:], weights_out=acc)
    res = {n: (_gnmax(out["R_W"][n], acc[n]), _cosine(out["R_W"][n], acc[n])) for n in NAMES}
    print(f"[bf16 planted R_W, B={FUSED_B} fused attention half] vs kernel by kernel (nmax, cosine): "
          + "  ".join(f"{n} {e:.2e} {c:.5f}" for n, (e, c) in res.items()))
    for n in ("qkv", "o"):
        assert res[n][0] <= 5e-2 and res[n][1] >= 0.995, (n, res[n])
