"""GPU: MXFP4 expert weights read inside the grouped expert GEMMs (ops.MoeQuantWeight, lrp_moe_*_q; Qwen3MoeLRP(weight_format="mxfp4")).
Every decoded value is exact in bf16 and fp32 and lands where the unquantised staging puts it, so the contract is BIT-IDENTITY with
"lrp_mxfp4_dequant, then the unquantised op / engine" -- the tests below hold the ops and the whole engine to torch.equal; the fp32 engine is
also held to the real reference run on the quantise-dequantise images of the experts (tests/golden/make_golden_mxfp4_qwen3_moe.py) at the
project's fp32 bar."""
import functools

import pytest
import torch

from tests.golden import moe_engine_models as mm
from tests.golden.moe_models import build_qwen3_moe, inputs, model_case
from tests.util import load, nmax, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 1e-4          # the project's fp32 engine bar (tests/test_qwen_moe_engine_gpu.py)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a HIP device")


def keep(out):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}


# ---- 1: storage ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_storage_is_the_2d_format_on_the_flat_view(dtype):
    _need_gpu()
    from lxt_amd import ops
    g = torch.Generator().manual_seed(3)
    E, N, K = 5, 136, 384          # (K / 32 = 12 scale bytes per row: rows stay on the 4-byte grid, K % 128 == 0 as H and I are)
    w = (torch.randn(E, N, K, generator=g) * torch.exp2(torch.randint(-12, 13, (E, N, K // 32, 1), generator=g).float()).expand(E, N, K // 32, 32)
         .reshape(E, N, K)).to(dtype).to(DEV)
    q = ops.MoeQuantWeight(w)
    assert q.shape == (E, N, K) and q.codes.shape == (E, N, K // 2) and q.scales.shape == (E, N, K // 32)
    assert q.codes.dtype == torch.uint8 and q.scales.dtype == torch.uint8 and q.nbytes() == E * N * K * 17 // 32
    codes, scales = ops.mxfp4_quantize(w.view(E * N, K))
    assert torch.equal(q.codes.view(E * N, -1), codes) and torch.equal(q.scales.view(E * N, -1), scales)
    want = ops.mxfp4_dequant(codes, scales, torch.empty(E * N, K, device=DEV, dtype=dtype))
    got = q.dequant(dtype)
    assert got.shape == (E, N, K) and got.dtype == dtype and torch.equal(got.view(E * N, K), want)
    q2 = ops.MoeQuantWeight(got)          # the round trip reproduces the bytes
    assert torch.equal(q2.codes, q.codes) and torch.equal(q2.scales, q.scales)
    with pytest.raises(ValueError, match="K % 128"):
        ops.MoeQuantWeight(w[:, :, :160].contiguous())


# ---- 2: the four ops, bit for bit ----------------------------------------------------------------------------------------------------------
def _bytes(E, N, K, seed):
    """codes / scales built as bytes: every code in both nibbles (-0 = code 8 included), scale bytes in [100, 140], and in EVERY expert
    blocks with E = 0, 1, 2 (subnormal products) and one all-zero block.  No E >= 253 (inf would make the comparison NaN != NaN)."""
    from lxt_amd import ops
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 256, (E, N, K // 2), generator=g, dtype=torch.uint8)
    codes[:, 3, :16] = (torch.arange(16) | (torch.arange(16).flip(0) << 4)).to(torch.uint8)      # all 16 codes, low and high nibble
    scales = torch.randint(100, 141, (E, N, K // 32), generator=g, dtype=torch.uint8)
    scales[:, 0, 0], scales[:, 0, 1], scales[:, 1, 0] = 0, 1, 2
    codes[:, 2, :16] = 0
    both = torch.stack((codes & 15, codes >> 4))
    assert all(bool((both == c).any()) for c in range(16)) and int(scales.max()) <= 140
    return ops.MoeQuantWeight.from_bytes(codes.to(DEV), scales.to(DEV))


def _planted_idx(E, k, T, counts, seed):
    """[T, k] expert indices with the given row counts per expert and ONE skipped slot (idx = E), in seeded order"""
    assert sum(counts) == T * k - 1 and len(counts) == E
    flat = torch.cat([torch.full((n,), e, dtype=torch.int64) for e, n in enumerate(counts)] + [torch.tensor([E])])
    return flat[torch.randperm(T * k, generator=torch.Generator().manual_seed(seed))].view(T, k)


def _topk_idx(E, k, T, seed):
    return torch.rand(T, E, generator=torch.Generator().manual_seed(seed)).argsort(1)[:, :k].contiguous()


OP_CASES = {
    # row counts 0, 1, 127, 128, 129 (tile edges) and a skipped slot
    "edges": dict(E=8, k=2, T=260, H=256, I=256, idx=lambda: _planted_idx(8, 2, 260, [0, 1, 127, 128, 129, 60, 70, 4], 1)),
    # the real fan-out, the shortest K loop, most experts with 0-3 rows
    "fanout": dict(E=128, k=8, T=48, H=128, I=128, idx=lambda: _topk_idx(128, 8, 48, 2)),
    # three N tiles, more than two K stages
    "tiles": dict(E=4, k=2, T=64, H=512, I=384, idx=lambda: _topk_idx(4, 2, 64, 3)),
}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", sorted(OP_CASES))
def test_four_ops_bit_for_bit(case, dtype):
    _need_gpu()
    from lxt_amd import ops
    c = OP_CASES[case]
    E, k, T, H, I = (c[n] for n in ("E", "k", "T", "H", "I"))
    g = torch.Generator().manual_seed(17)
    qgu, qd = _bytes(E, 2 * I, H, 5), _bytes(E, H, I, 6)
    wgu, wd = qgu.dequant(dtype), qd.dequant(dtype)
    assert wgu.dtype == dtype and bool(torch.isfinite(wgu).all()) and bool(torch.isfinite(wd).all())
    assert bool((wgu[:, 0, :32].abs().max() < 1e-36)) and bool((wgu[:, 0, :32] != 0).any())          # the E = 0 block is there, subnormal
    idx = c["idx"]().to(DEV)
    plan = ops.MoePlan(idx, E)
    cnt = plan.views()[0].cpu().tolist()
    if case == "edges":
        assert cnt == [0, 1, 127, 128, 129, 60, 70, 4] and int((idx == E).sum()) == 1
    R = T * k
    rnd = lambda *s: torch.randn(*s, generator=g).to(dtype).to(DEV)      # noqa: E731
    x, G, m_in, coef_in, Agu_in = rnd(T, H), rnd(T, H), rnd(R, I), rnd(R, 2 * I), rnd(R, 2 * I)
    w = torch.rand(T, k, generator=g).to(dtype).to(DEV)
    live = plan.views()[3].view(T, k) >= 0          # (a skipped slot has no plan row)
    nrows = int(live.sum())
    for act in (("silu", "gelu_tanh") if case == "edges" else ("silu",)):
        want, got = ops.moe_gate_up_fwd(x, wgu, plan, act), ops.moe_gate_up_fwd(x, qgu, plan, act)
        for name, a, b in zip(("coef", "m"), want, got):
            assert bool(torch.isfinite(a[:nrows]).all()), (name, act)
            assert torch.equal(a[:nrows], b[:nrows]), (name, act)
    want, got = ops.moe_down_fwd(m_in, wd, plan), ops.moe_down_fwd(m_in, qd, plan)
    assert bool(torch.isfinite(want[:nrows]).all()) and torch.equal(want[:nrows], got[:nrows]), "y"
    (Aw, gww), (Ag, gwg) = ops.moe_down_dgrad(G, wd, coef_in, m_in, w, plan), ops.moe_down_dgrad(G, qd, coef_in, m_in, w, plan)
    assert bool(torch.isfinite(Aw[:nrows]).all()) and bool(torch.isfinite(gww).all())
    assert torch.equal(Aw[:nrows], Ag[:nrows]), "Agu"
    assert torch.equal(gww, gwg), "G_w"
    want, got = ops.moe_gate_up_dgrad(Agu_in, wgu, plan), ops.moe_gate_up_dgrad(Agu_in, qgu, plan)
    assert bool(torch.isfinite(want[:nrows]).all()) and torch.equal(want[:nrows], got[:nrows]), "gx"
    assert float(want[:nrows].abs().max()) > 0 and float(Aw[:nrows].abs().max()) > 0


# ---- 3: the engine against the real reference -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def quant_case(case):
    """the quantised engine of a case, its control (an ordinary engine on the dequantised weights) and what both explain"""
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    if case == "planted":
        model, ids, lengths, dtype, S = mm.build(), mm.inputs(), None, torch.bfloat16, mm.S
    else:
        model, (ids, am, _), dtype, S = build_qwen3_moe(model_case(case)), inputs(case), torch.float32, 128
        lengths = am.sum(1) if case == "padded" else None
    eng = Qwen3MoeLRP.from_hf(model, dtype=dtype, device=DEV, max_seq=S, weight_format="mxfp4")
    ctl = Qwen3MoeLRP(*eng.dequantized_weights(), dtype=dtype, device=DEV, max_seq=S)
    full = dict(experts=True, layer_relevance=True, latent=("trace", "resid"))
    outs = [keep(e.explain(ids, lengths=lengths, **kw)) for e in (eng, ctl) for kw in ({}, full)]
    return eng, ctl, ids, outs


def test_fp32_engine_against_the_reference_on_quantised_experts():
    _need_gpu()
    fx = load("mxfp4_qwen3_moe_tiny.npz")
    assert float(fx["margin"]) >= 1e-4 and float(fx["ref_fp32_gap"]) <= 1e-5          # the generator's own conditions
    eng, _, ids, (_, full, _, _) = quant_case("tiny")
    assert torch.equal(ids, t(fx["ids"]))
    assert full["idx"].tolist() == fx["idx"].tolist()
    assert torch.equal(full["expert_index"].cpu(), t(fx["expert_index"]))
    for k in ("R_tok", "R_expert", "R_block"):
        err = nmax(full[k].cpu(), fx[k])
        print(f"[tiny, mxfp4 experts] {k} vs reference fp64 {err:.2e}")
        assert err <= BAR, (k, err)
    wd = eng.layers[0]["wd_e"]
    assert torch.equal(wd.codes.cpu(), t(fx["wd_codes"])) and torch.equal(wd.scales.cpu(), t(fx["wd_scales"]))


# ---- 4: engine bit-identity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tiny", "fanout", "padded", "planted"])
def test_engine_is_bit_identical_to_the_engine_on_dequantised_weights(case):
    _need_gpu()
    eng, ctl, ids, (plain_q, full_q, plain_c, full_c) = quant_case(case)
    assert eng.dtype == (torch.bfloat16 if case == "planted" else torch.float32) and ctl.flat_q is None and eng.flat_q is not None
    for k in ("R_tok", "logit", "logits", "idx"):
        assert torch.equal(plain_q[k], plain_c[k]), k
        assert bool(torch.isfinite(plain_c[k].float()).all()), k
    assert set(full_q) == set(full_c) and {"R_expert", "expert_index", "R_block", "layer_R", "R_trace", "R_resid"} <= set(full_q)
    for k, v in full_c.items():
        if torch.is_tensor(v):
            assert torch.equal(full_q[k], v), k
        else:
            assert full_q[k] == v, k
    assert float(full_c["R_expert"].abs().max()) > 0


# ---- 5: resident state ------------------------------------------------------------------------------------------------------------------------
def test_resident_state_is_codes_and_scales_only():
    _need_gpu()
    from lxt_amd import ops
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    eng, ctl, *_ = quant_case("tiny")
    c = eng.cfg
    n_sparse, Ne, H, I = sum(c["moe_layers"]), c["n_experts"], c["hidden"], c["moe_inter"]
    lo, hi = eng.flat_q.data_ptr(), eng.flat_q.data_ptr() + eng.flat_q.numel()
    assert eng.flat_q.dtype == torch.uint8 and eng.weight_format is None and eng.scratch is None          # (the base class sees no format)
    for Lw in eng.layers:
        for k, v in Lw.items():
            if k in ("wgu_e", "wd_e"):
                assert isinstance(v, ops.MoeQuantWeight)
                for b in (v.codes, v.scales):
                    assert b.dtype == torch.uint8 and lo <= b.data_ptr() and b.data_ptr() + b.numel() <= hi and b.data_ptr() % 128 == 0
            else:
                assert torch.is_tensor(v) and v.dim() <= 2, k          # vectors and matrices of `flat`: no [E, N, K] floating-point tensor
                assert eng.flat.data_ptr() <= v.data_ptr() < eng.flat.data_ptr() + eng.flat.numel() * 4, k
        assert ("wr" in Lw) == ("wgu_e" in Lw)
    wb, wc = eng.weight_bytes(), ctl.weight_bytes()
    assert wb["experts"] == n_sparse * Ne * 3 * H * I // 2 + n_sparse * Ne * 3 * H * I // 32
    assert wc["experts"] == n_sparse * Ne * 3 * H * I * 4 and wb["scratch"] == 0
    assert wb["resident"] == eng.flat.numel() * 4 + eng.flat_q.numel() and wb["experts"] <= eng.flat_q.numel() < wb["experts"] + 128 * 4 * n_sparse
    assert eng.flat.numel() == ctl.flat.numel()
    # a non-finite expert weight is refused at load, naming the layer
    model = build_qwen3_moe("tiny")
    with torch.no_grad():
        model.model.layers[2].mlp.experts.down_proj[3, 5, 7] = float("nan")
    with pytest.raises(ValueError, match="layer 2"):
        Qwen3MoeLRP.from_hf(model, dtype=torch.float32, device=DEV, max_seq=64, weight_format="mxfp4")
    with pytest.raises(ValueError, match="weight_format must be"):
        Qwen3MoeLRP.from_hf(model, dtype=torch.float32, device=DEV, weight_format="int4")
    for bad in (dict(graph=True), dict(latent="mlp")):
        with pytest.raises(ValueError):
            eng.explain(inputs("tiny")[0], **bad)
    with pytest.raises(NotImplementedError, match="explicit"):
        eng.set_mode("explicit")


# ---- 6: the default is untouched ----------------------------------------------------------------------------------------------------------------
def test_default_engine_is_untouched(monkeypatch):
    _need_gpu()
    from lxt_amd import ops
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP

    def boom(*a, **k):
        raise AssertionError("the default engine touches nothing of the MXFP4 path")
    for name in ("lrp_moe_gate_up_fwd_q", "lrp_moe_down_fwd_q", "lrp_moe_down_dgrad_q", "lrp_moe_gate_up_dgrad_q"):
        monkeypatch.setattr(ops.lib, name, boom)
    monkeypatch.setattr(ops, "mxfp4_dequant", boom)
    monkeypatch.setattr(ops, "mxfp4_quantize", boom)
    model = build_qwen3_moe("tiny")
    eng = Qwen3MoeLRP.from_hf(model, dtype=torch.float32, device=DEV, max_seq=64)
    assert eng.expert_format is None and eng.flat_q is None and eng.scratch is None
    assert all(torch.is_tensor(Lw[k]) and Lw[k].dtype == torch.float32 for Lw in eng.layers if "wr" in Lw for k in ("wgu_e", "wd_e"))
    out = eng.explain(inputs("tiny")[0], experts=True)
    assert bool(torch.isfinite(out["R_tok"]).all()) and bool(torch.isfinite(out["R_expert"]).all())
    with pytest.raises(AssertionError, match="MXFP4 path"):          # (the guard is live: a quantised engine does reach what was replaced)
        Qwen3MoeLRP.from_hf(model, dtype=torch.float32, device=DEV, max_seq=64, weight_format="mxfp4")
