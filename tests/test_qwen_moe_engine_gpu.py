"""GPU: the fused Qwen3-MoE driver (lxt_amd.engine_qwen_moe.Qwen3MoeLRP).
fp32 engine: the drop-in's fixtures from the real reference (hf_qwen3_moe_*.npz: same explained token, logit and R_tok at the bar
tests/moe_worker.py applies to them) and the expert fixtures (qwen3_moe_experts_*.npz: expert_index equal, R_expert <= 1e-4), left padding,
the 1/2-identity, the read-outs carried over from QwenLRP and the refusals.
bf16 engine: on the planted-routing model (tests/golden/moe_engine_models.py) the same routing as the fp32 engine, and an error against the
fp32 engine of at most twice what the bf16 DROP-IN shows against it (tests/qwen_moe_dropin_worker.py) -- both round the same operands in
different GEMM orders, a factor 2 separates rounding from a bug; once with 2 prompts of 128 tokens (every GEMM kernel by kernel) and once
with the same two prompts inside a batch large enough that the attention half takes the fused launch sequence."""
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from tests.golden import moe_engine_models as mm
from tests.golden.moe_models import build_qwen3_moe, model_case, wsum
from tests.util import load, nmax, t

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CASES = ("tiny", "fanout", "padded")
BAR = 1e-4          # tests/moe_worker.py: R_tok of the fp32 drop-in against the reference; the project's fp32 engine bar for read-outs


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a HIP device")


def cos(a, b):
    a, b = torch.as_tensor(a).double().flatten().cpu(), torch.as_tensor(b).double().flatten().cpu()
    return float(a @ b / (a.norm() * b.norm()))


def keep(out):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def fp32_case(case):
    """one engine and two explanations per case, shared by the tests below: plain, and with every read-out"""
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    fx, fe = load(f"hf_qwen3_moe_{case}.npz"), load(f"qwen3_moe_experts_{case}.npz")
    model = build_qwen3_moe(model_case(case))
    assert abs(wsum(model) - float(fx["wsum"])) < 1e-6 * float(fx["wsum"]), "weights did not reproduce"
    eng = Qwen3MoeLRP.from_hf(model, dtype=torch.float32, device="cuda", max_seq=128)
    ids, valid = t(fx["ids"]), t(fx["mask"]).bool()
    lengths = valid.sum(1) if case == "padded" else None
    plain = keep(eng.explain(ids, lengths=lengths))
    full = keep(eng.explain(ids, lengths=lengths, experts=True, layer_relevance=True, latent=("trace", "resid"), heads=("out",), attn_map="sum"))
    return eng, fx, fe, ids, valid, lengths, plain, full


@pytest.mark.parametrize("case", CASES)
def test_fp32_engine_against_the_reference(case):
    _need_gpu()
    eng, fx, fe, ids, valid, lengths, plain, full = fp32_case(case)
    assert plain["idx"].tolist() == fx["idx"].tolist()
    assert torch.allclose(plain["logit"].cpu(), t(fx["logit"]), rtol=1e-4, atol=1e-5), (plain["logit"], fx["logit"])
    for b in range(ids.shape[0]):
        R = plain["R_tok"][b].cpu()
        e32, e64 = nmax(R[valid[b]], t(fx["R_tok"])[b][valid[b]]), nmax(R[valid[b]], t(fx["R_tok_fp64"])[b][valid[b]])
        print(f"[{case} row {b}] R_tok vs reference fp32 {e32:.2e} | fp64 {e64:.2e}")
        assert max(e32, e64) < BAR
        assert bool((R[~valid[b]] == 0).all())                     # pad columns: exactly 0
    index, R_expert = full["expert_index"].cpu(), full["R_expert"].cpu()
    assert index.dtype == torch.int64 and R_expert.dtype == torch.float32
    want = t(fe["expert_index"])
    for b in range(ids.shape[0]):
        assert torch.equal(index[:, b][:, valid[b]], want[:, b][:, valid[b]])
        err = nmax(R_expert[:, b], fe["R_expert"][:, b])
        print(f"[{case} row {b}] R_expert vs reference fp64 {err:.2e}")
        assert err <= BAR
    for li, moe in enumerate(eng.cfg["moe_layers"]):
        if not moe:
            assert bool((R_expert[li] == 0).all()) and bool((index[li] == -1).all())
    # sum_e R_expert = 1/2 of the relevance at the sparse block's output, read by the ENGINE off the block's own output and the gradient
    # that reaches it (ops.readout: independent of the router read-out), and that read-out against the reference's out * out.grad
    R_block = full["R_block"].cpu().double()
    half, blk = nmax(R_expert.double().sum(-1), 0.5 * R_block), nmax(R_block, t(fe["R_block"]))
    print(f"[{case}] sum_e R_expert vs 1/2 R_block of the same call {half:.2e}; R_block vs reference {blk:.2e}")
    assert half <= BAR and blk <= BAR


@pytest.mark.parametrize("case", CASES)
def test_experts_keyword_changes_nothing_else(case):
    _need_gpu()
    eng, fx, fe, ids, valid, lengths, plain, full = fp32_case(case)
    for k in ("R_tok", "logit", "idx", "logits"):
        assert torch.equal(plain[k], full[k]), k
    assert not {"R_expert", "expert_index", "R_block"} & set(plain)
    again = eng.explain(ids, lengths=lengths, experts=True)
    assert torch.equal(again["R_expert"], full["R_expert"]) and torch.equal(again["expert_index"], full["expert_index"])


def test_padded_prompt_equals_the_prompt_alone():
    _need_gpu()
    eng, fx, fe, ids, valid, lengths, plain, full = fp32_case("padded")
    b = 1
    alone = eng.explain(ids[b, valid[b]][None], experts=True)
    assert int(alone["idx"][0]) == int(full["idx"][b])
    err = nmax(full["R_expert"][:, b], alone["R_expert"][:, 0])
    print(f"padded prompt against itself alone: R_expert {err:.2e}")
    assert err <= BAR
    assert nmax(full["R_tok"][b].cpu()[valid[b]], alone["R_tok"][0]) <= BAR
    assert torch.equal(full["expert_index"][:, b][:, valid[b]].cpu(), alone["expert_index"][:, 0].cpu())
    # pad tokens contribute exactly 0: G_w is exactly 0 on their rows, so prompt b's experts carry only what its own tokens give
    only = torch.zeros(eng.cfg["n_experts"], dtype=torch.bool)
    for li, moe in enumerate(eng.cfg["moe_layers"]):
        if moe:
            only.zero_()
            only[full["expert_index"][li, b][valid[b]].cpu().flatten()] = True
            assert bool((full["R_expert"][li, b].cpu()[~only] == 0).all())


@pytest.mark.parametrize("case", CASES)
def test_carried_over_read_outs(case):
    """layer_relevance, the latent trace / resid read-outs, per-head relevance and the attention map run as in QwenLRP and keep their
    identities: R_trace sums to layer_R, R_resid to it as well, a map row to R_head_out"""
    _need_gpu()
    eng, fx, fe, ids, valid, lengths, plain, full = fp32_case(case)
    nL = len(eng.layers)
    assert full["layer_R"].shape == (nL + 1, ids.shape[0]) and full["R_trace"].shape == (nL + 1, *ids.shape)
    assert nmax(full["R_trace"].sum(-1), full["layer_R"]) <= BAR and nmax(full["R_resid"].sum(-1), full["layer_R"]) <= BAR
    assert torch.equal(full["R_trace"][0], full["R_tok"])
    assert nmax(full["R_attn"].sum(-1), full["R_head_out"].sum(2)) <= BAR
    for b in range(ids.shape[0]):
        assert bool((full["R_attn"][:, b][:, ~valid[b]] == 0).all()) and bool((full["R_head_out"][:, b][:, :, ~valid[b]] == 0).all())


def test_refusals():
    _need_gpu()
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    eng, fx, fe, ids, *_ = fp32_case("tiny")
    with pytest.raises(ValueError, match="mlp"):
        eng.explain(ids, latent="mlp")
    with pytest.raises(ValueError, match="mlp"):
        eng.explain(ids, latent=("trace", "mlp"))
    with pytest.raises(ValueError, match="graph"):
        eng.explain(ids, graph=True)
    with pytest.raises(NotImplementedError, match="explicit"):
        eng.set_mode("explicit")
    with pytest.raises(NotImplementedError, match="explicit"):
        Qwen3MoeLRP.from_hf(build_qwen3_moe("tiny"), dtype=torch.float32, mode="explicit")
    assert eng.mode == "efficient" and not eng.sparse_top


# ---- bf16: seed 3 of tests/golden/moe_engine_models.py (recorded there as SEED)
FUSED_B = 384          # 384 x 128 = 49152 rows: the smallest batch whose four attention-half GEMMs (N = 256 / 512) reach the fused kernels' 190 tiles


def test_planted_model_routing_survives_bf16():
    """CPU side of the seed choice: HF in fp32 and bf16; the fp32 routing margins (k-th to (k+1)-th, and 1st to 2nd for the slot order) are
    at least 10 x the largest |p_bf16 - p_fp32|"""
    assert mm.SEED == 3
    m23, m12, shift = mm.margin_and_bf16_shift()
    print(f"planted model: margins {m23:.4f} / {m12:.4f}, bf16 probability shift {shift:.4f}")
    assert min(m23, m12) >= 10 * shift


@functools.lru_cache(maxsize=None)
def planted():
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    model, ids = mm.build(), mm.inputs()
    ref = keep(Qwen3MoeLRP.from_hf(model, dtype=torch.float32, device="cuda", max_seq=mm.S).explain(ids, experts=True))
    eng = Qwen3MoeLRP.from_hf(model, dtype=torch.bfloat16, device="cuda", max_seq=mm.S)
    return model, ids, ref, eng


@functools.lru_cache(maxsize=None)
def dropin_errors():
    """the bf16 drop-in against the fp32 engine, in a process of its own (once for both tests below)"""
    model, ids, ref, eng = planted()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "fp32_engine.npz")
        np.savez(path, R_tok=ref["R_tok"].cpu().numpy(), R_expert=ref["R_expert"].cpu().numpy(), expert_index=ref["expert_index"].cpu().numpy())
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "qwen_moe_dropin_worker.py"), path], capture_output=True, text=True,
                           timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["idx"] == ref["idx"].tolist() and res["same_routing"]
    return res


def _bf16_against_dropin(out, ref, drop, tag):
    assert out["idx"].tolist() == ref["idx"].tolist()
    assert torch.equal(out["expert_index"], ref["expert_index"])
    for k in ("R_tok", "R_expert"):
        err, c = nmax(out[k], ref[k]), cos(out[k], ref[k])
        print(f"[{tag}] {k}: bf16 engine vs fp32 engine nmax {err:.3e} cos {c:.5f} | bf16 drop-in vs fp32 engine nmax {drop[k][0]:.3e} "
              f"cos {drop[k][1]:.5f}")
        assert err <= 2 * drop[k][0], (k, err, drop[k])


def test_bf16_engine_against_the_drop_in():
    """2 prompts of 128 tokens (256 rows: below the fused GEMM kernels' gate, every launch kernel by kernel)"""
    _need_gpu()
    model, ids, ref, eng = planted()
    drop = dropin_errors()
    assert not eng._attn_fused(ids.numel())
    _bf16_against_dropin(eng.explain(ids, experts=True), ref, drop, "B=2")


def test_bf16_engine_fused_attention_half():
    """the same two prompts at the head of a batch of 384: the attention half of every layer runs fused_qkv_fwd / fused_attn_fwd /
    fused_attn_bwd (asserted), and a prompt's result does not depend on its neighbours beyond what the other GEMM kernels round"""
    _need_gpu()
    model, ids, ref, eng = planted()
    drop = dropin_errors()
    more = torch.randint(0, 256, (FUSED_B - ids.shape[0], ids.shape[1]), generator=torch.Generator().manual_seed(11))
    batch = torch.cat([ids, more])
    assert eng._attn_fused(batch.numel())
    out = eng.explain(batch, experts=True)
    assert bool(torch.isfinite(out["R_tok"]).all()) and bool(torch.isfinite(out["R_expert"]).all())
    head = dict(idx=out["idx"][:2], expert_index=out["expert_index"][:, :2], R_tok=out["R_tok"][:2], R_expert=out["R_expert"][:, :2])
    _bf16_against_dropin(head, ref, drop, f"B={FUSED_B}, fused attention half")
