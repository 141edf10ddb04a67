"""GPU: dense Qwen2 / Qwen3 on the fused decoder layer -- the QwenLRP driver (fp32 parity, bf16, ragged batches, graph replay) and the drop-in
path -- against the real reference's relevance on seeded models the fused path accepts (tests/golden/qwen_fused_*.npz)."""
import os
import subprocess
import sys

import pytest
import torch

from tests.golden import qwen_models as qm
from tests.util import load, t, nmax

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CASES = list(qm.CASES)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _worker(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "qwen_fused_worker.py"), *args], capture_output=True, text=True, timeout=900,
                       cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("case", CASES)
def test_qwen_lrp_fp32_matches_the_reference(case):
    """QwenLRP in fp32 (the per-kernel path: bias through the Linear kernel, head norms through head_rmsnorm_fwd / _bwd): the reference's idx
    on every prompt, R_tok within 1e-4 of the reference's fp64 run (the project's fp32 bar, BASELINE.json), per-layer sums of relevance too"""
    _need_gpu()
    import lxt_amd.engine_qwen as Q
    fx = load(f"qwen_fused_{case}.npz")
    model = qm.build(case)
    assert abs(qm.wsum(model) - float(fx["wsum"])) < 1e-6 * float(fx["wsum"]), "weights did not reproduce"
    eng = Q.QwenLRP.from_hf(model, dtype=torch.float32, max_seq=qm.S)
    assert (eng.lm_head.data_ptr() == eng.embed.data_ptr()) == qm.CASES[case]["tie"]          # tied: one stored copy
    ids, R64, lR = t(fx["ids"]).long(), t(fx["R_tok_fp64"]), t(fx["layer_R"])
    errs, lerrs = [], []
    for b0 in range(0, qm.B, 8):
        out = eng.explain(ids[b0: b0 + 8], layer_relevance=True)
        assert out["idx"].cpu().long().tolist() == fx["idx"][b0: b0 + 8].tolist()
        errs += [nmax(out["R_tok"][b], R64[b0 + b]) for b in range(8)]
        lerrs.append(nmax(out["layer_R"], lR[:, b0: b0 + 8]))
    print(f"[{case} QwenLRP fp32 vs reference fp64] max nmax {max(errs):.2e}; layer sums {max(lerrs):.2e}")
    assert max(errs) <= 1e-4 and max(lerrs) <= 1e-4


@pytest.mark.parametrize("case", CASES)
def test_dropin_fused_qwen_layer_matches_the_reference_like_the_per_module_dropin(case):
    """bf16 model under lxt_amd.efficient.monkey_patch, FUSE_LAYER off (the per-module patches: the yardstick) and on (every layer's
    _lrp_fused_layer["ok_rows"][(B, S)] true), both against the reference's fp64 R_tok: cosine > 0.999 and
    max(e_fused) < max(2e-2, 1.5 max(e_per_module)) -- the bar of test_hf_gpu.py's Llama test with the reference in place of the fp32 drop-in"""
    _need_gpu()
    _worker(case)


@pytest.mark.parametrize("case", CASES)
def test_qwen_lrp_bf16_matches_the_reference_like_the_per_module_dropin(case):
    """QwenLRP in bf16 on the fused layer: the fixture's idx, and the bar above with the per-module drop-in's error as yardstick; its distance
    to the fused drop-in run (the same launch sequence on the same folded weights) is printed, not gated"""
    _need_gpu()
    _worker(case, "engine")


def test_qwen3_left_padded_lengths_and_graph_replay():
    """lengths (left-padded) on a Qwen3 model: each padded prompt equals its un-padded single-prompt explanation to the Llama ragged test's
    tolerance (fp32, efficient placement: 1e-4); graph=True on the bf16 engine at the fused row count replays the eager result bit for bit"""
    _need_gpu()
    import lxt_amd.engine_qwen as Q
    case = "qwen3_d128"
    fx = load(f"qwen_fused_{case}.npz")
    ids = t(fx["ids"]).long()
    eng = Q.QwenLRP.from_hf(qm.build(case), dtype=torch.float32, max_seq=qm.S)
    S, lens = 256, [256, 157, 33]
    batch = ids[:3, :S].clone()
    out = eng.explain(batch, lengths=lens)
    for b, n in enumerate(lens):
        one = eng.explain(batch[b: b + 1, S - n:], target=out["idx"][b: b + 1])
        err = nmax(out["R_tok"][b, S - n:], one["R_tok"][0])
        print(f"[qwen3 lengths] prompt {b} (len {n}): padded vs un-padded {err:.2e}")
        assert err < 1e-4 and float(out["R_tok"][b, : S - n].abs().sum()) == 0.0
    del eng
    eng = Q.QwenLRP.from_hf(qm.to_bf16_rotary_fp32(qm.build(case)), max_seq=qm.S)
    assert eng._fused(qm.B * qm.S).full
    eager = {k: v.clone() for k, v in eng.explain(ids).items()}
    g1 = {k: v.clone() for k, v in eng.explain(ids, graph=True).items()}
    g2 = eng.explain(ids, graph=True)
    for g in (g1, g2):
        assert torch.equal(g["R_tok"], eager["R_tok"]) and torch.equal(g["idx"], eager["idx"]) and torch.equal(g["logits"], eager["logits"])
