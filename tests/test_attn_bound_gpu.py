"""The bf16 attention kernels against the element-wise rounding bound of tests/attn_bound.py: forward, attn_bwd_prep, dQ, dK / dV, the two
gqa_reduce and -- where they are served -- the D-forming dQ kernel and the dV-only kernel of CP-LRP, at every head dim, two GQA ratios, sequence
lengths one row past a 32-, 128- and 256-row block plus a ragged tail, and every mask family (causal, full, window below / one past the block
size, row intervals, q_begin).  Operands as tests/test_kernel_edges_gpu.py passes them: column slices of one fused buffer, NaN-filled over-wide
outputs.  Every output goes through attn_bound.check: finite, |x - fp64 reference| <= bound on EVERY element, exact zeros where nothing is
summed.  The signed-bias statistic (round-to-nearest, not truncation) runs on the cases tests/test_attn_bound_cpu.py admits, against the bar
computed from the truncating model of tests/attn_bound.py on the same case.

Which operands feed the reference: the kernels' own Gho, D, o and lse wherever the kernel under test consumes them; P is the normalised
softmax (not exp(s - the kernel's lse): that would take the forward's error out of the dq / dk / dv checks) except for the CP dv, whose
header defines P on the lse it is handed."""
import pytest
import torch

from tests import attn_bound as ab
from tests.test_kernel_edges_gpu import _attn_pipeline, _nan_buf, _qkv_slices, _spares_untouched, ops  # noqa: F401  (ops: the fixture)
from tests.test_kernels_gpu import _intervals, rnd

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _call(ops, Bn, S, Hq, Hkv, d, mask, log, bias_log=None):      # noqa: F811
    """one pipeline call on one case -> its outputs through attn_bound.evaluate (asserting); the bias statistic where the case is admitted"""
    name, causal, window, kind, q_begin = mask
    scale = d ** -0.5
    views, (q4, k4, v4) = _qkv_slices(Bn, S, Hq, Hkv, d, BF)
    q, k, v = views
    Go = rnd(Bn * S, Hq * d, dtype=BF, seed=4)
    Go.view(Bn, S, Hq * d)[:, :q_begin] = 0
    row_iv = None
    if kind is not None:
        lo, hi, causal = _intervals(kind, Bn, S)
        row_iv = (lo.cuda().contiguous(), hi.cuda().contiguous())
    vis = ab.visible(Bn, S, causal, window, row_iv, device="cuda")
    print(f"[d {d} heads {Hq}/{Hkv} B {Bn} S {S} {name}]")
    R = _attn_pipeline(ops, views, Bn, S, Hq, Hkv, d, BF, causal, window, Go, row_iv=row_iv)                  # dense: q_begin = 0
    _spares_untouched(R)
    fwd, bwd = R, R
    if q_begin:
        # as tests/test_kernel_edges_gpu.py::test_attention_q_begin: the sparse forward on its own; the backward with q_begin on a seed that is
        # zero below q_begin, fed the dense forward's o / lse
        fwd = _attn_pipeline(ops, views, Bn, S, Hq, Hkv, d, BF, causal, window, None, q_begin=q_begin, row_iv=row_iv)
        bwd = _attn_pipeline(ops, views, Bn, S, Hq, Hkv, d, BF, causal, window, Go, q_begin=q_begin, row_iv=row_iv, fwd_from=(R["o"], R["lse"]))
        _spares_untouched(fwd)
        _spares_untouched(bwd)
    out = dict(o=ab.h4(fwd["o"], Bn, S, Hq, d), lse=fwd["lse"].double(), o_bwd=ab.h4(R["o"], Bn, S, Hq, d), lse_bwd=R["lse"].double(),
               Gho=ab.h4(bwd["Gho"], Bn, S, Hq, d), D=bwd["D"].double(), dq=ab.h4(bwd["dq"], Bn, S, Hq, d),
               dk_h=ab.h4(bwd["dk_h"], Bn, S, Hq, d), dv_h=ab.h4(bwd["dv_h"], Bn, S, Hq, d),
               dk=ab.h4(bwd["dk"], Bn, S, Hkv, d), dv=ab.h4(bwd["dv"], Bn, S, Hkv, d))
    if "dq2" in bwd:
        out["D2"], out["dq2"] = bwd["D2"].double(), ab.h4(bwd["dq2"], Bn, S, Hq, d)
    cp = ops.attn_bwd_dv_ok(BF, d) and causal and not window
    if cp:
        G = bwd["Gho"]
        G_t = ops.transpose_heads(G, Bn, S, Hq, d) if ops.attn_needs_transposed(q, d) else None
        dv, spare = _nan_buf(Bn * S, Hkv * d, 8, BF)
        ops.attn_bwd_dv(q, k, G, R["lse"], dv, Bn, S, Hq, Hkv, d, scale, q_begin=q_begin, row_iv=row_iv, G_t=G_t)
        assert torch.isnan(spare).all(), "attn_bwd_dv wrote past its row width"
        out["cp_dv"] = ab.h4(dv, Bn, S, Hkv, d)
    q64, k64, v64 = q4.double(), k4.double(), v4.double()
    ab.evaluate(out, q64, k64, v64, vis, scale, q_begin=q_begin, log=log)
    if bias_log is not None and ab.bias_case(S, mask):
        got = ab.biases(out, q64, k64, v64, vis, scale)
        Go4 = Go.float().reshape(Bn, S, Hq, d).permute(0, 2, 1, 3)
        bars = {n: 0.5 * abs(b) for n, b in ab.biases(ab.model(q4.float(), k4.float(), v4.float(), Go4, vis, scale, rnd=ab.trunc, cp=cp),
                                                   q64, k64, v64, vis, scale).items()}
        print("  bias / bar, in u: " + " ".join(f"{n} {got[n]:+.3f} / {bars[n]:.3f}" for n in got))
        for n, b in got.items():
            bias_log[n] = max(bias_log.get(n, 0.0), abs(b))
            assert abs(b) <= bars[n], (n, b, bars[n])


@pytest.mark.parametrize("Hq,Hkv", ab.HEADS)
@pytest.mark.parametrize("d", ab.D_ALL)
def test_attention_within_rounding_bound(ops, d, Hq, Hkv):      # noqa: F811
    log, bias_log = {}, {}
    for S in ab.S_ALL:
        for mask in ab.masks(S):
            _call(ops, ab.B, S, Hq, Hkv, d, mask, log, bias_log)
    print(f"kernels d {d} heads {Hq}/{Hkv}: worst err / bound per output: " + " ".join(f"{n} {r:.3f}" for n, r in log.items()))
    print(f"kernels d {d} heads {Hq}/{Hkv}: largest |bias| per output, in u: " + " ".join(f"{n} {b:.3f}" for n, b in bias_log.items()))


def test_forward_256_query_workgroups_within_bound(ops):      # noqa: F811
    """B Hq ceil(S / 256) >= 512 at d = 32: the 8-wave forward's 256-query workgroups (two 16-row sub-tiles per wave), the shape of
    tests/test_kernels_gpu.py::test_attention; the backward kernels have one form at d = 32 and run along"""
    log = {}
    _call(ops, 4, 130, 128, 32, 32, ("causal", True, 0, None, 0), log)
    print("kernels d 32 heads 128/32 (256-query forward workgroups): worst err / bound per output: " + " ".join(f"{n} {r:.3f}" for n, r in log.items()))


@pytest.mark.parametrize("d", [64, 128])
def test_cp_dv_256_key_workgroups_within_bound(ops, d):      # noqa: F811
    """the dV-only kernel's 256-key (8-wave) workgroups: 4 prompts x 128 kv heads x 2 key blocks = 1024 workgroups, the grid of
    tests/test_cp_kernels_gpu.py::test_attn_bwd_dv_both_workgroup_sizes; prompt 0 against the bound (with the forward that made its lse)"""
    Bn, S, H = 4, 257, 128
    scale = d ** -0.5
    views, (q4, k4, v4) = _qkv_slices(Bn, S, H, H, d, BF)
    q, k, v = views
    G = rnd(Bn * S, H * d, dtype=BF, seed=4)
    o, lse = torch.full((Bn * S, H * d), float("nan"), dtype=BF, device="cuda"), torch.full((Bn, H, S), float("nan"), device="cuda")
    ops.attn_fwd(q, k, v, None, o, lse, Bn, S, H, H, d, scale, True, 0)
    dv, spare = _nan_buf(Bn * S, H * d, 8, BF)
    ops.attn_bwd_dv(q, k, G, lse, dv, Bn, S, H, H, d, scale)
    assert torch.isnan(spare).all() and torch.isfinite(dv.float()).all()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"[CP dv d {d}: {Bn * H * 2} workgroups of 256 keys on {cus} CUs (8-wave form from {4 * cus})]")
    one = lambda x: x[:1].double()      # noqa: E731
    vis = ab.visible(1, S, True, 0, device="cuda")
    R = ab.forward_ref(one(q4), one(k4), one(v4), vis, scale)
    log = {}
    ab.check("o", ab.h4(o, Bn, S, H, d)[:1], R["o"], ab.bound_o(R), log=log)
    ab.check("lse", lse[:1].double(), R["lse"], ab.bound_lse(R), log=log)
    ref, bound = ab.cp_dv_ref(R, one(q4), one(k4), ab.h4(G, Bn, S, H, d)[:1], lse[:1].double(), vis)
    ab.check("cp_dv", ab.h4(dv, Bn, S, H, d)[:1], ref, bound, log=log)
    print(f"kernels d {d} heads 128/128 (256-key CP workgroups): worst err / bound per output: " + " ".join(f"{n} {r:.3f}" for n, r in log.items()))
