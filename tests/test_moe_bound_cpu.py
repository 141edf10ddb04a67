"""No GPU: the element-wise bounds of tests/moe_bound.py for the routed-expert kernels.
  (a) soundness: a faithful torch model of the kernels' arithmetic (fp32 maths, a round trip through bf16 exactly where the kernels convert) is
      within every bound on every element of every case, in bf16 and in the fp32 form, with both activations on `edges`; the exact zeros and
      the cap on the share of cg left out are asserted;
  (b) discrimination: each planted fault leaves the bound on at least one element of every output it touches; next to it, whether the bars
      tests/test_moe_gpu.py holds the chain to (nmax 2e-2 / cos 0.999 in bf16, nmax 1e-5 in fp32) would have let it through -- at least one
      structural fault planted on a 2^-6-scaled row does pass them (asserted: the reason these tests exist);
  (c) the cases are what their table says, and the Lipschitz constants of the docstring hold on a grid."""
import pytest
import torch

from tests import moe_bound as mb

BF16, F32 = torch.bfloat16, torch.float32


def test_lipschitz_constants():
    g = torch.linspace(-40.0, 40.0, 800001, dtype=torch.float64)
    sig = torch.sigmoid
    for act in mb.ACTS:
        if act == "silu":
            S, dS = sig(g), sig(g) * (1 - sig(g))
        else:
            z2 = 2 * mb.K0 * (g + mb.K1 * g ** 3)
            S, dS = sig(z2), sig(z2) * (1 - sig(z2)) * 2 * mb.K0 * (1 + 3 * mb.K1 * g ** 2)
        assert float((S * g - mb.act64(g, act)).abs().max()) <= 1e-12                      # act = g S
        d_act, d_s = float((S + g * dS).abs().max()), float(dS.abs().max())
        print(f"{act}: sup |act'| = {d_act:.5f} (L_ACT {mb.L_ACT[act]}), sup |S'| = {d_s:.5f} (L_S {mb.L_S[act]})")
        assert 0.98 * mb.L_ACT[act] <= d_act <= mb.L_ACT[act] and 0.98 * mb.L_S[act] <= d_s <= mb.L_S[act]
    z = torch.linspace(-20.0, 20.0, 400001, dtype=torch.float64)
    assert float((z.abs() / torch.cosh(z) ** 2).max()) <= 0.448


def test_cases_are_what_the_table_says():
    for name, c in mb.CASES.items():
        idx, P = mb.routing(name), mb.plan_of(name)
        assert tuple(idx.shape) == (c["T"], c["k"]) and c["H"] % 128 == 0 and c["I"] % 128 == 0
        live = (idx >= 0) & (idx < c["E"])
        assert int((~live).sum()) == c["skips"]
        if c["counts"] is not None:
            assert P.cnt.tolist() == c["counts"]
        for t in range(c["T"]):                                  # a token never meets an expert twice
            e = idx[t][live[t]].tolist()
            assert len(set(e)) == len(e)
        d = mb.inputs(name, BF16)
        for key in ("m_in", "coef_in", "Agu_in", "rows_in"):
            assert bool(torch.isnan(d[key][P.n:]).all()) and bool(torch.isfinite(d[key][:P.n]).all()), key
        for key in ("x", "G"):
            assert bool(torch.isnan(d[key][~P.live_tok]).all()) and bool(torch.isfinite(d[key][P.live_tok]).all()), key
    P = mb.plan_of("seams")
    assert int((~P.live_tok).sum()) == 1 and {int(i) for i in mb.routing("seams")[~P.live_tok].flatten()} <= {-1, 6, 9}
    assert int(mb.plan_of("none").n) == 0 and int(mb.plan_of("fanout").cnt.max()) <= 8 and float((mb.plan_of("fanout").cnt <= 3).double().mean()) > 0.5
    # tile counts of the table: N / 128 per op
    ce, cs, cw = mb.CASES["edges"], mb.CASES["seams"], mb.CASES["wrap"]
    assert ce["I"] // 128 == 3 and 2 * ce["I"] // 128 == 6 and cs["H"] // 128 == 1
    assert int(mb.plan_of("wrap").toff[-1]) * (2 * cw["I"] // 128) == 1280 and int(mb.plan_of("wrap").toff[-1]) * (cw["I"] // 128) == 640
    # the planted rows of `edges` and their 2^-6 tokens
    d, P, pl = mb.inputs("edges", BF16), mb.plan_of("edges"), mb.planted("edges")
    assert int(P.expert[pl["p_last"]]) == 2 and int(P.expert[pl["p_last"] - 1]) == 2 and pl["p_last"] + 1 == int(P.off[3])
    assert int(P.expert[pl["p_second"]]) == 4 and pl["p_second"] - int(P.off[4]) == 128 and int(P.cnt[pl["e_prev"]]) > 0
    for t in d["small"]:
        assert float(d["x"][t].float().abs().max()) < 2.0 ** -6 * 6 and float(d["x"][t].float().abs().max()) > 0
    assert d["zero_tok"] not in d["small"] and not bool(d["x"][d["zero_tok"]].any()) and not bool(d["Wgu"][d["e0"], d["j0"]].any())
    assert int(P.cnt[d["e0"]]) == 129


@pytest.mark.parametrize("name,dtype,act", mb.RUNS, ids=mb.RUN_IDS)
def test_model_is_within_every_bound(name, dtype, act):
    d = mb.inputs(name, dtype)
    print(f"[{name} {dtype} {act}] the faithful model against its bounds")
    log = mb.evaluate(d, act, mb.model_ops(d, act))
    print(f"model {name} {dtype} {act}: worst err / bound per output: " + " ".join(f"{n} {r:.3f}" for n, r in log.items()))
    assert set(log) == {"m", "cg", "cu", "y", "Agu", "gw", "gx_rows", "out_w", "out_1"}
    if name == "none":
        out = mb.model_ops(d, act)
        assert not bool(out["gw"].any()) and not bool(out["out_w"].any()) and not bool(out["out_1"].any())


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_planted_faults_leave_the_bound(dtype):
    d, act = mb.inputs("edges", dtype), "silu"
    ref = mb.chain_ref(d, act)
    clean = mb.model_chain(d, act)
    for n in ref:
        assert mb.todays_bars(clean[n], ref[n], dtype)[0], n
    passed_today = []
    print(f"[edges {dtype}] fault: err / bound per touched output | today's bars on the chain (nmax, cos per touched chain output)")
    for fault, touched in mb.FAULTS.items():
        if fault == "trunc" and dtype != BF16:
            continue
        out = mb.model_ops(d, act, fault=fault)
        ratios = {n: mb.evaluate(d, act, out, strict=False, only=(n,))[n] for n in touched}
        chain = mb.model_chain(d, act, fault=fault)
        bars = {n: mb.todays_bars(chain[n], ref[n], dtype) for n in mb.CHAIN_TOUCH[fault]}
        through = all(b[0] for b in bars.values())
        print(f"  {fault:14s} " + " ".join(f"{n} {r:.3g}" for n, r in ratios.items()) + " | "
              + " ".join(f"{n} {b[1]:.2e} {b[2]:.6f}" for n, b in bars.items()) + f" | today's bars: {'PASS (missed)' if through else 'caught'}")
        for n, r in ratios.items():
            assert r > 1.0, (fault, n, r)
        if through and fault in ("last_row", "prev_weight"):          # the faults planted on a 2^-6-scaled row
            passed_today.append(fault)
    if dtype == BF16:
        assert passed_today, "no structural fault on a 2^-6-scaled row passes today's bars: the premise of these tests is gone"
