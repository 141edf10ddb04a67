#!/usr/bin/env python3
"""MXFP4 expert weights read inside the grouped expert GEMMs (csrc/moe_mxfp4.hip) at the Qwen3-30B-A3B layer: H 2048, I 768, 128 experts,
top-8, bf16.   python tools/moe_mxfp4_bench.py [--out profiles/moe_mxfp4_bench.txt] [--engine] [--parent-lib PATH]

  kernel level, T = 2048 and 8192, one process, the variants ALTERNATING inside every round (medians over the rounds, min ... max as spread):
    (i)   each of the four unquantised grouped GEMMs on the DEQUANTISED weights -- the control: same operand bits, same MFMA clocks;
    (ii)  each of the four _q GEMMs on the codes + scales -- the code under test;
    (iii) lrp_mxfp4_dequant of the layer's two tensors -- what a scratch scheme would add per pass.
    Criterion per GEMM and T: (ii) <= (i) + its tensor's share of (iii), with (i)'s own spread as the margin.
  --parent-lib: a liblrp_hip.so built from the parent commit; its four unquantised GEMMs alternate with this tree's in the same rounds
    (the default path against the parent).
  --engine: a randomly initialised Qwen3-30B-A3B-shaped model, S = 2048, 1 and 4 prompts; the engines weight_format=None, `deq` (an ordinary
    engine on the dequantised weights: the control) and "mxfp4" alternate; weight_bytes() and device memory of each."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import lxt_amd  # noqa: E402,F401
import lxt_amd._lib as L  # noqa: E402
import lxt_amd.ops as ops  # noqa: E402

H, I, E, K = 2048, 768, 128, 8
PEAK_FLOPS, PEAK_BW = 2.5e15, 8e12
ROUNDS, REPS = 9, 10
LINES = []
GEMMS = ("gate_up_fwd", "down_fwd", "down_dgrad", "gate_up_dgrad")


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, reps=REPS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us


def med(v):
    return statistics.median(v), min(v), max(v)


def parent_calls(path, x, G, m, coef, Agu, w, Wgu, Wd, plan):
    """the four unquantised entry points of ANOTHER build of the library (same ABI), on this process's tensors"""
    lib = ctypes.CDLL(path)
    for name in ("lrp_moe_gate_up_fwd", "lrp_moe_down_fwd", "lrp_moe_down_dgrad", "lrp_moe_gate_up_dgrad"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_int, getattr(L.lib, name).argtypes
    p, st, T, R = ops.p, ops.stream, plan.T, plan.rows
    o_coef, o_m, o_y = torch.empty_like(coef), torch.empty_like(m), torch.empty(R, H, device="cuda", dtype=x.dtype)
    o_A, o_part, o_gx = torch.empty_like(Agu), torch.empty(R, I // 128, device="cuda"), torch.empty(R, H, device="cuda", dtype=x.dtype)
    BF = L.BF16
    return {
        "gate_up_fwd": lambda: lib.lrp_moe_gate_up_fwd(p(x), p(Wgu), p(plan.buf), p(o_coef), p(o_m), T, K, E, H, I, H, 2 * I, I, L.ACT["silu"], BF, st()),
        "down_fwd": lambda: lib.lrp_moe_down_fwd(p(m), p(Wd), p(plan.buf), p(o_y), T, K, E, H, I, I, H, BF, st()),
        "down_dgrad": lambda: lib.lrp_moe_down_dgrad(p(G), p(Wd), p(coef), p(m), p(w), p(plan.buf), p(o_A), p(o_part), T, K, E, H, I, H, 2 * I, I,
                                                     2 * I, BF, st()),
        "gate_up_dgrad": lambda: lib.lrp_moe_gate_up_dgrad(p(Agu), p(Wgu), p(plan.buf), p(o_gx), T, K, E, H, I, 2 * I, H, BF, st()),
    }


def kernel_level(T, qgu, qd, Wgu, Wd, parent_lib=None):
    g = torch.Generator(device="cuda").manual_seed(T)
    x = torch.randn(T, H, device="cuda", generator=g, dtype=torch.bfloat16)
    idx = torch.rand(T, E, device="cuda", generator=g).argsort(1)[:, :K].contiguous()
    w = (torch.rand(T, K, device="cuda", generator=g) / K).to(torch.bfloat16)
    G = torch.randn(T, H, device="cuda", generator=g, dtype=torch.bfloat16)
    R = T * K
    plan = ops.MoePlan(idx, E)
    coef, m = ops.moe_gate_up_fwd(x, Wgu, plan)
    Agu, _ = ops.moe_down_dgrad(G, Wd, coef, m, w, plan)
    calls = {
        "gate_up_fwd": lambda W: ops.moe_gate_up_fwd(x, W, plan),
        "down_fwd": lambda W: ops.moe_down_fwd(m, W, plan),
        "down_dgrad": lambda W: ops.moe_down_dgrad(G, W, coef, m, w, plan),
        "gate_up_dgrad": lambda W: ops.moe_gate_up_dgrad(Agu, W, plan),
    }
    tensor = {"gate_up_fwd": (Wgu, qgu), "down_fwd": (Wd, qd), "down_dgrad": (Wd, qd), "gate_up_dgrad": (Wgu, qgu)}
    # the outputs are the same bits (the contract of the tests), checked here once on the benchmark's own operands
    for name in GEMMS:
        a, b = calls[name](tensor[name][0]), calls[name](tensor[name][1])
        for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert torch.equal(u, v), name
    sgu, sd = torch.empty_like(Wgu), torch.empty_like(Wd)
    deq = {"Wgu": lambda: qgu.dequant(torch.bfloat16, out=sgu), "Wd": lambda: qd.dequant(torch.bfloat16, out=sd)}
    par = parent_calls(parent_lib, x, G, m, coef, Agu, w, Wgu, Wd, plan) if parent_lib else {}
    t = {(n, v): [] for n in GEMMS for v in ("plain", "q", "parent")}
    td = {n: [] for n in deq}
    for fn in [lambda n=n, i=i: calls[n](tensor[n][i]) for n in GEMMS for i in (0, 1)] + list(deq.values()) + list(par.values()):
        timed(fn, 3)          # warm-up
    for _ in range(ROUNDS):
        for n in GEMMS:
            t[n, "plain"].append(timed(lambda: calls[n](tensor[n][0])))
            t[n, "q"].append(timed(lambda: calls[n](tensor[n][1])))
            if par:
                t[n, "parent"].append(timed(par[n]))
        for n, fn in deq.items():
            td[n].append(timed(fn))
    f = {"gate_up_fwd": 2.0 * R * 2 * I * H, "down_fwd": 2.0 * R * H * I, "down_dgrad": 2.0 * R * H * I, "gate_up_dgrad": 2.0 * R * 2 * I * H}
    nel = {"gate_up_fwd": E * 2 * I * H, "down_fwd": E * H * I, "down_dgrad": E * H * I, "gate_up_dgrad": E * 2 * I * H}
    say(f"\n== T = {T} tokens, {R} routed rows (~{R / E:.0f} per expert), bf16; {ROUNDS} rounds x {REPS} launches, median [min ... max] us")
    say(f"{'GEMM':14s} {'(i) plain on dequantised':>30s} {'(ii) _q':>30s} {'(ii)/(i)':>9s} {'(iii) share':>12s} {'(i)+(iii)':>10s} "
        f"{'PFLOP/s frac i|ii':>18s} {'8TB/s frac i|ii':>16s}  criterion")
    res = {}
    dq = {n: med(v) for n, v in td.items()}
    for n in GEMMS:
        (pm, plo, phi), (qm, qlo, qhi) = med(t[n, "plain"]), med(t[n, "q"])
        share = dq["Wgu" if "gate_up" in n else "Wd"][0]
        ok = qm <= pm + share + (phi - plo)
        ffr = [f[n] / (u * 1e-6) / PEAK_FLOPS for u in (pm, qm)]
        bfr = [nel[n] * 2 / (pm * 1e-6) / PEAK_BW, nel[n] * 17 / 32 / (qm * 1e-6) / PEAK_BW]
        say(f"{n:14s} {pm:9.1f} [{plo:8.1f} ... {phi:8.1f}] {qm:9.1f} [{qlo:8.1f} ... {qhi:8.1f}] {qm / pm:9.3f} {share:12.1f} {pm + share:10.1f} "
            f"{ffr[0]:8.3f} | {ffr[1]:6.3f} {bfr[0]:7.3f} | {bfr[1]:6.3f}  {'met' if ok else 'MISSED'}")
        res[n] = dict(plain_us=pm, plain_spread=(plo, phi), q_us=qm, q_spread=(qlo, qhi), ratio=qm / pm, dequant_share_us=share, met=ok)
        if par:
            am, alo, ahi = med(t[n, "parent"])
            inside = alo - (ahi - alo) <= pm <= ahi + (ahi - alo)
            say(f"{'':14s} parent build, same rounds: {am:9.1f} [{alo:8.1f} ... {ahi:8.1f}]; this tree / parent {pm / am:.3f} "
                f"({'inside' if inside else 'OUTSIDE'} the parent's spread)")
            res[n].update(parent_us=am, parent_spread=(alo, ahi))
    for n, (m_, lo, hi) in dq.items():
        nb = (E * 2 * I * H if n == "Wgu" else E * H * I) * (2 + 17 / 32)
        say(f"(iii) lrp_mxfp4_dequant {n}: {m_:9.1f} [{lo:8.1f} ... {hi:8.1f}] us = {nb / (m_ * 1e-6) / PEAK_BW:.3f} of 8 TB/s on bytes read + written")
    res["dequant_us"] = {n: v[0] for n, v in dq.items()}
    return res


def engine_level(prompts_list=(1, 4), S=2048):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from moe_bench import build_30b_a3b
    from lxt_amd.engine_qwen_moe import Qwen3MoeLRP
    gib = lambda: torch.cuda.memory_allocated() / 2 ** 30      # noqa: E731
    model = build_30b_a3b()
    base = gib()
    say(f"\n== engine level: random-init Qwen3-30B-A3B shape, bf16, S = {S}; the HF model itself holds {base:.1f} GiB on the device")
    engines = {}
    m0 = gib()
    engines["mxfp4"] = Qwen3MoeLRP.from_hf(model, max_seq=S, weight_format="mxfp4")
    m1 = gib()
    engines["None"] = Qwen3MoeLRP.from_hf(model, max_seq=S)          # (its experts ARE the model's tensors: no copy)
    m2 = gib()
    engines["deq"] = Qwen3MoeLRP(*engines["mxfp4"].dequantized_weights(), max_seq=S)
    m3 = gib()
    held = {"mxfp4": m1 - m0, "None": (m2 - m1) + engines["None"].weight_bytes()["experts"] / 2 ** 30, "deq": m3 - m2}
    for name, eng in engines.items():
        wb = eng.weight_bytes()
        say(f"{name:6s} weight_bytes: resident {wb['resident'] / 1e9:7.2f} GB, experts {wb['experts'] / 1e9:7.2f} GB, scratch {wb['scratch']}; "
            f"device memory the engine holds {held[name]:6.1f} GiB")
    res = dict(weight_bytes={n: e.weight_bytes() for n, e in engines.items()}, held_gib=held)
    for B in prompts_list:
        ids = torch.randint(0, model.config.vocab_size, (B, S), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B))
        outs = {n: e.explain(ids) for n, e in engines.items()}
        assert torch.equal(outs["mxfp4"]["R_tok"], outs["deq"]["R_tok"]), "quantised engine != engine on the dequantised weights"
        ts = {n: [] for n in engines}
        for _ in range(5):
            for n, e in engines.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.explain(ids)
                torch.cuda.synchronize()
                ts[n].append((time.perf_counter() - t0) * 1e3)
        for n in engines:
            m_, lo, hi = med(ts[n])
            say(f"{B} prompt(s) {n:6s}: {m_:7.1f} [{lo:7.1f} ... {hi:7.1f}] ms per explain -> {B / m_ * 1e3:.2f} expl/s")
        res[f"B{B}"] = {n: med(v)[0] for n, v in ts.items()}
        say(f"{B} prompt(s): mxfp4 / deq = {res[f'B{B}']['mxfp4'] / res[f'B{B}']['deq']:.3f}, mxfp4 / None = {res[f'B{B}']['mxfp4'] / res[f'B{B}']['None']:.3f}; "
            f"R_tok of mxfp4 and deq: bit-identical")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--engine", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    say(f"device: {torch.cuda.get_device_name(0)}; layer H {H}, I {I}, {E} experts, top-{K}")
    g = torch.Generator(device="cuda").manual_seed(1)
    qgu = ops.MoeQuantWeight((torch.randn(E, 2 * I, H, device="cuda", generator=g) * H ** -0.5).to(torch.bfloat16))
    qd = ops.MoeQuantWeight((torch.randn(E, H, I, device="cuda", generator=g) * I ** -0.5).to(torch.bfloat16))
    Wgu, Wd = qgu.dequant(torch.bfloat16), qd.dequant(torch.bfloat16)
    say(f"layer weights: bf16 {(Wgu.numel() + Wd.numel()) * 2 / 1e9:.3f} GB, MXFP4 {(qgu.nbytes() + qd.nbytes()) / 1e9:.3f} GB per direction")
    result = dict(kernels={T: kernel_level(T, qgu, qd, Wgu, Wd, a.parent_lib) for T in (2048, 8192)})
    del qgu, qd, Wgu, Wd
    torch.cuda.empty_cache()
    if a.engine:
        result["engine"] = engine_level()
    say("JSON " + json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
