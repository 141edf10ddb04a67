#!/usr/bin/env python3
"""CP-LRP on the MI355X, at the Llama-3-8B shape, bf16, S = 2048, B in {4, 1}:
  1. lrp_attn_bwd_dv against the pair it replaces on the same operands -- lrp_attn_bwd_dkv (fed Gho = G) + lrp_gqa_reduce of dv_h (the dK
     reduce, which the AttnLRP backward also runs, is NOT counted): microseconds from device events, median (min) of --reps calls after
     warm-up, the two alternated call by call; and the normalised max difference of the two results.
  2. LlamaLRP.explain() under rule="attnlrp" and rule="cp" on one engine (synthetic weights, --layers layers), milliseconds per call, device
     events, median (min) of --reps, the two rules alternated block by block.
usage: python tools/cp_bench.py [--out FILE] [--reps 20] [--layers 8] [--no-engine]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


def timed(fns, reps, warm=3):
    """median and min microseconds of each fn over reps calls between device events, the fns alternated call by call"""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b) * 1e3)
    return [(statistics.median(t), min(t)) for t in ts]


def kernel_part(ops, say, reps):
    Hq, Hkv, d, S, dt = 32, 8, 128, 2048, torch.bfloat16
    scale, rep = d ** -0.5, Hq // Hkv
    say(f"lrp_attn_bwd_dv vs lrp_attn_bwd_dkv + lrp_gqa_reduce(dv_h), Hq {Hq} / Hkv {Hkv} heads of {d}, bf16, S {S}, causal; "
        f"us = median (min) of {reps} device-event times, alternated")
    g = torch.Generator(device="cuda").manual_seed(0)
    for B in (4, 1):
        M = B * S
        q, G = (torch.randn(M, Hq * d, generator=g, device="cuda").to(dt) for _ in range(2))
        k, v = (torch.randn(M, Hkv * d, generator=g, device="cuda").to(dt) for _ in range(2))
        o, lse = torch.empty_like(q), torch.empty(B, Hq, S, device="cuda")
        ops.attn_fwd(q, k, v, None, o, lse, B, S, Hq, Hkv, d, scale, True, 0)
        D = torch.zeros(B, Hq, S, device="cuda")
        dv, red = torch.empty_like(k), torch.empty_like(k)
        dk_h, dv_h = torch.empty_like(q), torch.empty_like(q)

        def new():
            ops.attn_bwd_dv(q, k, G, lse, dv, B, S, Hq, Hkv, d, scale)

        def old():
            ops.attn_bwd_dkv(q, k, v, None, G, None, lse, D, dk_h, dv_h, B, S, Hq, Hkv, d, scale, 0.0, 0.0)
            ops.gqa_reduce(dv_h, red, M, Hkv, rep, d)

        (nm, nb), (om, ob) = timed((new, old), reps)
        err = float((dv.float() - red.float()).abs().max() / red.float().abs().max())
        # causal: S^T = Q K^T and dV^T = G^T P^T over half the (query, key) pairs, 2 S^2 / 2 d flops each per query head
        fl = 2 * (2.0 * S * S / 2 * d) * B * Hq
        say(f"  B {B}: attn_bwd_dv {nm:8.1f} us ({nb:8.1f})  {fl / nm / 1e6:6.1f} TFLOP/s of its two contractions   dkv + gqa_reduce {om:8.1f} us "
            f"({ob:8.1f})   ratio {om / nm:5.2f} x   [dv vs reduce(dv_h), max-normalised {err:.1e}]")


def engine_part(say, reps, layers):
    import bench
    import lxt_amd.engine as E
    cfg = dict(bench.LLAMA3_8B, n_layers=layers)
    S = 2048
    W = bench.synth_weights(cfg, "cuda", torch.bfloat16, seed=0)
    eng = E.LlamaLRP(cfg, W, dtype=torch.bfloat16, mode="efficient", max_seq=S)
    say(f"LlamaLRP.explain(), Llama-3-8B widths, {layers} layers, bf16, S {S}; ms = median (min) of {reps} device-event times per rule, the "
        f"rules alternated in blocks of {reps}")
    for B in (4, 1):
        ids = torch.randint(0, cfg["vocab"], (B, S), generator=torch.Generator().manual_seed(B))
        res = {}
        for rnd in range(2):
            for rule in ("attnlrp", "cp"):
                eng.set_rule(rule)
                res.setdefault(rule, []).append(timed((lambda: eng.explain(ids),), reps, warm=2)[0])
        eng.set_rule("attnlrp")
        line = "   ".join(f"{rule} " + " / ".join(f"{m / 1e3:8.2f} ms ({b / 1e3:8.2f})" for m, b in res[rule]) for rule in ("attnlrp", "cp"))
        say(f"  B {B}: {line}   cp / attnlrp {res['cp'][-1][0] / res['attnlrp'][-1][0]:5.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--no-engine", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cp_bench.py measures on a HIP device; none found")
    from lxt_amd import ops
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/cp_bench.py on {torch.cuda.get_device_name(0)}")
    kernel_part(ops, say, a.reps)
    if not a.no_engine:
        engine_part(say, a.reps, a.layers)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
