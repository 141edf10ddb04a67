#!/usr/bin/env python3
"""Answer-span attribution on the MI355X: what lrp_span_seed and explain(positions=...) cost.
  1. lrp_span_seed at V = 128256, R in {4, 256, 2048} rows, both objectives (the log-probability's dense seed in bf16): microseconds from
     device events (median of --reps timed calls after warm-up), the bytes the kernel has to move (the fp32 row once from HBM, the seed once
     to it; the second and third pass over a row are L2 hits and are not counted) per second as a fraction of 8 TB/s, and beside it the torch
     composition a caller would otherwise write (log_softmax + gather; softmax, one-hot, scale, cast).
  2. explain(positions=...) on LlamaLRP at the Llama-3-8B shape (32 layers, bf16, random init), B = 1, S = 2048, T in {1, 64, 256} positions,
     both objectives, against the plain last-position call of the same engine (the default path is the parent commit's, bitwise:
     profiles/span_default_path_ab.txt) and against T of them -- what T single-position explanations cost without the keyword;
     per_position=True at T = 64 against 64 plain calls; the dense top layer against the sparse one (the plain call with sparse_top off).
     Wall-clock milliseconds of whole synchronised calls (the request's checks synchronise with the host), median of --calls.
usage: python tools/span_bench.py [--out FILE] [--reps 20] [--calls 10] [--layers 32]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

V8B = 128256
HBM = 8.0e12


def timed(fn, reps):
    """median microseconds of fn() over reps calls, each between two device events"""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts)


def wall(fn, calls):
    """median milliseconds of whole calls of fn(), device idle before and after each"""
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def kernel_part(ops, say, reps):
    say(f"lrp_span_seed, V = {V8B}, fp32 logits; us = median (min) of device-event times; bytes = 4 R V read (+ 2 R V bf16 seed written)")
    g = torch.Generator(device="cuda").manual_seed(0)
    for R in (4, 256, 2048):
        logits = torch.randn(R, V8B, generator=g, device="cuda") * 4.0
        idx = torch.randint(0, V8B, (R,), generator=g, device="cuda", dtype=torch.int32)
        w, rstd = torch.rand(R, generator=g, device="cuda"), torch.rand(R, generator=g, device="cuda") + 0.5
        seed = torch.empty(R, V8B, device="cuda", dtype=torch.bfloat16)
        outs = [torch.empty(R, device="cuda") for _ in range(3)]
        il = idx.long()[:, None]

        def k_logit():
            ops.span_seed(logits, idx, w, rstd, "logit", logit=outs[0], logprob=outs[1], rs=outs[2])

        def k_logprob():
            ops.span_seed(logits, idx, w, rstd, "logprob", seed=seed, logit=outs[0], logprob=outs[1], rs=outs[2])

        def t_logit():
            torch.log_softmax(logits, -1).gather(1, il)
            logits.gather(1, il)
            torch.mul(w, rstd)

        def t_logprob():
            t_logit()
            p = torch.softmax(logits, -1).neg_()
            p.scatter_add_(1, il, torch.ones_like(il, dtype=p.dtype))
            seed.copy_(p.mul_(w[:, None]))

        for tag, kern, comp, nbytes in (("logit", k_logit, t_logit, 4.0 * R * V8B), ("logprob", k_logprob, t_logprob, 6.0 * R * V8B)):
            for fn in (kern, comp):
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            (km, kb), (cm, cb) = timed(kern, reps), timed(comp, reps)
            say(f"  R {R:5d} {tag:8s}: kernel {km:9.1f} us ({kb:9.1f})  {nbytes / km / 1e6:7.3f} TB/s = {nbytes / (km * 1e-6) / HBM:5.3f} of 8 TB/s"
                f"   torch composition {cm:9.1f} us ({cb:9.1f})")
        del logits, seed


def engine_part(say, calls, layers):
    import bench
    import lxt_amd.engine as E
    cfg = dict(bench.LLAMA3_8B, n_layers=layers)
    B, S = 1, 2048
    eng = E.LlamaLRP(cfg, bench.synth_weights(cfg, "cuda", torch.bfloat16, seed=0), dtype=torch.bfloat16, mode="efficient", max_seq=S)
    ids = torch.randint(0, cfg["vocab"], (B, S), generator=torch.Generator().manual_seed(1)).cuda()
    say(f"LlamaLRP, Llama-3-8B shape, {layers} layers, bf16, B = {B}, S = {S}; ms = median wall time of {calls} synchronised calls")
    for _ in range(2):
        eng.explain(ids)
    plain = wall(lambda: eng.explain(ids), calls)
    eng.sparse_top = False
    for _ in range(2):
        eng.explain(ids)
    dense = wall(lambda: eng.explain(ids), calls)
    eng.sparse_top = True
    say(f"  plain last-position call: {plain:8.2f} ms; with a dense top layer (sparse_top off): {dense:8.2f} ms  (+{dense - plain:.2f} ms)")
    for T in (1, 64, 256):
        pos = torch.randperm(S - 1, generator=torch.Generator().manual_seed(T))[:T].sort().values[None]
        for objective in ("logit", "logprob"):
            run = lambda: eng.explain(ids, positions=pos, objective=objective)          # noqa: E731
            for _ in range(2):
                run()
            ms = wall(run, calls)
            say(f"  T {T:4d} {objective:8s}: one span call {ms:8.2f} ms = {ms / plain:5.2f} x the plain call; T plain calls {T * plain:10.1f} ms "
                f"({T * plain / ms:6.1f} x the span call)")
    T = 64
    pos = torch.randperm(S - 1, generator=torch.Generator().manual_seed(T))[:T].sort().values[None]
    run = lambda: eng.explain(ids, positions=pos, per_position=True)                     # noqa: E731
    run()
    ms = wall(run, max(3, calls // 3))
    say(f"  T {T:4d} per_position=True (one forward, {T} backward passes): {ms:9.1f} ms; {T} plain calls {T * plain:9.1f} ms ({T * plain / ms:4.2f} x)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--layers", type=int, default=32)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("span_bench needs a HIP device")
    from lxt_amd import ops
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    kernel_part(ops, say, a.reps)
    engine_part(say, a.calls, a.layers)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
