#!/usr/bin/env python3
"""Repetition / presence / frequency penalties on the MI355X: what lrp_logit_penalty costs and what it adds to a
decode step.
  1. lrp_logit_penalty alone on fp32 logits 3 randn, V in {128256, 262208}, B in {1, 4, 128}, the table of a 2048-token prompt with 64
     generated tokens: repetition penalty only, and all three with a bias.  Microseconds from device events, median (min) of --reps
     windows, two ways: ONE call per window (what a token loop that waits for its token sees: launch latency included), and 50 calls back to
     back per window divided by 50 (the kernel's own time once launches overlap).  Beside each the time its bytes take at 6.3 TB/s, the
     project's HBM figure -- 12 B per element, 16 with a bias (the bias row is re-read per row of the batch: those reads are L2 hits) -- and
     the fraction of that floor reached; lrp_span_seed (objective "logit": one read of the row) and lrp_argmax_rows on the same logits,
     timed the same way, as the yardsticks of section 20; the smallest call the entry can make (V = 64, B = 1) as the launch floor; and
     lrp_token_hist_init of a [B, 2048] prompt.  Every call of a window works on the next of up to 4 sets of buffers, enough sets to exceed
     768 MB where 4 suffice (B = 128): a repeated call on one 200 MB set would be served by the 256 MB Infinity Cache, not by HBM.
  2. LlamaLRP.generate at the Llama-3-8B shape (synthetic weights, bf16), S = 2048, 64 new tokens, B in {1, 4}, graph=True: milliseconds per
     token with penalties (repetition 1.1, presence 0.5, frequency 0.25) against without, alternated in one session, tools/generate_bench.py's
     method ((call - a 1-token call) / (new - 1), medians of 3 rounds).
usage: python tools/penalty_bench.py [--out FILE] [--reps 30] [--layers 32] [--new 64] [--no-engine]"""
import argparse
import itertools
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

HBM = 6.3e12          # bytes / s
BURST = 50
SETTINGS = (("repetition 1.1", dict(repetition_penalty=1.1), False),
            ("all three + bias", dict(repetition_penalty=1.1, presence_penalty=0.5, frequency_penalty=0.25), True))


def timed(fn, reps, burst=1):
    """median and min microseconds per call of fn() over reps windows of `burst` calls, each window between two device events"""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(burst):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / burst)
    return statistics.median(ts), min(ts)


def both(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return timed(fn, reps), timed(fn, reps, BURST)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def kernel_part(ops, say, reps):
    say(f"lrp_logit_penalty on fp32 logits 3 randn, the table of a 2048-token prompt + 64 generated tokens; us per call = median (min) of {reps} "
        f"device-event windows: 'single' = one call per window, 'burst' = {BURST} calls back to back per window / {BURST}; floor = bytes / 6.3 TB/s")
    g = torch.Generator(device="cuda").manual_seed(0)
    tiny_l, tiny_h = torch.randn(1, 64, device="cuda"), torch.zeros(1, 64, dtype=torch.int32, device="cuda")
    tiny_o = torch.empty_like(tiny_l)
    (ls, _), (lb, _) = both(lambda: ops.logit_penalty(tiny_l, tiny_h, repetition_penalty=1.1, out=tiny_o), reps)
    say(f"  launch floor (V 64, B 1): single {ls:7.1f} us  burst {lb:7.1f} us")
    for V in (128256, 262208):
        for B in (1, 4, 128):
            nsets = min(4, max(1, math.ceil(768e6 / (12.0 * B * V))))
            ids = torch.randint(0, V, (B, 2048), generator=g, device="cuda")
            gen = torch.randint(0, V, (B, 64), generator=g, device="cuda")
            sets = []
            for _ in range(nsets):
                logits = 3.0 * torch.randn(B, V, generator=g, device="cuda")
                hist = ops.token_hist_init(ids, None, V)
                hist.scatter_add_(1, gen, torch.ones_like(gen, dtype=torch.int32))
                sets.append((logits, hist, torch.empty_like(logits), torch.empty(B, V, dtype=torch.int32, device="cuda")))
            ring = itertools.cycle(sets)
            last = gen[:, -1].to(torch.int32).contiguous()
            bias = torch.randn(V, generator=g, device="cuda")
            idx = ops.argmax_rows(sets[0][0])[0]
            (hs, _), (hb, _) = both(lambda: ops.token_hist_init(ids, None, V, hist=next(ring)[3]), reps)
            (am, _), (ab, _) = both(lambda: ops.argmax_rows(next(ring)[0]), reps)
            (sm, _), (sb, _) = both(lambda: ops.span_seed(next(ring)[0], idx), reps)
            rd = 4.0 * B * V / HBM * 1e6
            say(f"  V {V} B {B:3d} ({nsets} buffer sets of {12e-6 * B * V:6.1f} MB): lrp_argmax_rows single {am:7.1f} burst {ab:7.1f} us   lrp_span_seed single {sm:7.1f} burst {sb:7.1f} us "
                f"(one read of the rows: floor {rd:6.2f} us, burst reaches {100 * rd / sb:5.1f} %)   lrp_token_hist_init single {hs:7.1f} burst {hb:7.1f} us")
            for label, kw, with_bias in SETTINGS:
                def fn():
                    lg, h, o, _ = next(ring)
                    return ops.logit_penalty(lg, h, None, bias=bias if with_bias else None, out=o, **kw)

                (m1, b1), (m2, b2) = both(fn, reps)
                floor = (16.0 if with_bias else 12.0) * B * V / HBM * 1e6
                say(f"      {label:16s}: single {m1:7.1f} us ({b1:7.1f})  burst {m2:7.1f} us ({b2:7.1f})  floor {floor:7.2f} us  -> "
                    f"{100 * floor / m1:5.1f} % (single) {100 * floor / m2:5.1f} % (burst) of the byte floor")
            lg, h, o, _ = sets[0]
            assert int(ops.logit_penalty(lg, h.clone(), last, out=o, **SETTINGS[1][1]).isnan().sum()) == 0          # (with `last`: a count moves)
            del sets, ring


def engine_part(say, layers, new):
    import bench
    import lxt_amd.engine as E
    cfg = dict(bench.LLAMA3_8B, n_layers=layers)
    S, V = 2048, cfg["vocab"]
    W = bench.synth_weights(cfg, "cuda", torch.bfloat16, seed=0)
    eng = E.LlamaLRP(cfg, W, dtype=torch.bfloat16, mode="efficient", max_seq=S + new + 1)
    del W
    variants = (("plain", dict()), ("penalised", dict(repetition_penalty=1.1, presence_penalty=0.5, frequency_penalty=0.25)))
    say(f"LlamaLRP.generate, Llama-3-8B shape, {layers} layers, bf16, S = {S}, {new} new tokens, graph=True, greedy; ms per token = (call - a 1-token "
        f"call) / {new - 1}, medians of 3 rounds, plain and penalised (repetition 1.1, presence 0.5, frequency 0.25) alternated inside each round")
    for B in (1, 4):
        ids = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(B)).cuda()
        pre, tot = {v[0]: [] for v in variants}, {v[0]: [] for v in variants}
        for rnd in range(5):                                                                # two warm-up rounds (capture included), three timed
            for label, kw in variants:
                if rnd < 2:
                    eng.generate(ids, 3, graph=True, **kw)
                    eng.generate(ids, new, graph=True, **kw)
                else:
                    pre[label].append(wall(lambda: eng.generate(ids, 1, **kw))[0])
                    tot[label].append(wall(lambda: eng.generate(ids, new, graph=True, **kw))[0])
        per = {}
        for label, _ in variants:
            p_, t_ = statistics.median(pre[label]), statistics.median(tot[label])
            per[label] = (t_ - p_) / (new - 1)
            say(f"  B {B} {label:9s}: prefill + first token {p_:8.2f} ms, {new} tokens {t_:8.2f} ms ({min(tot[label]):8.2f} .. {max(tot[label]):8.2f}) -> "
                f"{per[label]:6.3f} ms per token")
        d = per["penalised"] - per["plain"]
        say(f"  B {B} the penalties add {d * 1e3:7.1f} us per token = {100 * d / per['plain']:5.2f} % of the plain step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--no-engine", action="store_true", help="skip part 2 (generate at the 8B shape)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("penalty_bench needs a HIP device")
    from lxt_amd import ops
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:          # (written as it goes: a later part that fails keeps the earlier lines)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    kernel_part(ops, say, a.reps)
    if not a.no_engine:
        engine_part(say, a.layers, a.new)


if __name__ == "__main__":
    main()
