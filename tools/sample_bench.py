#!/usr/bin/env python3
"""Seeded sampling on the MI355X: what lrp_sample_rows costs and what it adds to a decode step.
  1. lrp_sample_rows alone on fp32 logits 3 randn, V in {128256, 262208}, B in {1, 4, 128}: filters off, top-k 20, top-p 0.95, all three
     (T 0.7, top-k 20, top-p 0.95, min-p 0.02).  Microseconds from device events (median (min) of --reps timed calls after warm-up) and the
     bytes of ONE pass over the rows per second; beside it lrp_argmax_rows on the same logits (what the greedy path launches) and the torch
     composition a user would write on the same device: sort, softmax, cumsum, mask, multinomial.
  2. LlamaLRP.generate at the Llama-3-8B shape (synthetic weights, bf16), S = 2048, 64 new tokens, B in {1, 4}, graph=True: milliseconds per
     token sampled (T 0.7, top-k 20, top-p 0.95) against greedy, alternated in one session, tools/generate_bench.py's method
     ((call - a 1-token call) / (new - 1), medians of 3 rounds).
usage: python tools/sample_bench.py [--out FILE] [--reps 30] [--layers 32] [--new 64] [--no-engine]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

SETTINGS = (("filters off", dict(temperature=0.7)), ("top-k 20", dict(temperature=0.7, top_k=20)), ("top-p 0.95", dict(temperature=0.7, top_p=0.95)),
            ("all three", dict(temperature=0.7, top_k=20, top_p=0.95, min_p=0.02)))


def timed(fn, reps):
    """median and min microseconds of fn() over reps calls, each between two device events"""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def torch_sample(logits, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0):
    """the composition a user would write: temperature, top-k, top-p on a sort, min-p, multinomial"""
    s = logits / temperature
    if top_k:
        s = s.masked_fill(s < torch.topk(s, top_k)[0][..., -1, None], float("-inf"))
    if top_p < 1:
        srt, order = torch.sort(s, descending=False)
        drop = srt.softmax(-1).cumsum(-1) <= 1 - top_p
        drop[..., -1:] = False
        s = s.masked_fill(drop.scatter(1, order, drop), float("-inf"))
    if min_p:
        pr = s.softmax(-1)
        s = s.masked_fill(pr < min_p * pr.amax(-1, keepdim=True), float("-inf"))
    return torch.multinomial(s.softmax(-1), 1)


def kernel_part(ops, say, reps):
    say(f"lrp_sample_rows on fp32 logits 3 randn; us = median (min) of {reps} device-event times; GB/s = the bytes of ONE pass over the rows "
        f"(4 B V) per second -- the kernel makes 2 (filters off), 6 (top-k or top-p) or 10 (both) passes, the first from HBM, the others L2 hits")
    g = torch.Generator(device="cuda").manual_seed(0)
    for V in (128256, 262208):
        for B in (1, 4, 128):
            logits = 3.0 * torch.randn(B, V, generator=g, device="cuda")
            seeds = torch.full((B,), 1234, dtype=torch.int64, device="cuda")
            streams = torch.arange(B, dtype=torch.int32, device="cuda")
            nbytes = 4.0 * B * V
            fa = lambda: ops.argmax_rows(logits)          # noqa: E731
            for _ in range(3):
                fa()
            am, ab = timed(fa, reps)
            say(f"  V {V} B {B:3d}: lrp_argmax_rows {am:8.1f} us ({ab:8.1f})  {nbytes / am / 1e3:8.1f} GB/s")
            for label, kw in SETTINGS:
                fs = lambda: ops.sample_rows(logits, seeds=seeds, streams=streams, step=3, **kw)          # noqa: E731
                ft = lambda: torch_sample(logits, **kw)          # noqa: E731
                for _ in range(3):
                    fs()
                    ft()
                torch.cuda.synchronize()
                (sm, sb), (tm, tb) = timed(fs, reps), timed(ft, max(5, reps // 3))
                nk = ops.sample_rows(logits, seeds=seeds, streams=streams, step=3, **kw)[2]
                say(f"      {label:12s}: lrp_sample_rows {sm:8.1f} us ({sb:8.1f})  {nbytes / sm / 1e3:8.1f} GB/s  = {sm / am:6.2f} x argmax_rows   "
                    f"torch composition {tm:9.1f} us ({tb:9.1f}) = {tm / sm:6.2f} x lrp_sample_rows   [kept per row {int(nk.min())} .. {int(nk.max())}]")


def engine_part(say, layers, new):
    import bench
    import lxt_amd.engine as E
    cfg = dict(bench.LLAMA3_8B, n_layers=layers)
    S, V = 2048, cfg["vocab"]
    W = bench.synth_weights(cfg, "cuda", torch.bfloat16, seed=0)
    eng = E.LlamaLRP(cfg, W, dtype=torch.bfloat16, mode="efficient", max_seq=S + new + 1)
    del W
    variants = (("greedy", dict()), ("sampled", dict(do_sample=True, seed=7, temperature=0.7, top_k=20, top_p=0.95)))
    say(f"LlamaLRP.generate, Llama-3-8B shape, {layers} layers, bf16, S = {S}, {new} new tokens, graph=True; ms per token = (call - a 1-token call) "
        f"/ {new - 1}, medians of 3 rounds, greedy and sampled (T 0.7, top-k 20, top-p 0.95) alternated inside each round")
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
            say(f"  B {B} {label:8s}: prefill + first token {p_:8.2f} ms, {new} tokens {t_:8.2f} ms ({min(tot[label]):8.2f} .. {max(tot[label]):8.2f}) -> "
                f"{per[label]:6.3f} ms per token")
        d = per["sampled"] - per["greedy"]
        say(f"  B {B} sampling adds {d * 1e3:7.1f} us per token = {100 * d / per['greedy']:5.2f} % of the greedy step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--no-engine", action="store_true", help="skip part 2 (generate at the 8B shape)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench needs a HIP device")
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
