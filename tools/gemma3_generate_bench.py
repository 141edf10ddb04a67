#!/usr/bin/env python3
"""Gemma3LRP.generate() and explain(positions=...) on the MI355X.
  1. lrp_decode_qknorm_rope_append against the three launches it replaces (2 x lrp_head_rmsnorm_fwd + lrp_decode_rope_append) at the
     Gemma-3-4B head shape (8 query / 4 kv heads of 256, bf16), B in {1, 4}: microseconds from device events around one eager call (median
     of --reps after warm-up; this includes the launches' host side), and microseconds per call inside a replayed hipGraph of 64 back-to-back
     calls (what a captured decode step pays), the two forms alternated.
  2. Gemma3LRP.generate at the Gemma-3-4B text shape (bench.config4_text_engine: synthetic weights, the released 262208-token vocabulary,
     bf16), S = 2048, 64 new tokens, B in {1, 4}: milliseconds per token = (the call - a 1-token call) / 63, eager and graph=True, with the
     fused site kernel and with the three launches in its place (the same engine, ops.decode_qknorm_rope_append swapped for the
     composition by this tool), against the floor: the bytes of the weights a step streams plus the live K / V rows it reads (a sliding
     layer reads at most `window` rows), over 6.3 TB/s.  HF `generate` (bf16, sdpa, its own cache; a model of its own random init: timing
     only) on the same device, if transformers runs it there.
  3. explain(positions=...) with T = 64 explained rows against the plain call, S = 2048, B in {1, 4}, both objectives.
usage: python tools/gemma3_generate_bench.py [--out FILE] [--reps 30] [--layers 34] [--new 64] [--no-hf] [--no-kernel] [--no-span]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

HBM = 6.3e12          # achievable HBM rate the floors are quoted against


def timed(fn, reps):
    """median and minimum microseconds of fn() over reps calls, each between two device events"""
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


def three_launches(ops, scratch):
    """-> a function with ops.decode_qknorm_rope_append's signature that runs the launch sequence it replaces; scratch: {} for its buffers"""
    def run(qk, v, wq, wk, eps, cos, sin, pos, q_rot, kc, vc, nq, nk, d, w_offset=0.0):
        B = qk.shape[0]
        key = (B, nq, nk, d, qk.dtype)
        if key not in scratch:
            scratch[key] = (torch.empty(B, (nq + nk) * d, device=qk.device, dtype=qk.dtype), torch.empty(B * nq, device=qk.device),
                            torch.empty(B * nk, device=qk.device))
        qn, rq, rk = scratch[key]
        ops.head_rmsnorm_fwd(qk[:, : nq * d], wq, qn[:, : nq * d], rq, nq, d, eps, w_offset)
        ops.head_rmsnorm_fwd(qk[:, nq * d:], wk, qn[:, nq * d:], rk, nk, d, eps, w_offset)
        return ops.decode_rope_append(qn, v, cos, sin, pos, q_rot, kc, vc, nq, nk, d)
    return run


def kernel_part(ops, say, reps):
    nq, nk, d, dt, cap, chain = 8, 4, 256, torch.bfloat16, 2112, 64
    say(f"lrp_decode_qknorm_rope_append vs 2 x lrp_head_rmsnorm_fwd + lrp_decode_rope_append, {nq} / {nk} heads of {d}, bf16; eager: us = median (min) "
        f"of {reps} device-event times around ONE call; graph: us per call in a replayed hipGraph of {chain} calls, median (min) of {reps} replays")
    g = torch.Generator(device="cuda").manual_seed(0)
    unfused = three_launches(ops, {})
    for B in (1, 4):
        qkv = torch.randn(B, (nq + 2 * nk) * d, generator=g, device="cuda").to(dt)
        wq, wk = (torch.randn(d, generator=g, device="cuda") * 0.1).to(dt), (torch.randn(d, generator=g, device="cuda") * 0.1).to(dt)
        ang = torch.rand(cap, d, generator=g, device="cuda") * 6.0
        cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
        pos = torch.tensor([2048], dtype=torch.int32, device="cuda")
        nqk = (nq + nk) * d
        outs = {}
        for name, fn in (("fused", ops.decode_qknorm_rope_append), ("three launches", unfused)):
            kc, vc = torch.zeros(B, cap, nk * d, device="cuda", dtype=dt), torch.zeros(B, cap, nk * d, device="cuda", dtype=dt)
            q = torch.zeros(B, nq * d, device="cuda", dtype=dt)
            call = lambda fn=fn, q=q, kc=kc, vc=vc: fn(qkv[:, :nqk], qkv[:, nqk:], wq, wk, 1e-6, cos, sin, pos, q, kc, vc, nq, nk, d, 1.0)      # noqa: E731
            for _ in range(5):
                call()
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                call()
            torch.cuda.current_stream().wait_stream(side)
            with torch.cuda.graph(cg):
                for _ in range(chain):
                    call()
            cg.replay()
            torch.cuda.synchronize()
            outs[name] = (call, cg, q, kc)
        same = torch.equal(outs["fused"][2], outs["three launches"][2]) and torch.equal(outs["fused"][3], outs["three launches"][3])
        res = {n: dict(eager=[], graph=[]) for n in outs}
        for _ in range(3):                                   # the two forms alternated, three rounds
            for n, (call, cg, _, _) in outs.items():
                res[n]["eager"].append(timed(call, reps))
                res[n]["graph"].append(tuple(x / chain for x in timed(cg.replay, reps)))
        for n in outs:
            e = min(res[n]["eager"])
            gph = min(res[n]["graph"])
            say(f"  B {B} {n:15s}: eager {e[0]:7.2f} us ({e[1]:7.2f})   in a replayed graph {gph[0]:6.2f} us ({gph[1]:6.2f}) per call")
        say(f"  B {B}: outputs bitwise equal: {same}")


def engine_part(say, layers, new):
    import bench
    from lxt_amd import ops
    S = 2048
    eng, _, V = bench.config4_text_engine("cuda", torch.bfloat16, S4=S + new, L=layers)
    c = eng.cfg
    H, I, d, nq, nk, win = c["hidden"], c["inter"], c["head_dim"], c["n_heads"], c["n_kv"], c["window"]
    lin = layers * ((nq + 2 * nk) * d * H + H * nq * d + 3 * I * H)
    wbytes = 2.0 * (lin + V * H)                              # every Linear once, the tied head once (the embedding rows are B gathers)
    n_slide = sum(t == "sliding_attention" for t in c["layer_types"])
    fused, unfused = ops.decode_qknorm_rope_append, three_launches(ops, {})
    say(f"Gemma3LRP.generate, Gemma-3-4B text shape, {layers} layers ({n_slide} sliding, window {win}), vocabulary {V}, bf16, S = {S}, {new} new tokens; "
        f"ms per token = (call - a 1-token call) / {new - 1}, medians of 3 rounds, the two site forms alternated inside each round")
    rows = {}
    for B in (1, 4):
        ids = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(B)).cuda()
        live = S + new / 2
        kv = 2.0 * B * nk * d * 2 * ((layers - n_slide) * live + n_slide * min(win, live))
        for graph in (False, True):
            variants = (("fused site kernel", fused), ("three launches", unfused))
            pre, tot = {v[0]: [] for v in variants}, {v[0]: [] for v in variants}
            for rnd in range(5):                              # two warm-up rounds (capture included), three timed
                for label, fn in variants:
                    ops.decode_qknorm_rope_append = fn
                    eng._graphs.clear()                       # (a graph holds the form it was captured with)
                    if rnd < 2 or graph:
                        eng.generate(ids, 3, graph=graph)
                        eng.generate(ids, new, graph=graph)
                    if rnd >= 2:
                        pre[label].append(wall(lambda: eng.generate(ids, 1))[0])
                        tot[label].append(wall(lambda: eng.generate(ids, new, graph=graph))[0])
            ops.decode_qknorm_rope_append = fused
            for label, _ in variants:
                p_, t_ = statistics.median(pre[label]), statistics.median(tot[label])
                per, floor = (t_ - p_) / (new - 1), (wbytes + kv) / HBM * 1e3
                rows[(label, B, graph)] = per
                say(f"  B {B} {'graph' if graph else 'eager'} {label:18s}: prefill + first token {p_:8.2f} ms, {new} tokens {t_:8.2f} ms -> {per:6.3f} ms per "
                    f"token; floor {floor:5.3f} ms ({wbytes / 1e9:.2f} GB weights + {kv / 1e9:.3f} GB K / V at 6.3 TB/s) = {floor / per:5.3f} of the step")
    return eng, V, rows


def span_part(say, eng, V):
    S, T = 2048, 64
    say(f"Gemma3LRP.explain(positions=...) with T = {T} explained rows (the last {T} columns but one) against the plain call, S = {S}, bf16; ms = "
        "median of 3 wall-clock calls after a warm-up")
    for B in (1, 4):
        ids = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(10 + B)).cuda()
        pos = torch.arange(S - 1 - T, S - 1).expand(B, T)
        calls = (("plain", lambda: eng.explain(ids)), ("span logit", lambda: eng.explain(ids, positions=pos)),
                 ("span logprob", lambda: eng.explain(ids, positions=pos, objective="logprob")))
        ms = {}
        for name, fn in calls:
            fn()
            ms[name] = statistics.median(wall(fn)[0] for _ in range(3))
        say(f"  B {B}: plain {ms['plain']:8.2f} ms   span logit {ms['span logit']:8.2f} ms ({ms['span logit'] / ms['plain']:4.2f} x)   span logprob "
            f"{ms['span logprob']:8.2f} ms ({ms['span logprob'] / ms['plain']:4.2f} x)   = {T} single-position calls in "
            f"{ms['span logit'] / (T * ms['plain']):5.3f} of their time")


def hf_part(say, layers, new, rows):
    S, V = 2048, 262208
    try:
        from transformers import Gemma3ForCausalLM, Gemma3TextConfig
        cfg = Gemma3TextConfig(vocab_size=V, hidden_size=2560, intermediate_size=10240, num_hidden_layers=layers, num_attention_heads=8,
                               num_key_value_heads=4, head_dim=256, sliding_window=1024, max_position_embeddings=8192,
                               layer_types=[("full_attention" if (i + 1) % 6 == 0 else "sliding_attention") for i in range(layers)],
                               query_pre_attn_scalar=256, attn_implementation="sdpa", tie_word_embeddings=True)
        with torch.device("cuda"):
            model = Gemma3ForCausalLM(cfg).to(torch.bfloat16).eval()
        for B in (1, 4):
            ids = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(B)).cuda()
            gen = lambda n: model.generate(ids, attention_mask=torch.ones_like(ids), max_new_tokens=n, min_new_tokens=n, do_sample=False,      # noqa: E731
                                           pad_token_id=0)
            with torch.no_grad():
                gen(3)
                pre = statistics.median(wall(lambda: gen(1))[0] for _ in range(3))
                tot = statistics.median(wall(lambda: gen(new))[0] for _ in range(3))
            per = (tot - pre) / (new - 1)
            say(f"  B {B} HF generate (sdpa, bf16, its own cache): prefill + first token {pre:8.2f} ms, {new} tokens {tot:8.2f} ms -> {per:6.3f} ms per "
                f"token = {per / rows[('fused site kernel', B, False)]:5.2f} x the eager engine step, "
                f"{per / rows[('fused site kernel', B, True)]:5.2f} x the graph step")
    except Exception as e:          # noqa: BLE001  (the comparison is optional; say what happened instead of a number)
        say(f"  HF generate: not measured ({type(e).__name__}: {e})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--layers", type=int, default=34)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--no-hf", action="store_true")
    ap.add_argument("--no-kernel", action="store_true", help="skip part 1 (the site kernel alone)")
    ap.add_argument("--no-span", action="store_true", help="skip part 3 (explain(positions=...))")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemma3_generate_bench needs a HIP device")
    from lxt_amd import ops
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:          # (written as it goes: a later part that fails keeps the earlier lines)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if not a.no_kernel:
        kernel_part(ops, say, a.reps)
    eng, V, rows = engine_part(say, a.layers, a.new)
    if not a.no_span:
        span_part(say, eng, V)
    eng.release()
    del eng
    torch.cuda.empty_cache()
    if not a.no_hf:
        hf_part(say, a.layers, a.new, rows)


if __name__ == "__main__":
    main()
