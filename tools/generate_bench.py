#!/usr/bin/env python3
"""KV-cached generation on the MI355X: what a decode step of LlamaLRP.generate costs and how far it is from its floor.
  1. lrp_attn_decode alone at the Llama-3-8B head shape (32 query / 8 kv heads of 128, bf16), live lengths 2048 and 4096, B in {1, 4}:
     microseconds from device events (median of --reps timed calls after warm-up), the K and V bytes of the live rows per second, and beside
     it lrp_attn_fwd(q_begin = S - 1) on the same operands (what the library had for one live query row) and torch's
     scaled_dot_product_attention on the same operands with one query row.
  2. LlamaLRP.generate at the Llama-3-8B shape (synthetic weights, bf16), S = 2048, 64 new tokens, B in {1, 4}: milliseconds per token of the
     decode steps, eager and graph=True (the prefill is timed on its own and taken off), against the floor (the bytes of the weights a step
     streams + the live K / V bytes) / 6.3 TB/s, and HF `generate` (sdpa, its own cache) on the same device at the same shape (a model of its
     own random init: timing only).
     --weight-format mxfp4 adds the quantised engine: reading the codes in place and, on the same build, the
     dequantise-per-token launch sequence it replaced (ops.STREAM_Q = False), alternated call by call with the bf16 engine.
usage: python tools/generate_bench.py [--out FILE] [--reps 30] [--layers 32] [--new 64] [--no-hf] [--no-kernel] [--weight-format mxfp4]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

HBM = 6.3e12          # achievable HBM rate the floors are quoted against


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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def kernel_part(ops, say, reps):
    Hq, Hkv, d, dt = 32, 8, 128, torch.bfloat16
    scale = d ** -0.5
    say(f"lrp_attn_decode, Hq {Hq} / Hkv {Hkv} heads of {d}, bf16; us = median (min) of {reps} device-event times; bytes = the live K and V rows")
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in (2048, 4096):
        for B in (1, 4):
            q = torch.randn(B, Hq * d, generator=g, device="cuda").to(dt)
            kc = torch.randn(B, n, Hkv * d, generator=g, device="cuda").to(dt)
            vc = torch.randn(B, n, Hkv * d, generator=g, device="cuda").to(dt)
            lo = torch.zeros(B, dtype=torch.int32, device="cuda")
            pos = torch.tensor([n - 1], dtype=torch.int32, device="cuda")
            out = torch.empty(B, Hq * d, device="cuda", dtype=dt)
            ws = torch.empty(ops.attn_decode_ws(B, Hq, d, n), dtype=torch.uint8, device="cuda")
            # the same operands as a prefill-shaped call with one live query row per prompt: q as row S - 1 of a [B S, Hq d] tensor
            qf = torch.zeros(B * n, Hq * d, device="cuda", dtype=dt)
            qf[n - 1:: n] = q
            of, lse = torch.empty_like(qf), torch.empty(B, Hq, n, device="cuda")
            k2, v2 = kc.view(B * n, Hkv * d), vc.view(B * n, Hkv * d)
            v_t = ops.transpose_heads(v2, B, n, Hkv, d) if ops.attn_needs_transposed(v2, d) else None
            q4 = q.view(B, Hq, 1, d)
            k4, v4 = kc.view(B, n, Hkv, d).transpose(1, 2), vc.view(B, n, Hkv, d).transpose(1, 2)

            def dec():
                ops.attn_decode(q, kc, vc, lo, pos, Hq, Hkv, d, scale, out=out, ws=ws)

            def fwd():
                ops.attn_fwd(qf, k2, v2, v_t, of, lse, B, n, Hq, Hkv, d, scale, True, 0, q_begin=n - 1)

            def sdpa():
                torch.nn.functional.scaled_dot_product_attention(q4, k4, v4, enable_gqa=True)

            for fn in (dec, fwd, sdpa):
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            err = float((out.float() - of[n - 1:: n].float()).abs().max() / of[n - 1:: n].float().abs().max())
            nbytes = 2.0 * B * n * Hkv * d * 2
            (dm, db), (fm, fb), (sm, sb) = timed(dec, reps), timed(fwd, reps), timed(sdpa, reps)
            say(f"  live {n:5d} B {B}: attn_decode {dm:7.1f} us ({db:7.1f})  {nbytes / dm / 1e6:6.3f} TB/s = {nbytes / (dm * 1e-6) / HBM:5.3f} of 6.3 TB/s"
                f"   attn_fwd(q_begin = S - 1) {fm:7.1f} us ({fb:7.1f})  {nbytes / fm / 1e6:6.3f} TB/s   torch sdpa {sm:7.1f} us ({sb:7.1f})  "
                f"{nbytes / sm / 1e6:6.3f} TB/s   [decode vs attn_fwd row, max-normalised {err:.1e}]")


def engine_part(say, layers, new, hf, weight_format=None):
    import bench
    import lxt_amd.engine as E
    from lxt_amd import ops
    cfg = dict(bench.LLAMA3_8B, n_layers=layers)
    S = 2048
    H, I, d, nq, nk, V = cfg["hidden"], cfg["inter"], cfg["head_dim"], cfg["n_heads"], cfg["n_kv"], cfg["vocab"]
    W = bench.synth_weights(cfg, "cuda", torch.bfloat16, seed=0)
    mk = lambda fmt: E.LlamaLRP(cfg, W, dtype=torch.bfloat16, mode="efficient", max_seq=S + new + 1, weight_format=fmt)      # noqa: E731
    lin = layers * ((nq + 2 * nk) * d * H + H * nq * d + 3 * I * H)                                # elements of the Linears of every layer
    # variants: (label, engine, ops.STREAM_Q while it runs, bytes of weights a step must read).  weight_format="mxfp4": the engine that reads the
    # codes, the SAME build with ops.STREAM_Q = False -- the launch sequence before section 22: four dequantisations per
    # layer and token, then the bf16 stream kernels -- on an engine (and graph cache) of its own, and the bf16 engine; alternated call by call
    if weight_format is None:
        variants = [("bf16", mk(None), True, 2.0 * (lin + V * H))]
    else:
        qb = lin * 4.25 / 8 + 2.0 * V * H
        variants = [(f"{weight_format} codes", mk(weight_format), True, qb), (f"{weight_format} dequant per token", mk(weight_format), False, qb),
                    ("bf16", mk(None), True, 2.0 * (lin + V * H))]
    del W
    say(f"LlamaLRP.generate, Llama-3-8B shape, {layers} layers, bf16, S = {S}, {new} new tokens; ms per token = (call - a 1-token call) / {new - 1}, "
        f"medians of 3 rounds, the variants alternated inside each round")
    rows = {}
    for B in (1, 4):
        ids = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(B)).cuda()
        kv = 2.0 * layers * B * (S + new / 2) * nk * d * 2                                       # live K and V rows, mid-way through the answer
        for graph in (False, True):
            pre, tot = {v[0]: [] for v in variants}, {v[0]: [] for v in variants}
            for rnd in range(5):                                                                # two warm-up rounds (capture included), three timed
                for label, eng, sq, _ in variants:
                    ops.STREAM_Q = sq
                    if rnd < 2:
                        eng.generate(ids, 3, graph=graph)
                        eng.generate(ids, new, graph=graph)
                    else:
                        pre[label].append(wall(lambda: eng.generate(ids, 1))[0])
                        tot[label].append(wall(lambda: eng.generate(ids, new, graph=graph))[0])
            ops.STREAM_Q = True
            for label, _, _, wbytes in variants:
                p_, t_ = statistics.median(pre[label]), statistics.median(tot[label])
                per, floor = (t_ - p_) / (new - 1), (wbytes + kv) / HBM * 1e3
                rows[(label, B, graph)] = per
                say(f"  B {B} {'graph' if graph else 'eager'} {label:28s}: prefill + first token {p_:8.2f} ms, {new} tokens {t_:8.2f} ms -> {per:6.3f} ms per "
                    f"token; floor {floor:5.3f} ms ({wbytes / 1e9:.2f} GB weights + {kv / 1e9:.3f} GB K / V at 6.3 TB/s) = {floor / per:5.3f} of the step")
    rows.update({(B, g): rows[("bf16", B, g)] for B in (1, 4) for g in (False, True)})
    del variants
    torch.cuda.empty_cache()
    if not hf:
        return
    try:
        from transformers import LlamaConfig, LlamaForCausalLM
        kw = dict(hidden_size=H, intermediate_size=I, num_hidden_layers=layers, num_attention_heads=nq, num_key_value_heads=nk, vocab_size=V,
                  rms_norm_eps=1e-5, max_position_embeddings=8192, tie_word_embeddings=False, attn_implementation="sdpa")
        with torch.device("cuda"):
            model = LlamaForCausalLM(LlamaConfig(**kw)).to(torch.bfloat16).eval()
        for B in (1, 4):
            ids = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(B)).cuda()
            gen = lambda n: model.generate(ids, attention_mask=torch.ones_like(ids), max_new_tokens=n, min_new_tokens=n, do_sample=False,      # noqa: E731
                                           pad_token_id=0)
            with torch.no_grad():
                gen(3)
                pre = statistics.median(wall(lambda: gen(1))[0] for _ in range(3))
                tot = statistics.median(wall(lambda: gen(new))[0] for _ in range(3))
            per = (tot - pre) / (new - 1)
            say(f"  B {B} HF generate (sdpa, bf16, DynamicCache): prefill + first token {pre:8.2f} ms, {new} tokens {tot:8.2f} ms -> {per:6.3f} ms per "
                f"token = {per / rows[(B, False)]:5.2f} x the eager engine step, {per / rows[(B, True)]:5.2f} x the graph step")
    except Exception as e:          # noqa: BLE001  (the comparison is optional; say what happened instead of a number)
        say(f"  HF generate: not measured ({type(e).__name__}: {e})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--no-hf", action="store_true")
    ap.add_argument("--weight-format", default=None, choices=[None, "mxfp4"], help="also run the quantised engine (codes read in place, and the "
                    "dequantise-per-token sequence) beside the bf16 one")
    ap.add_argument("--no-kernel", action="store_true", help="skip part 1 (lrp_attn_decode alone)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("generate_bench needs a HIP device")
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
    engine_part(say, a.layers, a.new, not a.no_hf, a.weight_format)


if __name__ == "__main__":
    main()
