#!/usr/bin/env python3
"""MXFP4 weight storage on the MI355X (profiles/mxfp4_bench.txt):
  (1) lrp_mxfp4_dequant at the four Linear matrices of a Llama-3-8B layer, at the engine's pitches, bf16: time per call from device events
      (median and best over --reps timed calls after warm-up), the bytes the algorithm must move (codes + scales read, bf16 written) over it
      and that rate over the 8 TB/s HBM peak -- next to three yardsticks of the same process: a device-to-device copy of the bf16 matrix
      (read + write), lrp_colsum_dot (a streaming read of two [8192, N] operands) and the weight-streaming Linear at M = 8;
  (2) the step time of LlamaLRP(weight_format="mxfp4") on the random-init benchmark model (bench.py's weights, --layers layers), S = 2048, at
      4 prompts and at 1 prompt per step, against two ordinary engines in this process, the three alternating inside every round: `deq`, built
      from the quantised engine's dequantised weights -- the same operand data in every GEMM, so the difference to it IS the overhead of the
      feature -- and `none`, built from the original weights (full-mantissa operands: MFMA clocks depend on operand entropy, so this
      difference mixes the overhead with a data effect);
  (3) for the record: cosine and normalised-max distance of R_tok between the two engines on --prompts seeded prompts.  Random weights are
      the worst case for a 4-bit format (no structure for the block scales to follow).
usage: python tools/mxfp4_bench.py [--out FILE] [--layers 32] [--reps 50] [--rounds 5] [--steps 2] [--prompts 4]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    """(median, best) milliseconds of fn() over reps calls, each between two device events"""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--prompts", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mxfp4_bench needs a HIP device")
    import bench
    from lxt_amd import ops
    import lxt_amd.engine as E
    dev, bf = torch.device("cuda", 0), torch.bfloat16
    lines = [f"device: {torch.cuda.get_device_name(0)}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def rate(nbytes, ms):
        return f"{nbytes / ms / 1e9:5.2f} TB/s = {nbytes / ms / 1e9 / 8.0:.2f} of 8 TB/s"

    # ---- (1) the kernel at the four matrices of a layer
    cfg = dict(bench.LLAMA3_8B, n_layers=a.layers)
    _, layer = E.LlamaLRP.flat_layout(cfg, bf)
    _, lin, qspec = E.quant_layout(layer)
    _, _, (qv,) = E.pack_flat({}, qspec, 1, torch.uint8, dev, align=128)
    _, _, (wv,) = E.pack_flat({}, lin, 1, bf, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    say(f"lrp_mxfp4_dequant, bf16, the Linears of a Llama-3-8B layer at the engine's pitches; {a.reps} timed calls each:")
    tot_ms = tot_bytes = 0.0
    for k, ((N, K), pitch) in lin.items():
        wv[k].copy_((torch.randn(N, K, generator=g, device=dev) * 0.02).to(bf))
        ops.mxfp4_quantize(wv[k], qv[k + "_c"], qv[k + "_s"])
        fn = lambda: ops.mxfp4_dequant(qv[k + "_c"], qv[k + "_s"], wv[k])      # noqa: E731
        for _ in range(5):
            fn()
        med, best = timed(fn, a.reps)
        nbytes = N * K // 2 + N * K // 32 + N * K * 2
        tot_ms, tot_bytes = tot_ms + med, tot_bytes + nbytes
        say(f"  {k:5s} [{N:5d}, {K:5d}] pitch {pitch or K:5d}: {med * 1e3:7.1f} us median, {best * 1e3:7.1f} us best; {nbytes / 1e6:6.1f} MB moved "
            f"-> {rate(nbytes, med)} (best {nbytes / best / 1e9:.2f} TB/s)")
    say(f"  one layer, four launches: {tot_ms * 1e3:7.1f} us, {tot_bytes / 1e6:.1f} MB -> {rate(tot_bytes, tot_ms)}")
    say("yardsticks of the same process:")
    for k in ("wgu", "wd"):
        (N, K), _ = lin[k]
        src, dst = wv[k], torch.empty_like(wv[k])
        for _ in range(5):
            dst.copy_(src)
        med, best = timed(lambda: dst.copy_(src), a.reps)
        say(f"  device copy of {k} (bf16, read + write {4 * N * K / 1e6:.1f} MB): {med * 1e3:7.1f} us median -> {rate(4 * N * K, med)} "
            f"(best {4 * N * K / best / 1e9:.2f} TB/s)")
        del dst
    B, S = 4, 2048
    for N, pad in ((4096, 0), (14336, 64)):
        x = torch.randn(B * S, N + pad, generator=g, device=dev).bfloat16()[:, :N]
        y = torch.randn(B * S, N + pad, generator=g, device=dev).bfloat16()[:, :N]
        out = torch.empty(B, N, device=dev)
        for _ in range(5):
            ops.colsum_dot(x, y, B, S, out=out)
        med, best = timed(lambda: ops.colsum_dot(x, y, B, S, out=out), a.reps)
        say(f"  lrp_colsum_dot bf16 [8192, {N}] x 2 read ({4 * B * S * N / 1e6:.0f} MB): {med * 1e3:7.1f} us median -> {rate(4 * B * S * N, med)}")
        del x, y
    for k in ("wgu", "wd"):
        (N, K), _ = lin[k]
        x = torch.randn(8, K, generator=g, device=dev).bfloat16()
        out = torch.empty(8, N, device=dev, dtype=bf)
        for _ in range(5):
            ops.linear_fwd(x, wv[k], out=out)
        med, best = timed(lambda: ops.linear_fwd(x, wv[k], out=out), a.reps)
        say(f"  weight-streaming Linear M = 8 over {k} ({2 * N * K / 1e6:.1f} MB of weights read): {med * 1e3:7.1f} us median -> {rate(2 * N * K, med)}")
    del qv, wv

    # ---- (2) the step time, both engines in one process
    S = 2048
    W = bench.synth_weights(cfg, dev, bf, seed=0)
    plain = E.LlamaLRP(cfg, W, dtype=bf, device=dev, max_seq=S)
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated(dev)
    quant = E.LlamaLRP(cfg, W, dtype=bf, device=dev, max_seq=S, weight_format="mxfp4")
    torch.cuda.synchronize()
    added = torch.cuda.memory_allocated(dev) - m0          # (before the source weights go: they are not the engine's)
    del W
    torch.cuda.empty_cache()
    pb, qb = plain.weight_bytes(), quant.weight_bytes()
    say(f"weights, {a.layers} layers: ordinary engine {pb['resident'] / 1e9:.2f} GB resident; mxfp4 {qb['resident'] / 1e9:.2f} GB resident "
        f"({quant.flat_q.numel() / 1e9:.2f} GB of codes + scales, {quant.flat.numel() * 2 / 1e9:.2f} GB embedding / LM head / norms) + "
        f"{qb['scratch'] / 1e6:.1f} MB scratch layer; device memory the quantised engine added: {added / 1e9:.2f} GB")
    deq = E.LlamaLRP(*quant.dequantized_weights(), dtype=bf, device=dev, max_seq=S)          # the control: the quantised engine's operand data
    torch.cuda.empty_cache()
    engines = dict(none=plain, deq=deq, mxfp4=quant)
    for B in (4, 1):
        ids = torch.randint(0, cfg["vocab"], (B, S), generator=torch.Generator().manual_seed(1234)).to(dev)
        for eng in engines.values():                            # warm-up: every arena buffer, every kernel
            for _ in range(2):
                eng.explain(ids)
        torch.cuda.synchronize()
        ts = {k: [] for k in engines}
        for _ in range(a.rounds):
            for k, eng in engines.items():
                ts[k].append(timed(lambda: eng.explain(ids), a.steps)[0])
        base, ctl = statistics.median(ts["none"]), statistics.median(ts["deq"])
        say(f"step time, S = {S}, {B} prompt(s) per step, median of {a.rounds} rounds x {a.steps} steps, engines alternating:")
        for k in engines:
            m = statistics.median(ts[k])
            say(f"  {k:5s}: {m:8.2f} ms per step   vs none {m - base:+7.2f} ms ({100 * (m - base) / base:+5.1f} %)   vs deq {m - ctl:+7.2f} ms "
                f"({100 * (m - ctl) / ctl:+5.1f} %) = {(m - ctl) / (2 * a.layers) * 1e3:6.1f} us per layer and pass   "
                f"[spread {min(ts[k]):.2f} .. {max(ts[k]):.2f}]")

    # ---- (3) for the record: how far the 4-bit model's relevance is from the bf16 model's
    ids = torch.randint(0, cfg["vocab"], (a.prompts, S), generator=torch.Generator().manual_seed(99)).to(dev)
    rp = plain.explain(ids)
    idx, Rp = rp["idx"].clone(), rp["R_tok"].double().clone()
    rq = quant.explain(ids, target=idx)                        # the same logit explained by both
    Rq = rq["R_tok"].double()
    own = quant.explain(ids)["idx"]
    say(f"R_tok of the mxfp4 engine against the bf16 engine, {a.prompts} seeded prompts of the random-init model (the worst case: random weights "
        f"have no structure a block scale can follow), the bf16 engine's arg-max logit explained by both:")
    for b in range(a.prompts):
        cos = float((Rp[b] * Rq[b]).sum() / (Rp[b].norm() * Rq[b].norm()))
        say(f"  prompt {b}: cosine {cos:+.4f}, normalised max {float((Rq[b] - Rp[b]).abs().max() / Rp[b].abs().max()):.3f}; "
            f"arg-max logit {int(idx[b])} (bf16) / {int(own[b])} (mxfp4)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
